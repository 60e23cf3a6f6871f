"""NumPy restatement of shg_patch_ssd_u16 and shg_stack_combine_field_u16, written from the arithmetic include/shg_hip.h states, not
from the kernels, and of the host steps of local alignment in solex_ser_recon_en_amd/stack.py (align_lattice, measure_field,
fill_field, field_stats, local_fields) from their docstrings; what the two calls share with shg_shift_ssd_u16 and
shg_stack_combine_u16 comes from tests/stack_ref.py by import.  Also the synthetic series the accuracy is measured on -- three
frames of flatten_ref's scene with a texture, two of them bent along the scan --, the measures themselves and the bounds
(TOLERANCE)."""
import numpy as np

from tests import flatten_ref as fr
from tests import stack_ref as sr

EXTRA = 3                   # after a point's sums: the size of its set, the sum of ref and the sum of ref^2 over it
DEFAULTS = {'step': 16, 'size': 33, 'search': 4, 'region': 0.9, 'min_contrast': 0.0}


# ---- shg_patch_ssd_u16 ----
def patch_ssd(ref, img, points, half, search, circle=None):
    """uint64 [n, (2 S + 1)^2 + 3]: per point the sums over its set, then the size of the set, the sum of ref, the sum of ref^2."""
    ref, img = np.asarray(ref, dtype=np.uint16), np.asarray(img, dtype=np.uint16)
    assert ref.shape == img.shape
    h, w = ref.shape
    b, s = int(half), int(search)
    side = 2 * s + 1
    points = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((len(points), side * side + EXTRA), dtype=np.uint64)
    on = np.ones((h, w), dtype=bool)
    if circle is not None and tuple(float(t) for t in circle) != (-1.0, -1.0, -1.0):
        on = fr.rings(h, w, circle)[0]
    for p, (pr, pc) in enumerate(points):
        r_lo, r_hi = max(int(pr) - b, s), min(int(pr) + b, h - s - 1)
        c_lo, c_hi = max(int(pc) - b, s), min(int(pc) + b, w - s - 1)
        if r_lo > r_hi or c_lo > c_hi:
            continue
        mask = on[r_lo:r_hi + 1, c_lo:c_hi + 1]
        a = ref[r_lo:r_hi + 1, c_lo:c_hi + 1].astype(np.int64)
        for v in range(-s, s + 1):
            for u in range(-s, s + 1):
                d = a - img[r_lo + v:r_hi + 1 + v, c_lo + u:c_hi + 1 + u].astype(np.int64)
                out[p, (v + s) * side + (u + s)] = int((d * d)[mask].sum())
        out[p, side * side] = int(mask.sum())
        out[p, side * side + 1] = int(a[mask].sum())
        out[p, side * side + 2] = int((a * a)[mask].sum())
    return out


# ---- shg_stack_combine_field_u16 ----
def lattice_shape(shape, step):
    oh, ow = shape
    return (oh - 1 + step - 1) // step + 1, (ow - 1 + step - 1) // step + 1


def _cells(shape, step):
    """(gh, gw, j, j1, i, i1, fx, fy) of every pixel's cell: j = r // step, j1 = min(j + 1, gh - 1), fy = (r - j step) / step as a
    column, i, i1 and fx alike as a row."""
    oh, ow = shape
    gh, gw = lattice_shape(shape, step)
    r, c = np.arange(oh, dtype=np.int64), np.arange(ow, dtype=np.int64)
    j, i = r // step, c // step
    j1, i1 = np.minimum(j + 1, gh - 1), np.minimum(i + 1, gw - 1)
    fy = ((r - j * step).astype(np.float64) / np.float64(step))[:, None]
    fx = ((c - i * step).astype(np.float64) / np.float64(step))[None, :]
    return gh, gw, j, j1, i, i1, fx, fy


def displacement(field, shape, step):
    """(dx, dy) float64 [oh, ow] of a field [gh, gw, 2] at every pixel: j = r // step, j1 = min(j + 1, gh - 1), fy = (r - j step) /
    step, columns alike; per component top = a + (b - a) fx, bot = c + (d - c) fx, top + (bot - top) fy."""
    field = np.asarray(field, dtype=np.float64)
    gh, gw, j, j1, i, i1, fx, fy = _cells(shape, step)
    assert field.shape == (gh, gw, 2)
    out = []
    with np.errstate(invalid='ignore', over='ignore'):
        for k in (0, 1):
            a, b = field[j][:, i, k], field[j][:, i1, k]
            cc, d = field[j1][:, i, k], field[j1][:, i1, k]
            top = a + (b - a) * fx
            bot = cc + (d - cc) * fx
            out.append(top + (bot - top) * fy)
    return out[0], out[1]


def resample_field(src, xform, shape, field=None, step=None):
    """stack_ref.resample with a displacement: sx = tx + s (c + dx), sy = ty + s (r + dy); without a field sx = tx + s c,
    sy = ty + s r.  A displacement that is not finite fails the presence test."""
    src = np.asarray(src, dtype=np.uint16)
    h, w = src.shape
    s, tx, ty, gain = (np.float64(t) for t in xform)
    oh, ow = shape
    c = np.broadcast_to(np.arange(ow, dtype=np.float64)[None, :], (oh, ow))
    r = np.broadcast_to(np.arange(oh, dtype=np.float64)[:, None], (oh, ow))
    with np.errstate(invalid='ignore', over='ignore'):
        if field is not None:
            dx, dy = displacement(field, shape, step)
            c, r = c + dx, r + dy
        sx = tx + s * c
        sy = ty + s * r
        present = (sx >= 0.0) & (sx <= np.float64(w - 1)) & (sy >= 0.0) & (sy <= np.float64(h - 1))
        x0 = np.where(present, sx, 0.0).astype(np.int64)
        y0 = np.where(present, sy, 0.0).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        fx, fy = sx - x0.astype(np.float64), sy - y0.astype(np.float64)
        f = src.astype(np.float64)
        a, b, cc, d = f[y0, x0], f[y0, x1], f[y1, x0], f[y1, x1]
        top = a + (b - a) * fx
        bot = cc + (d - cc) * fx
        val = top + (bot - top) * fy
        v = val * gain
    return present, v


def stack_combine_field(srcs, xforms, fields, step, shape, mode, kappa=2.5, iterations=2):
    """(out uint16 [oh, ow], count uint8 [oh, ow])."""
    mode = sr.MODES.get(mode, mode)
    planes = [resample_field(src, xf, shape, f, step) for src, xf, f in zip(srcs, xforms, fields)]
    present = np.stack([p for p, _ in planes])
    v = np.stack([np.where(p, x, 0.0) for p, x in planes])           # (an absent sample is never read: its value may be anything)
    m, count = sr.combine_samples(present, v, mode, kappa, iterations)
    return sr.quantise(m), count.astype(np.uint8)


# ---- the host steps (stack.py) ----
def align_lattice(shape, step):
    gh, gw = lattice_shape(shape, step)
    return gh, gw, np.array([(j * step, i * step) for j in range(gh) for i in range(gw)], dtype=np.int32)


def measure_field(table, gh, gw, half, search, min_contrast=0.0):
    """(field float64 [gh, gw, 2], measured bool [gh, gw])."""
    n_off = (2 * search + 1) ** 2
    field, measured = np.zeros((gh, gw, 2), np.float64), np.zeros((gh, gw), bool)
    for p in range(gh * gw):
        row = [int(t) for t in table[p]]
        pixels, total, squares = row[n_off], row[n_off + 1], row[n_off + 2]
        if 2 * pixels < (2 * half + 1) ** 2:
            continue
        u, v, du, dv, _, _, rejected = sr.refine_offset(row[:n_off + 1], search)
        if rejected:
            continue
        if min_contrast > 0:
            mean = np.float64(total) / np.float64(pixels)
            var = np.float64(squares) / np.float64(pixels) - mean * mean
            with np.errstate(invalid='ignore', divide='ignore'):
                if np.sqrt(var) / mean < np.float64(min_contrast):
                    continue
        field[p // gw, p % gw] = (np.float64(u) + du, np.float64(v) + dv)
        measured[p // gw, p % gw] = True
    return field, measured


NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]           # row-major


def fill_field(field, measured):
    """Node by node: in each pass an unfilled node with a filled 8-neighbour takes their mean, added one at a time in row-major
    neighbour order from the state before the pass; until every node is filled.  Nothing measured: all zero."""
    field = np.array(field, dtype=np.float64)
    filled = np.array(measured, dtype=bool)
    gh, gw = filled.shape
    field[~filled] = 0.0
    if not filled.any():
        return field
    while not filled.all():
        before, had = field.copy(), filled.copy()
        for j in range(gh):
            for i in range(gw):
                if had[j, i]:
                    continue
                count, sx, sy = 0, np.float64(0.0), np.float64(0.0)
                for dj, di in NEIGHBOURS:
                    jj, ii = j + dj, i + di
                    if 0 <= jj < gh and 0 <= ii < gw and had[jj, ii]:
                        sx, sy, count = sx + before[jj, ii, 0], sy + before[jj, ii, 1], count + 1
                if count:
                    field[j, i, 0], field[j, i, 1], filled[j, i] = sx / np.float64(count), sy / np.float64(count), True
    return field


def field_stats(field, measured):
    total, worst, used = np.float64(0.0), np.float64(0.0), 0
    for j in range(measured.shape[0]):
        for i in range(measured.shape[1]):
            if measured[j, i]:
                d2 = field[j, i, 0] * field[j, i, 0] + field[j, i, 1] * field[j, i, 1]
                total, worst, used = total + d2, max(worst, d2), used + 1
    return {'points': int(measured.size), 'used': used, 'rms': float(np.sqrt(total / np.float64(used))) if used else 0.0,
            'max': float(np.sqrt(worst)) if used else 0.0}


def local_fields(images, records, circles, reference=0, step=16, size=33, search=4, region=0.9, min_contrast=0.0, want_measured=False):
    """stack.local_fields restated -> (fields, stats[, measured masks]), None for the reference and for a rejected frame."""
    cx0, cy0, rad0 = (np.float64(t) for t in circles[reference])
    shape = images[reference].shape
    disk = (float(cx0), float(cy0), float(np.float64(region) * rad0))
    half = (size - 1) // 2
    gh, gw, points = align_lattice(shape, step)
    fields, stats, masks = [], [], []
    for i, (img, rec) in enumerate(zip(images, records)):
        if i == reference or rec['rejected']:
            fields.append(None), stats.append(None), masks.append(None)
            continue
        plane = sr.stack_combine([img], [(rec['s'], rec['tx'], rec['ty'], rec['gain'])], shape, sr.MEAN)[0]
        raw, measured = measure_field(patch_ssd(images[reference], plane, points, half, search, disk), gh, gw, half, search, min_contrast)
        fields.append(fill_field(raw, measured)), stats.append(field_stats(raw, measured)), masks.append(measured)
    return (fields, stats, masks) if want_measured else (fields, stats)


def stack_series(images, circles, reference=0, mode='sigma', kappa=2.5, iterations=2, search=8, region=0.9, local=None):
    """stack.stack_scans from the disks on: (stack, count, records, fields, stats); local None: stack_ref.stack_series, no fields."""
    if local is None:
        return sr.stack_series(images, circles, reference, mode, kappa, iterations, search, region) + (None, None)
    local = dict(DEFAULTS, **local)
    records = sr.register_disks(images, circles, reference, search, region)
    fields, stats = local_fields(images, records, circles, reference, **local)
    used = [i for i, rec in enumerate(records) if not rec['rejected']]
    rows = [(records[i]['s'], records[i]['tx'], records[i]['ty'], records[i]['gain']) for i in used]
    out, count = stack_combine_field([images[i] for i in used], rows, [fields[i] for i in used], local['step'], images[reference].shape,
                                     mode, kappa, iterations)
    return out, count, records, fields, stats


# ---- the accuracy: three frames of flatten_ref's scene with a texture, frames 1 and 2 bent along the scan ----
FRAMES = 3                                                           # stack_ref.SERIES[0 .. 2]: centres, radii, gains, circle errors
TEXTURE_SIGMA, TEXTURE_STD, TEXTURE_SEED = 2.0, 0.05, 23
BEND, BEND_PERIOD = 1.5, 120.0                                       # dx = 1.5 sin(2 pi r / 120 + phi), dy = 1.5 cos(2 pi c / 120 + psi)
PHASES = [None, (0.3, 1.1), (2.0, 4.0)]
NOISE = 0.004


def texture():
    """t float64 [260, 250]: white noise through a Gaussian of sigma 2 px, scaled to a standard deviation of 0.05."""
    from scipy.ndimage import gaussian_filter                        # (the test helper only: the package does not need SciPy)
    t = gaussian_filter(np.random.default_rng(TEXTURE_SEED).standard_normal((fr.SCENE['h'], fr.SCENE['w'])), TEXTURE_SIGMA, mode='wrap')
    return t * (TEXTURE_STD / t.std())


def bend(i, r, c):
    """(dx, dy) of frame i at the frame's own (r, c)."""
    if PHASES[i] is None:
        return np.zeros_like(r + c), np.zeros_like(r + c)
    phi, psi = PHASES[i]
    return (BEND * np.sin(2.0 * np.pi * r / BEND_PERIOD + phi) + 0.0 * c, BEND * np.cos(2.0 * np.pi * c / BEND_PERIOD + psi) + 0.0 * r)


def frame_model(i, t=None):
    """The noise-free frame i on the relative scale (float64 [260, 250]): stack_ref.series_model's disk, spot and gain times
    (1 + t) on the disk, t sitting on the Sun (it moves and scales with the disk), drawn at (c - dx, r - dy)."""
    from scipy.ndimage import map_coordinates
    t = texture() if t is None else t
    h, w = fr.SCENE['h'], fr.SCENE['w']
    cx, cy, rad = sr.series_circle(i)
    cx0, cy0, rad0 = sr.series_circle(0)
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    dx, dy = bend(i, r, c)
    x, y = c - dx, r - dy                                            # where the undistorted frame is read
    rho = np.sqrt((x - cx) ** 2 + (y - cy) ** 2)
    scale = rad / rad0
    tex = map_coordinates(t, [cy0 + (y - cy) / scale, cx0 + (x - cx) / scale], order=3, mode='nearest')
    img = np.where(rho <= rad, fr.SCENE['scale'] * fr.law(rho / rad) * (1.0 + tex), fr.SCENE['sky'])
    width = 5.0 * sr.SERIES[i][2]
    img = img * (1.0 - 0.4 * np.exp(-0.5 * (((x - (cx + rad / 3.0)) / width) ** 2 + ((y - (cy - rad / 5.0)) / width) ** 2)))
    return img * sr.SERIES[i][3]


_SERIES = {}


def synthetic_series():
    """(images: three read-only uint16 [260, 250], the true circles, the circles handed to the registration); computed once."""
    if not _SERIES:
        t = texture()
        images, true, given = [], [], []
        for i in range(FRAMES):
            img = frame_model(i, t) + NOISE * np.random.default_rng([19, i]).standard_normal((fr.SCENE['h'], fr.SCENE['w']))
            img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
            img.setflags(write=False)
            images.append(img)
            true.append(sr.series_circle(i))
            ex, ey = sr.SERIES[i][4]
            given.append((true[i][0] + ex, true[i][1] + ey, true[i][2]))
        _SERIES.update(images=images, true=true, given=given, model=frame_model(0, t) * 65535.0)
    return _SERIES['images'], _SERIES['true'], _SERIES['given']


def true_displacement(i, record, points):
    """Where the reference's pixel (r, c) really lies in frame i, as a displacement against the record's transform: the point goes
    through the true similarity to p, the bend moves it to the q with q - d(q) = p (a fixed point, d is smooth), and
    (c + dx, r + dy) is q through the inverse of the record's transform -> float64 [n, 2] of (dx, dy)."""
    cx, cy, rad = sr.series_circle(i)
    cx0, cy0, rad0 = sr.series_circle(0)
    scale = rad / rad0
    r, c = points[:, 0].astype(np.float64), points[:, 1].astype(np.float64)
    px, py = cx + scale * (c - cx0), cy + scale * (r - cy0)
    qx, qy = px.copy(), py.copy()
    for _ in range(50):
        dx, dy = bend(i, qy, qx)
        qx, qy = px + dx, py + dy
    return np.stack([(qx - record['tx']) / record['s'] - c, (qy - record['ty']) / record['s'] - r], axis=1)


def series_measures(stack_of, fields_of):
    """The measures of the accuracy with the defaults.  stack_of(images, circles, local) -> (stack, count, records, ...) under MEAN;
    fields_of(images, records, circles) -> (fields, stats, measured masks).  -> {'rms', 'worst': the difference between measured
    and true displacement over the measured nodes of frames 1 and 2, px; 'rejected_inside': the unmeasured nodes whose whole patch
    lies within region rad_0; 'inside', 'used': how many nodes that is about; 'noise_local', 'noise_global': the standard deviation
    of stack - model of frame 0 within 0.8 R, counts of 65535; 'frame': the same of frame 0 alone}."""
    images, true, given = synthetic_series()
    model = _SERIES['model']
    step, half, region = DEFAULTS['step'], (DEFAULTS['size'] - 1) // 2, DEFAULTS['region']
    gh, gw, points = align_lattice(images[0].shape, step)
    on = fr.rings(*model.shape, (true[0][0], true[0][1], 0.8 * true[0][2]))[0]
    out = {'frame': float((images[0].astype(np.float64) - model)[on].std())}
    for key, local in (('noise_global', None), ('noise_local', {})):
        res = stack_of(images, given, local)
        out[key] = float((res[0].astype(np.float64) - model)[on].std())
        records = res[2]
    fields, stats, masks = fields_of(images, records, given)
    limit = region * given[0][2]
    corners = [np.hypot(points[:, 1] + sx * half - given[0][0], points[:, 0] + sy * half - given[0][1]) for sx in (-1, 1) for sy in (-1, 1)]
    inside = (np.max(corners, axis=0) <= limit).reshape(gh, gw)
    errors, rejected = [], 0
    for i in (1, 2):
        truth = true_displacement(i, records[i], points).reshape(gh, gw, 2)
        errors.append(np.hypot(*np.moveaxis(fields[i] - truth, 2, 0))[masks[i]])
        rejected += int((inside & ~masks[i]).sum())
    errors = np.concatenate(errors)
    out.update(rms=float(np.sqrt((errors ** 2).mean())), worst=float(errors.max()), rejected_inside=rejected, inside=int(inside.sum()),
               used=[s['used'] for s in stats[1:]], stats=stats[1:])
    return out


def patch_contrast(image, circle, step=16, size=33, region=0.9):
    """The contrast (standard deviation over mean) of the reference's patches that lie wholly within region rad: (least, median)."""
    half = (size - 1) // 2
    gh, gw, points = align_lattice(image.shape, step)
    table = patch_ssd(image, image, points, half, 0, (circle[0], circle[1], region * circle[2]))
    full = table[:, 1] == size * size
    n, total, squares = (table[full, k].astype(np.float64) for k in (1, 2, 3))
    contrast = np.sqrt(squares / n - (total / n) ** 2) / (total / n)
    return float(contrast.min()), float(np.median(contrast))


# What the restatement achieves on synthetic_series() with the defaults (step 16, size 33, search 4, region 0.9, MEAN; the global
# registration with search 8); tests/test_align_cpu.py re-measures and prints them.  Each bound is the measured value plus a
# quarter, rounded up to two significant digits; the quarter covers other seeds of the same scene.
#   displacement, measured against true over the 2 x 141 measured nodes of frames 1 and 2: rms 0.277360 px, worst 0.749487 px
#   (the true field, bend and what the global registration leaves, has an rms of 1.35 px and reaches 2.03 px);
#   none of the 2 x 93 nodes whose whole patch lies within 0.9 R is rejected;
#   noise, the standard deviation of stack - model of frame 0 within 0.8 R under MEAN against frame 0's own (261.35 counts):
#   0.541796 with the fields, 1.434797 with the global transforms alone -- three frames stacked without local alignment are
#   worse than one, because the bend moves the texture by more than its correlation length.
# The contrast of the reference's 93 whole patches (what --ap-min-contrast is compared with): 0.040 at least, median 0.062.
TOLERANCE = {'rms': 0.35, 'worst': 0.94, 'noise': 0.68}
