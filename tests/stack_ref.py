"""NumPy restatement of shg_stack_combine_u16 and shg_shift_ssd_u16, written from the arithmetic include/shg_hip.h states, not from
the kernels, and of the host registration step of solex_ser_recon_en_amd/stack.py from its docstrings.  Every per-pixel step is
float64 with one NumPy operation a step; where order matters -- the in-order sums and the clipping passes -- a Python loop walks the
sources in their order, one addition at a time (a sample that is absent or not kept adds +0.0 to a sum that is >= +0, which changes
no bit).  Also the synthetic series the accuracy is measured on, the measures themselves and the bounds (TOLERANCE)."""
import numpy as np

from tests import flatten_ref as fr

MEAN, MEDIAN, SIGMA = 0, 1, 2
MODES = {'mean': MEAN, 'median': MEDIAN, 'sigma': SIGMA}


# ---- shg_stack_combine_u16 ----
def resample(src, xform, shape):
    """(present bool [oh, ow], v float64 [oh, ow]) of one source: sx = tx + s c, sy = ty + s r; present iff 0 <= sx <= w - 1 and
    0 <= sy <= h - 1; bilinear as top = a + (b - a) fx, bot = c + (d - c) fx, val = top + (bot - top) fy; v = val gain."""
    src = np.asarray(src, dtype=np.uint16)
    h, w = src.shape
    s, tx, ty, gain = (np.float64(t) for t in xform)
    oh, ow = shape
    c = np.arange(ow, dtype=np.float64)[None, :]
    r = np.arange(oh, dtype=np.float64)[:, None]
    sx = np.broadcast_to(tx + s * c, (oh, ow))
    sy = np.broadcast_to(ty + s * r, (oh, ow))
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
    with np.errstate(over='ignore'):
        v = val * gain
    return present, v


def _sum_in_order(v, mask):
    acc = np.zeros(v.shape[1:], dtype=np.float64)
    for j in range(v.shape[0]):
        acc = acc + np.where(mask[j], v[j], 0.0)
    return acc


def combine_samples(present, v, mode, kappa=2.5, iterations=2):
    """present bool [N, ...], v float64 [N, ...] -> (m float64 [...] (0 where no sample is present), count int64 [...])."""
    present = np.asarray(present, dtype=bool)
    v = np.asarray(v, dtype=np.float64)
    n = present.sum(axis=0)
    some = n > 0
    safe_n = np.where(some, n, 1).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if mode == MEAN:
            return np.where(some, _sum_in_order(v, present) / safe_n, 0.0), n
        if mode == MEDIAN:
            ordered = np.sort(np.where(present, v, np.inf), axis=0)
            lo = np.take_along_axis(ordered, (np.maximum(n - 1, 0) // 2)[None], axis=0)[0]
            hi = np.take_along_axis(ordered, (n // 2)[None], axis=0)[0]
            return np.where(some, (lo + hi) / 2.0, 0.0), n
        assert mode == SIGMA
        kept = present.copy()
        active = n >= 3
        for _ in range(int(iterations)):
            size = np.where(some, kept.sum(axis=0), 1).astype(np.float64)
            m = _sum_in_order(v, kept) / size
            q = np.zeros(m.shape, dtype=np.float64)
            for j in range(v.shape[0]):
                dev = v[j] - m
                q = q + np.where(kept[j], dev * dev, 0.0)
            lim = np.float64(kappa) * np.sqrt(q / size)
            nxt = kept & (np.abs(v - m[None]) <= lim[None])
            change = active & nxt.any(axis=0) & ~(nxt == kept).all(axis=0)
            kept = np.where(change[None], nxt, kept)
            active = change & (kept.sum(axis=0) >= 3)
        count = kept.sum(axis=0)
        return np.where(some, _sum_in_order(v, kept) / np.where(some, count, 1).astype(np.float64), 0.0), count


def quantise(m):
    with np.errstate(invalid='ignore'):
        return np.clip(np.rint(m), 0.0, 65535.0).astype(np.uint16)


def stack_combine(srcs, xforms, shape, mode, kappa=2.5, iterations=2):
    """(out uint16 [oh, ow], count uint8 [oh, ow])."""
    mode = MODES.get(mode, mode)
    planes = [resample(src, xf, shape) for src, xf in zip(srcs, xforms)]
    present = np.stack([p for p, _ in planes])
    v = np.stack([x for _, x in planes])
    m, count = combine_samples(present, v, mode, kappa, iterations)
    return quantise(m), count.astype(np.uint8)


# ---- shg_shift_ssd_u16 ----
def shift_ssd(ref, img, search, circle=None):
    """uint64 [(2 S + 1)^2 + 1]: the sums over the set, then the size of the set."""
    ref, img = np.asarray(ref, dtype=np.uint16), np.asarray(img, dtype=np.uint16)
    assert ref.shape == img.shape
    h, w = ref.shape
    s = int(search)
    side = 2 * s + 1
    out = np.zeros(side * side + 1, dtype=np.uint64)
    if w < side or h < side:
        return out
    on = np.ones((h, w), dtype=bool)
    if circle is not None and tuple(float(t) for t in circle) != (-1.0, -1.0, -1.0):
        on = fr.rings(h, w, circle)[0]
    on = on[s:h - s, s:w - s]
    a = ref[s:h - s, s:w - s].astype(np.int64)
    for v in range(-s, s + 1):
        for u in range(-s, s + 1):
            d = a - img[s + v:h - s + v, s + u:w - s + u].astype(np.int64)
            out[(v + s) * side + (u + s)] = int((d * d)[on].sum())
    out[side * side] = int(on.sum())
    return out


# ---- the host registration step (stack.py) ----
def parabola_offset(e_minus, e_0, e_plus):
    e_minus, e_0, e_plus = np.float64(e_minus), np.float64(e_0), np.float64(e_plus)
    den = (e_minus - np.float64(2.0) * e_0) + e_plus
    if not den > 0.0:
        return np.float64(0.0)
    return (np.float64(0.5) * (e_minus - e_plus)) / den


def refine_offset(ssd, search):
    """(u, v, du, dv, the minimum, the pixels, rejected): the first minimum in row-major order, a parabola an axis."""
    s = int(search)
    side = 2 * s + 1
    sums = [int(t) for t in ssd[:side * side]]
    pixels = int(ssd[side * side])
    k = min(range(side * side), key=lambda i: (sums[i], i))
    iv, iu = k // side, k % side
    border = s >= 1 and (iu == 0 or iu == side - 1 or iv == 0 or iv == side - 1)
    du = dv = np.float64(0.0)
    if s >= 1 and not border:
        du = parabola_offset(float(sums[k - 1]), float(sums[k]), float(sums[k + 1]))
        dv = parabola_offset(float(sums[k - side]), float(sums[k]), float(sums[k + side]))
    return iu - s, iv - s, du, dv, sums[k], pixels, bool(border or pixels == 0)


def disk_level(img, circle):
    """np.median of the first max(1, K // 10) ring medians, the empty rings filled from the nearest ring that has pixels."""
    profile = fr.profile_of(*fr.ring_medians(img, circle))
    count, med = profile['count'], profile['median']
    have = [i for i in range(len(med)) if count[i] > 0]
    if not have:
        raise ValueError('no ring holds a pixel')
    filled = [med[i] if count[i] > 0 else med[min(have, key=lambda q: (abs(q - i), q))] for i in range(len(med))]
    return np.float64(np.median(np.array(filled[:max(1, len(med) // 10)], dtype=np.float64)))


def register_disks(images, circles, reference=0, search=8, region=0.9):
    """stack.register_disks restated: records of (s, tx, ty, gain, offset (u + du, v + dv), ssd per pixel, pixels, rejected)."""
    levels = [disk_level(img, c) for img, c in zip(images, circles)]
    if any(not lv > 0 for lv in levels):
        raise ValueError('a brightness level of 0')
    cx0, cy0, rad0 = (np.float64(t) for t in circles[reference])
    shape = images[reference].shape
    disk = (float(cx0), float(cy0), float(np.float64(region) * rad0))
    records = []
    for i, (img, circle) in enumerate(zip(images, circles)):
        if i == reference:
            records.append({'s': 1.0, 'tx': 0.0, 'ty': 0.0, 'gain': 1.0, 'offset': (0.0, 0.0), 'ssd_per_pixel': 0.0, 'pixels': None,
                            'rejected': False})
            continue
        cx, cy, rad = (np.float64(t) for t in circle)
        s = rad / rad0
        tx, ty = cx - s * cx0, cy - s * cy0
        gain = levels[reference] / levels[i]
        plane = stack_combine([img], [(s, tx, ty, gain)], shape, MEAN)[0]
        u, v, du, dv, least, pixels, rejected = refine_offset(shift_ssd(images[reference], plane, search, disk), search)
        records.append({'s': float(s), 'tx': float(tx + s * (np.float64(u) + du)), 'ty': float(ty + s * (np.float64(v) + dv)),
                        'gain': float(gain), 'offset': (u + float(du), v + float(dv)),
                        'ssd_per_pixel': least / pixels if pixels else float('nan'), 'pixels': pixels, 'rejected': rejected})
    return records


def stack_series(images, circles, reference=0, mode='sigma', kappa=2.5, iterations=2, search=8, region=0.9):
    """stack.stack_scans from the disks on: (stack, count, records), the rejected frames left out."""
    records = register_disks(images, circles, reference, search, region)
    used = [i for i, rec in enumerate(records) if not rec['rejected']]
    rows = [(records[i]['s'], records[i]['tx'], records[i]['ty'], records[i]['gain']) for i in used]
    out, count = stack_combine([images[i] for i in used], rows, images[reference].shape, mode, kappa, iterations)
    return out, count, records


# ---- the accuracy: a series of five synthetic disks of flatten_ref's scene ----
# (dx, dy: the centre against the scene's, px; the radius against the scene's; the gain; the error of the circle handed to the
# registration, px -- the limb fit's, which the search has to take out again)
SERIES = [(0.0, 0.0, 1.000, 1.00, (0.0, 0.0)),
          (2.37, -1.62, 1.007, 0.80, (1.3, -0.8)),
          (-2.81, 0.44, 0.992, 1.20, (-1.6, 1.1)),
          (1.05, 2.93, 1.010, 0.90, (0.7, 1.9)),
          (-0.58, -2.26, 0.990, 1.10, (-1.9, -1.4))]
NOISE = 0.004
STREAK_FRAME, STREAK_ROWS, STREAK_GAIN = 3, (150, 152), 1.5      # a trail two rows high, half as bright again, across frame 3


def series_circle(i):
    cx, cy, rad = fr.SCENE['circle']
    dx, dy, scale, _, _ = SERIES[i]
    return (cx + dx, cy + dy, rad * scale)


def series_model(i, gain=None):
    """The noise-free frame i on the relative scale (float64 [260, 250]), without the streak."""
    h, w = fr.SCENE['h'], fr.SCENE['w']
    cx, cy, rad = series_circle(i)
    gain = SERIES[i][3] if gain is None else gain
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    rho = np.sqrt((c - cx) ** 2 + (r - cy) ** 2)
    img = np.where(rho <= rad, fr.SCENE['scale'] * fr.law(rho / rad), fr.SCENE['sky'])
    width = 5.0 * SERIES[i][2]                                       # the spot sits on the sun: it moves and scales with the disk
    img = img * (1.0 - 0.4 * np.exp(-0.5 * (((c - (cx + rad / 3.0)) / width) ** 2 + ((r - (cy - rad / 5.0)) / width) ** 2)))
    return img * gain


def synthetic_series(noise=NOISE, streak=True):
    """(images: five uint16 [260, 250], the true circles, the circles handed to the registration)."""
    images, true, given = [], [], []
    for i in range(len(SERIES)):
        img = series_model(i)
        if streak and i == STREAK_FRAME:
            img[STREAK_ROWS[0]:STREAK_ROWS[1], :] *= STREAK_GAIN
        img = img + noise * np.random.default_rng([17, i]).standard_normal(img.shape)
        images.append(np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16))
        circle = series_circle(i)
        true.append(circle)
        ex, ey = SERIES[i][4]
        given.append((circle[0] + ex, circle[1] + ey, circle[2]))
    return images, true, given


def registration_error(record, true_circle, true_ref):
    """The worst distance, over the reference disk's centre and the four ends of its axes, between where the record's transform and
    where the true one put that point in the frame, px."""
    s_true = true_circle[2] / true_ref[2]
    worst = 0.0
    for px, py in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
        c, r = true_ref[0] + px * true_ref[2], true_ref[1] + py * true_ref[2]
        want = (true_circle[0] + s_true * (c - true_ref[0]), true_circle[1] + s_true * (r - true_ref[1]))
        got = (record['tx'] + record['s'] * c, record['ty'] + record['s'] * r)
        worst = max(worst, float(np.hypot(got[0] - want[0], got[1] - want[1])))
    return worst


SERIES_KAPPA = 1.5          # among n samples none lies further than (n - 1) / sqrt(n) standard deviations from their mean: 1.79 for
#                             five frames, so the default kappa of 2.5 rejects nothing below nine frames and the series is clipped at 1.5


def series_measures(stack_of):
    """The measures of the accuracy, stack_of(images, circles, mode) -> (stack, count, records), at kappa = SERIES_KAPPA and two
    passes, being the implementation under measurement -> {'registration': the worst registration error, px; 'noise': the standard deviation of stack - model over the
    reference disk within 0.9 R (the streak's rows left out) against the reference frame's own; 'streak_sigma', 'streak_mean': the
    mean of (stack - model) / model over the streak's pixels within 0.9 R; 'rejected': frames the search rejected}."""
    images, true, given = synthetic_series()
    model = series_model(0) * 65535.0
    on = fr.rings(*model.shape, (true[0][0], true[0][1], 0.9 * true[0][2]))[0]
    # where frame 3's streak lands on the reference grid: its rows through the true transform, a row of margin either way
    s = true[STREAK_FRAME][2] / true[0][2]
    ty = true[STREAK_FRAME][1] - s * true[0][1]
    rows = np.arange(model.shape[0], dtype=np.float64)
    src_rows = ty + s * rows
    near = (src_rows > STREAK_ROWS[0] - 2.0) & (src_rows < STREAK_ROWS[1] + 1.0)
    core = (src_rows >= STREAK_ROWS[0]) & (src_rows <= STREAK_ROWS[1] - 1.0)
    quiet, trail = on & ~near[:, None], on & core[:, None]
    out = {}
    for mode in ('sigma', 'mean'):
        stack, _, records = stack_of(images, given, mode)
        resid = stack.astype(np.float64) - model
        out['streak_' + mode] = float((resid[trail] / model[trail]).mean())
        if mode == 'sigma':
            out['noise'] = float(resid[quiet].std() / (images[0].astype(np.float64) - model)[quiet].std())
            out['registration'] = max(registration_error(records[i], true[i], true[0]) for i in range(1, len(images)))
            out['rejected'] = [i for i, rec in enumerate(records) if rec['rejected']]
            out['offsets'] = [rec['offset'] for rec in records]
    return out


# What the restatement achieves on synthetic_series() (sigma: kappa SERIES_KAPPA, two passes; search 8; region 0.9);
# tests/test_stack_cpu.py re-measures and prints them.  Each bound is the measured value plus a quarter, rounded up to two
# significant digits; the quarter covers other seeds of the same scene.
#   registration 0.157714 px; noise 0.410598 of a single frame's (1 / sqrt(5) = 0.447: the bilinear resampling smooths the four
#   frames it moves); the streak, 50 % in its frame: 0.101508 of the disk under 'mean' (a fifth), 0.001736 under 'sigma'
# 'pipeline': the noise measure on pipeline_series() -- three scans, so 1 / sqrt(3) = 0.577 at best --, the disks and circles
# oracle/pipeline_oracle.py makes of them stacked by the restatement with the defaults; the measure is difference_noise, which
# needs no model (the limb fits of the three scans differ by 1 % in radius, and so do the scales: no model fits all three):
#   noise 0.471342 of the reference frame's (below 0.577: the resampling smooths the two frames it moves)
TOLERANCE = {'registration': 0.20, 'noise': 0.52, 'streak_sigma': 0.0022, 'streak_mean': 0.13, 'pipeline': {'noise': 0.59}}


# ---- three small scans of one scene, for the end-to-end test ----
PIPELINE = {'n': 300, 'ih': 400, 'iw': 32, 'moves': [(0.0, 0.0), (3.0, -2.0), (-2.0, 4.0)]}     # (frames, rows) each scan's disk is moved by


def pipeline_series(noise=0.004):
    """Three scans (file layout, uint16 [300, 32, 400]) of synth's scene with one spot, their disks moved by a few frames and rows,
    each with its own noise seed."""
    from solex_ser_recon_en_amd import synth
    n, ih, iw = PIPELINE['n'], PIPELINE['ih'], PIPELINE['iw']
    base = synth.scene_params(n, ih, iw)

    def scan(move, seed, level):
        cx, cy = base['cx'] + move[0], base['cy'] + move[1]
        scene = {'cx': cx, 'cy': cy, 'noise': level, 'spots': [(cx + 30.0, cy - 45.0, 6.0, 6.0, 0.4)]}
        return synth.synth_frames_numpy(n, ih, iw, 16, seed=seed, scene=scene)

    return [scan(move, 11 + i, noise) for i, move in enumerate(PIPELINE['moves'])]


def difference_noise(img, circle):
    """A noise measure that needs no model: the standard deviation of the differences of horizontal neighbours, over sqrt(2), on
    the disk within 0.9 R of `circle` (the scene's own gradients are small against the noise there; the spot adds to every image
    alike)."""
    on = fr.rings(*img.shape, (circle[0], circle[1], 0.9 * circle[2]))[0]
    d = img[:, 1:].astype(np.float64) - img[:, :-1].astype(np.float64)
    return float(d[on[:, 1:] & on[:, :-1]].std() / np.sqrt(2.0))


def pipeline_noise(stack, ref_image, circle):
    """difference_noise of the stack against the reference frame's own."""
    return difference_noise(stack, circle) / difference_noise(ref_image, circle)
