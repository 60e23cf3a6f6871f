"""NumPy restatement of shg_patch_sharpness_u16 and shg_stack_combine_weighted_u16, written from the arithmetic include/shg_hip.h
states, not from the kernels, and of the host steps of the quality ranking in solex_ser_recon_en_amd/stack.py (patch_quality,
disk_quality, local_quality, quality_weights, node_shares, select_scans and stack_scans' use of them) from their docstrings; what
the two calls share with the field combine and the registration comes from tests/align_ref.py and tests/stack_ref.py by import.
Also the synthetic series the accuracy is measured on -- the quadrant series: four frames of one geometry, each blurred in one
quadrant of the disk --, the measures themselves and the bound (TOLERANCE)."""
import numpy as np

from tests import align_ref as ar
from tests import flatten_ref as fr
from tests import stack_ref as sr

DEFAULTS = {'step': 16, 'size': 33, 'arm': 3, 'region': 0.9, 'best': None, 'min_quality': None, 'lucky': None, 'power': 0.0}


# ---- shg_patch_sharpness_u16 ----
def patch_sharpness(img, points, half, arm, circle=None):
    """uint64 [n, 4]: per point the size of its set, the sum of I, the sum of I^2 and the sum of L^2 over it."""
    img = np.asarray(img, dtype=np.uint16)
    h, w = img.shape
    b, d = int(half), int(arm)
    points = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((len(points), 4), dtype=np.uint64)
    on = np.ones((h, w), dtype=bool)
    if circle is not None and tuple(float(t) for t in circle) != (-1.0, -1.0, -1.0):
        on = fr.rings(h, w, circle)[0]
    f = img.astype(np.int64)
    for p, (pr, pc) in enumerate(points):
        r_lo, r_hi = max(int(pr) - b, d), min(int(pr) + b, h - d - 1)
        c_lo, c_hi = max(int(pc) - b, d), min(int(pc) + b, w - d - 1)
        if r_lo > r_hi or c_lo > c_hi:
            continue
        rows, cols = slice(r_lo, r_hi + 1), slice(c_lo, c_hi + 1)
        mask = on[rows, cols]
        a = f[rows, cols]
        lap = (4 * a - f[r_lo - d:r_hi + 1 - d, cols] - f[r_lo + d:r_hi + 1 + d, cols] - f[rows, c_lo - d:c_hi + 1 - d]
               - f[rows, c_lo + d:c_hi + 1 + d])
        out[p] = (int(mask.sum()), int(a[mask].sum()), int((a * a)[mask].sum()), int((lap * lap)[mask].sum()))
    return out


# ---- shg_stack_combine_weighted_u16 ----
def node_weight(lattice, shape, step):
    """w float64 [oh, ow] of a lattice [gh, gw] at every pixel: the cell of align_ref.displacement, top = a + (b - a) fx,
    bot = c + (d - c) fx, top + (bot - top) fy."""
    lattice = np.asarray(lattice, dtype=np.float64)
    gh, gw, j, j1, i, i1, fx, fy = ar._cells(shape, step)
    assert lattice.shape == (gh, gw)
    with np.errstate(invalid='ignore', over='ignore'):
        a, b = lattice[j][:, i], lattice[j][:, i1]
        cc, d = lattice[j1][:, i], lattice[j1][:, i1]
        top = a + (b - a) * fx
        bot = cc + (d - cc) * fx
        return top + (bot - top) * fy


def kept_samples(present, v, mode, kappa, iterations):
    """The kept set K bool [N, ...] of the present samples: all of them under MEAN; under SIGMA the clipping passes of
    shg_stack_combine_u16 (unweighted), with its rule for fewer than three samples and its rule for an empty K'."""
    kept = present.copy()
    if mode == sr.MEAN:
        return kept
    assert mode == sr.SIGMA
    active = present.sum(axis=0) >= 3
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for _ in range(int(iterations)):
            size = np.maximum(kept.sum(axis=0), 1).astype(np.float64)
            total = np.zeros(size.shape, dtype=np.float64)
            for j in range(v.shape[0]):
                total = total + np.where(kept[j], v[j], 0.0)
            m = total / size
            q = np.zeros(size.shape, dtype=np.float64)
            for j in range(v.shape[0]):
                dev = v[j] - m
                q = q + np.where(kept[j], dev * dev, 0.0)
            lim = np.float64(kappa) * np.sqrt(q / size)
            nxt = kept & (np.abs(v - m[None]) <= lim[None])
            change = active & nxt.any(axis=0) & (nxt != kept).any(axis=0)
            kept = np.where(change[None], nxt, kept)
            active = change & (kept.sum(axis=0) >= 3)
    return kept


def stack_combine_weighted(srcs, xforms, fields, weights, step, shape, mode, kappa=2.5, iterations=2):
    """(out uint16 [oh, ow], count uint8 [oh, ow]).  fields: None, or one entry a source."""
    mode = sr.MODES.get(mode, mode)
    assert mode in (sr.MEAN, sr.SIGMA)
    fields = [None] * len(srcs) if fields is None else fields
    present, v, w = [], [], []
    for src, xf, f, lattice in zip(srcs, xforms, fields, weights):
        p, x = ar.resample_field(src, xf, shape, f, step)
        ws = np.ones(shape, dtype=np.float64) if lattice is None else node_weight(lattice, shape, step)
        with np.errstate(invalid='ignore'):
            p = p & (ws > 0.0)
        present.append(p), v.append(np.where(p, x, 0.0)), w.append(np.where(p, ws, 0.0))
    present, v, w = np.stack(present), np.stack(v), np.stack(w)
    kept = kept_samples(present, v, mode, kappa, iterations)
    num, den = np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for j in range(len(srcs)):
            num = num + np.where(kept[j], w[j] * v[j], 0.0)
            den = den + np.where(kept[j], w[j], 0.0)
        count = kept.sum(axis=0)
        m = np.where(count > 0, num / np.where(count > 0, den, 1.0), 0.0)
    return sr.quantise(m), count.astype(np.uint8)


# ---- the host steps (stack.py) ----
def patch_quality(table, half):
    """q float64 [n], node by node: (float(sum L^2) float(n)) / (float(sum I) float(sum I)); NaN for a set below half a patch or dark."""
    q = np.full(len(table), np.nan, dtype=np.float64)
    for p, row in enumerate(table):
        n, total, _, lap = (int(t) for t in row)
        if 2 * n < (2 * half + 1) ** 2 or total == 0:
            continue
        q[p] = (np.float64(lap) * np.float64(n)) / (np.float64(total) * np.float64(total))
    return q


def disk_quality(image, circle, step=16, size=33, arm=3, region=0.9):
    half = (size - 1) // 2
    gh, gw, points = ar.align_lattice(image.shape, step)
    disk = (float(circle[0]), float(circle[1]), float(np.float64(region) * np.float64(circle[2])))
    qmap = patch_quality(patch_sharpness(image, points, half, arm, disk), half).reshape(gh, gw)
    finite = qmap[np.isfinite(qmap)]
    return {'map': qmap, 'quality': float(np.median(finite)) if finite.size else 0.0, 'nodes': int(finite.size)}


def local_quality(images, records, circles, reference, fields=None, step=16, size=33, arm=3, region=0.9):
    half = (size - 1) // 2
    gh, gw, points = ar.align_lattice(images[reference].shape, step)
    maps = []
    for i, (img, rec, circle) in enumerate(zip(images, records, circles)):
        if rec['rejected']:
            maps.append(None)
            continue
        s, tx, ty = np.float64(rec['s']), np.float64(rec['tx']), np.float64(rec['ty'])
        field = None if fields is None or fields[i] is None else np.asarray(fields[i], dtype=np.float64).reshape(gh * gw, 2)
        src = np.empty((gh * gw, 2), dtype=np.int64)
        for p, (r, c) in enumerate(points):
            dx, dy = (field[p, 0], field[p, 1]) if field is not None else (np.float64(0.0), np.float64(0.0))
            row = np.rint(ty + s * (np.float64(r) + dy))
            col = np.rint(tx + s * (np.float64(c) + dx))
            src[p] = (int(min(max(row, -2.0 ** 31), 2.0 ** 31 - 1.0)), int(min(max(col, -2.0 ** 31), 2.0 ** 31 - 1.0)))
        disk = (float(circle[0]), float(circle[1]), float(np.float64(region) * np.float64(circle[2])))
        maps.append(patch_quality(patch_sharpness(img, src, half, arm, disk), half).reshape(gh, gw))
    return maps


def node_order(qs):
    """The scans of one node, best first: q descending, ties to the lower index, NaN last."""
    return sorted(range(len(qs)), key=lambda k: (np.isnan(qs[k]), -qs[k] if not np.isnan(qs[k]) else 0.0, k))


def quality_weights(maps, keep=None, power=0.0):
    n = len(maps)
    gh, gw = maps[0].shape
    out = [np.zeros((gh, gw), dtype=np.float64) for _ in range(n)]
    for j in range(gh):
        for i in range(gw):
            qs = [np.float64(m[j, i]) for m in maps]
            if all(np.isnan(q) for q in qs):
                for k in range(n):
                    out[k][j, i] = 1.0
                continue
            order = node_order(qs)
            best = qs[order[0]]
            for rank, k in enumerate(order):
                w = np.float64(1.0 if keep is None or rank < keep else 0.0)
                if power > 0 and best > 0.0:
                    w = w * (np.float64(0.0) if np.isnan(qs[k]) else np.power(qs[k] / best, np.float64(power)))
                out[k][j, i] = w
    return out


def node_shares(maps):
    n = len(maps)
    wins, total = [0] * n, 0
    for j in range(maps[0].shape[0]):
        for i in range(maps[0].shape[1]):
            qs = [np.float64(m[j, i]) for m in maps]
            if not all(np.isnan(q) for q in qs):
                wins[node_order(qs)[0]] += 1
                total += 1
    return [wins[k] / total if total else 0.0 for k in range(n)]


def select_scans(qualities, best=None, min_quality=None):
    q = [np.float64(t) for t in qualities]
    keep = list(range(len(q)))
    if min_quality is not None:
        keep = [i for i in keep if q[i] >= np.float64(min_quality) * max(q)]
    if best is not None:
        if best < 2:
            raise ValueError('best < 2')
        keep = sorted(sorted(keep, key=lambda i: (-q[i], i))[:best])
    if len(keep) < 2:
        raise ValueError('fewer than two scans pass')
    return keep


def stack_series(images, circles, reference=0, mode='sigma', kappa=2.5, iterations=2, search=8, region=0.9, local=None, quality=None):
    """stack.stack_scans from the disks on -> {'stack', 'count', 'records', 'reference', 'used', 'unselected', 'figures', 'maps',
    'weights' (one a used scan, or None), 'shares'}."""
    if quality is None and reference != 'best':
        out, count, records, fields, _ = ar.stack_series(images, circles, reference, mode, kappa, iterations, search, region, local)
        return {'stack': out, 'count': count, 'records': records, 'reference': reference, 'figures': None}
    q = dict(DEFAULTS, **(quality or {}))
    if local is not None:
        local = dict(ar.DEFAULTS, **local)
        q['step'] = local['step']
    measured = [disk_quality(img, c, q['step'], q['size'], q['arm'], q['region']) for img, c in zip(images, circles)]
    figures = [m['quality'] for m in measured]
    if reference == 'best':
        reference = max(range(len(images)), key=lambda i: (figures[i], -i))
    records = sr.register_disks(images, circles, reference, search, region)
    used = [i for i, rec in enumerate(records) if not rec['rejected']]
    unselected = []
    if q['best'] is not None or q['min_quality'] is not None:
        keep = select_scans([figures[i] for i in used], q['best'], q['min_quality'])
        unselected = [i for k, i in enumerate(used) if k not in keep]
        used = [used[k] for k in keep]
    fields = None
    if local is not None:
        fields, _ = ar.local_fields(images, records, circles, reference, **local)
    rows = [(records[i]['s'], records[i]['tx'], records[i]['ty'], records[i]['gain']) for i in used]
    shape = images[reference].shape
    used_fields = None if fields is None else [fields[i] for i in used]
    weights = shares = None
    if q['lucky'] is not None or q['power'] > 0:
        maps = local_quality(images, records, circles, reference, fields, q['step'], q['size'], q['arm'], q['region'])
        maps = [maps[i] for i in used]
        weights, shares = quality_weights(maps, q['lucky'], q['power']), node_shares(maps)
        out, count = stack_combine_weighted([images[i] for i in used], rows, used_fields, weights, q['step'], shape, mode, kappa, iterations)
    elif fields is not None:
        out, count = ar.stack_combine_field([images[i] for i in used], rows, used_fields, local['step'], shape, mode, kappa, iterations)
    else:
        out, count = sr.stack_combine([images[i] for i in used], rows, shape, mode, kappa, iterations)
    return {'stack': out, 'count': count, 'records': records, 'reference': reference, 'used': used, 'unselected': unselected,
            'figures': figures, 'maps': [m['map'] for m in measured], 'weights': weights, 'shares': shares}


# ---- the accuracy: the quadrant series ----
FRAMES = 4
BLUR_SIGMA, MASK_SIGMA, NOISE_SEED = 1.5, 6.0, 31
AXIS_MARGIN = 24.0                                                   # a node counts when it is further than this from both axes
IDENTITY = {'s': 1.0, 'tx': 0.0, 'ty': 0.0, 'gain': 1.0, 'rejected': False}

_QUADRANTS = {}


def quadrant_of(r, c, circle):
    """0 .. 3: above-left, above-right, below-left, below-right of the disk's centre."""
    return 2 * (np.asarray(r) >= circle[1]).astype(np.int64) + (np.asarray(c) >= circle[0]).astype(np.int64)


def quadrant_series():
    """(images: four read-only uint16 [260, 250], the circle of all four, the noise-free model in counts); computed once.  All four
    are align_ref.frame_model(0); frame i is blurred by a Gaussian of sigma 1.5 px inside quadrant i about the disk's centre, the
    quadrant's mask smoothed by a Gaussian of sigma 6 px, and then takes noise align_ref.NOISE with the seed [31, i]."""
    if not _QUADRANTS:
        from scipy.ndimage import gaussian_filter                    # (the test helper only: the package does not need SciPy)
        model = ar.frame_model(0)
        circle = sr.series_circle(0)
        h, w = model.shape
        soft = gaussian_filter(model, BLUR_SIGMA, mode='nearest')
        quadrant = quadrant_of(np.arange(h)[:, None], np.arange(w)[None, :], circle)
        images = []
        for i in range(FRAMES):
            mask = gaussian_filter((quadrant == i).astype(np.float64), MASK_SIGMA, mode='nearest')
            img = model * (1.0 - mask) + soft * mask + ar.NOISE * np.random.default_rng([NOISE_SEED, i]).standard_normal((h, w))
            img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
            img.setflags(write=False)
            images.append(img)
        _QUADRANTS.update(images=images, circle=circle, model=model * 65535.0)
    return _QUADRANTS['images'], _QUADRANTS['circle'], _QUADRANTS['model']


def quadrant_measures(local_quality_of, stack_of):
    """The measures with the defaults (arm 3, step 16, size 33, region 0.9).  local_quality_of(images, records, circles, reference)
    -> the maps; stack_of(images, records, weights or None, step) -> (stack, count) under MEAN, being the implementation under
    measurement -> {'nodes': the nodes that are valid in every frame and further than 24 px from both axes; 'last': at how many of
    them the blurred frame ranks last; 'lucky', 'all', 'frame': the standard deviation of stack - model within 0.8 R for best-3-of-4
    a node, for the plain mean of all four and for frame 0 alone, counts; 'ratio': lucky / all; 'maps', 'weights', 'stack'}."""
    images, circle, model = quadrant_series()
    step = DEFAULTS['step']
    records, circles = [dict(IDENTITY) for _ in images], [circle] * FRAMES
    maps = local_quality_of(images, records, circles, 0)
    gh, gw, points = ar.align_lattice(images[0].shape, step)
    q = np.stack(maps).reshape(FRAMES, gh * gw)
    valid = np.isfinite(q).all(axis=0)
    valid &= (np.abs(points[:, 0] - circle[1]) > AXIS_MARGIN) & (np.abs(points[:, 1] - circle[0]) > AXIS_MARGIN)
    blurred = quadrant_of(points[:, 0], points[:, 1], circle)
    last = sum(1 for p in np.nonzero(valid)[0] if node_order(list(q[:, p]))[-1] == blurred[p])
    weights = quality_weights(maps, FRAMES - 1, 0.0)
    on = fr.rings(*model.shape, (circle[0], circle[1], 0.8 * circle[2]))[0]
    lucky, count = stack_of(images, records, weights, step)
    plain, _ = stack_of(images, records, None, step)
    out = {'nodes': int(valid.sum()), 'last': int(last), 'maps': maps, 'weights': weights, 'stack': lucky, 'count': count,
           'lucky': float((lucky.astype(np.float64) - model)[on].std()), 'all': float((plain.astype(np.float64) - model)[on].std()),
           'frame': float((images[0].astype(np.float64) - model)[on].std())}
    out['ratio'] = out['lucky'] / out['all']
    return out


def restated_measures():
    """quadrant_measures of the restatement itself; computed once."""
    if 'measures' not in _QUADRANTS:
        rows = [(1.0, 0.0, 0.0, 1.0)] * FRAMES

        def stack_of(images, records, weights, step):
            if weights is None:
                return sr.stack_combine(images, rows, images[0].shape, sr.MEAN)
            return stack_combine_weighted(images, rows, None, weights, step, images[0].shape, sr.MEAN)

        _QUADRANTS['measures'] = quadrant_measures(lambda *a: local_quality(*a), stack_of)
    return _QUADRANTS['measures']


# What the restatement achieves on quadrant_series() with the defaults (arm 3, step 16, size 33, region 0.9, MEAN);
# tests/test_quality_cpu.py re-measures and prints them.
#   at all 72 nodes that are valid in every frame and further than 24 px from both axes the blurred frame ranks last;
#   the residual against the noise-free model within 0.8 R: 153.090 counts for best-3-of-4 a node, 178.744 for the plain mean of all
#   four -- a ratio of 0.856475 --, 343.516 for frame 0 alone (its blurred quadrant included).
# 'lucky': the bound on that ratio is the measured ratio plus a quarter of its distance to 1 (0.892356), rounded up to two digits.
TOLERANCE = {'lucky': 0.90}
