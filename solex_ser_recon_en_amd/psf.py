"""Measure the blur from the limb: the width of the point-spread function along the image's two axes, read off
the one knife edge every disk carries -- the limb, whose circle the pipeline already fits.  Across an edge with the normal
(cos theta, sin theta) a separable Gaussian (sigma_x, sigma_y) leaves a Gaussian edge spread of
sigma(theta)^2 = sigma_x^2 cos^2 theta + sigma_y^2 sin^2 theta: the width a sector of the limb gives both from one linear regression.
The pass over the image is a HIP kernel that leaves exact integer tables (ops.limb_profile_u16, stated in include/shg_hip.h); the fit
of an edge a sector and the regression are host NumPy in float64, deterministic.

    python -m solex_ser_recon_en_amd.psf INPUT [--shift S] [--circle cx,cy,rad] [--reach Q] [--sub N] [--sectors S] [SHG_MAIN flags]

A pixel integrates over its own area, so the widths come out with 1 / sqrt(12) px an axis in them: they are returned as measured,
because that is the blur the image has and the one deconvolve has to invert.  In H-alpha the limb is a spicule forest and not a step:
there the estimate is an upper bound; it is tightest in a photospheric wing or in the continuum.  Out of scope: point-spread
functions that are not separable or not Gaussian, a blur that varies across the disk, any edge but the limb, an ellipse.
"""
import argparse
import math
import os
import sys
import time

import numpy as np

DEFAULT_REACH, DEFAULT_SUB, DEFAULT_SECTORS = 12, 4, 32
SIGMA_GRID = np.round(np.arange(0.3, 5.0 + 1e-9, 0.1), 10)        # the widths tried, in pixels
T0_REACH, GRID = 1.5, 16                                           # the edge may sit +- 1.5 px off the circle; tables on a 1/16 px grid
T0_GRID = np.arange(-int(T0_REACH * GRID), int(T0_REACH * GRID) + 1, dtype=np.float64) / GRID
MAX_EMPTY = 0.10                     # a sector with more than this fraction of empty bins leaves the image
OUTLIER_SIGMAS, OUTLIER_FLOOR = 3.0, 0.05        # a sector whose sigma^2 is beyond 3 robust sigma of the regression; the robust sigma is
                                                 # at least 0.05 of the median sigma^2 (an exact fit has no scatter to go by)
MAX_CONDITION = 100.0                # of the regression's 2 x 2 normal matrix: beyond it the sectors do not span both axes
MIN_SECTORS = 3


def limb_profiles(image, circle, reach=DEFAULT_REACH, sub=DEFAULT_SUB, sectors=DEFAULT_SECTORS):
    """The edge-spread tables of the uint16 image around `circle` (cx, cy, rad), ops.limb_profile_u16's, as host arrays ->
    (count uint32, sum uint64, sumsq uint64, each [sectors, 2 reach sub], t float64 [2 reach sub]): t = (b + 1/2) / sub - reach is
    the distance of bin b's centre from the circle, negative on the disk."""
    import torch
    from . import ops
    from .device import to_device_u16
    count, total, sumsq = ops.limb_profile_u16(to_device_u16(image), circle, reach, sub, sectors)
    host = [count.view(torch.int32).cpu().numpy().view(np.uint32)] + \
           [t.view(torch.int64).cpu().numpy().view(np.uint64) for t in (total, sumsq)]
    return host[0], host[1], host[2], bin_centres(reach, sub)


def bin_centres(reach, sub):
    return (np.arange(2 * int(reach) * int(sub), dtype=np.float64) + 0.5) / float(sub) - float(reach)


def sector_angles(sectors):
    """The middle of every sector: (s + 1/2) 2 pi / S, from the +column axis towards the +row axis."""
    return (np.arange(int(sectors), dtype=np.float64) + 0.5) * (2.0 * np.pi / int(sectors))


_ERF = np.vectorize(math.erf, otypes=[np.float64])
_BASES = {}


def _bases(span):
    """The two blurred bases for every width of SIGMA_GRID on the grid u = j / 16, |u| <= span: the step (1 on the disk, u < 0) under
    a Gaussian -- erfc(u / (sigma sqrt 2)) / 2 -- and sqrt(max(-u, 0)) under it, summed on the same grid from the square root's
    exact mean over every 1/16 px cell.  -> (u [n], step [n_sigma, n], root [n_sigma, n]); tabulated once a span."""
    if span not in _BASES:
        n = int(math.ceil(span * GRID))
        u = np.arange(-n, n + 1, dtype=np.float64) / GRID
        half = 0.5 / GRID
        wide = np.arange(-n - 6 * GRID * 5, n + 6 * GRID * 5 + 1, dtype=np.float64) / GRID       # 6 of the widest sigma to either side
        antiderivative = lambda y: -(2.0 / 3.0) * np.maximum(-y, 0.0) ** 1.5                      # of sqrt(max(-y, 0))
        cell = (antiderivative(wide + half) - antiderivative(wide - half)) * GRID
        step = np.empty((SIGMA_GRID.size, u.size))
        root = np.empty((SIGMA_GRID.size, u.size))
        for k, sigma in enumerate(SIGMA_GRID):
            step[k] = 0.5 * (1.0 - _ERF(u / (sigma * math.sqrt(2.0))))
            m = int(math.ceil(6.0 * sigma * GRID))
            x = np.arange(-m, m + 1, dtype=np.float64) / GRID
            g = np.exp(-(x * x) / (2.0 * sigma * sigma))
            root[k] = np.convolve(cell, g / g.sum(), mode='same')[(wide.size - u.size) // 2:(wide.size + u.size) // 2]
        _BASES[span] = (u, step, root)
    return _BASES[span]


def _parabola(below, at, above):
    """The minimum of the parabola through three equally spaced values with the middle one lowest -> (its offset in steps, within
    +- 1/2; its value)."""
    curve = below - 2.0 * at + above
    if not curve > 0.0:
        return 0.0, at
    x = 0.5 * (below - above) / curve
    x = min(max(x, -0.5), 0.5)
    return x, at - 0.125 * (below - above) ** 2 / curve


def fit_edges(t, mean, count):
    """fit_edge for every row of mean and count [sectors, bins] at once -> (sigma, t0, residual, on_edge), arrays [sectors]; a row
    without three counted bins comes back as nan, nan, nan, True."""
    t = np.asarray(t, dtype=np.float64)
    mean = np.atleast_2d(np.asarray(mean, dtype=np.float64))
    w = np.atleast_2d(np.asarray(count, dtype=np.float64))
    n_sec, n_bins = mean.shape
    u, step, root = _bases(float(math.ceil(np.abs(t).max() + T0_REACH + 1.0)))
    # the bases at t - t0 for every width and every t0: [sigma, t0, bin, 3]
    at = (t[None, :] - T0_GRID[:, None]).reshape(-1)
    basis = np.empty((SIGMA_GRID.size, T0_GRID.size, n_bins, 3))
    basis[..., 0] = 1.0
    for k in range(SIGMA_GRID.size):
        basis[k, :, :, 1] = np.interp(at, u, step[k]).reshape(T0_GRID.size, n_bins)
        basis[k, :, :, 2] = np.interp(at, u, root[k]).reshape(T0_GRID.size, n_bins)
    scale = np.where(w > 0, mean, 0.0).max(axis=1)
    scale = np.where(scale > 0, scale, 1.0)
    y = np.where(w > 0, mean, 0.0) / scale[:, None]
    pairs = (basis[..., :, None] * basis[..., None, :]).reshape(SIGMA_GRID.size, T0_GRID.size, n_bins, 9)
    normal = np.tensordot(w, pairs, axes=([1], [2])).reshape(n_sec, SIGMA_GRID.size, T0_GRID.size, 3, 3)
    rhs = np.tensordot(w * y, basis, axes=([1], [2]))                          # [sector, sigma, t0, 3]
    total = (w * y * y).sum(axis=1)
    ok = (w > 0).sum(axis=1) >= 3
    trace = np.trace(normal, axis1=-2, axis2=-1)
    ridge = (1e-12 * trace + (~ok)[:, None, None])[..., None, None] * np.eye(3)     # (a row that is not fitted stays solvable)
    coef = np.linalg.solve(normal + ridge, rhs[..., None])[..., 0]
    res = np.maximum(total[:, None, None] - (rhs * coef).sum(axis=-1), 0.0)
    sigma, t0, residual = (np.full(n_sec, np.nan) for _ in range(3))
    on_edge = np.ones(n_sec, dtype=bool)
    for s in np.nonzero(ok)[0]:
        k, j = np.unravel_index(np.argmin(res[s]), res[s].shape)
        on_edge[s] = k in (0, SIGMA_GRID.size - 1) or j in (0, T0_GRID.size - 1)
        sigma[s], t0[s] = SIGMA_GRID[k], T0_GRID[j]
        residual[s] = res[s, k, j]
        if on_edge[s]:
            continue
        # the lowest residual over t0 at the three widths around the minimum, each refined by a parabola in t0; then one in sigma
        low, shift = [], 0.0
        for kk in (k - 1, k, k + 1):
            jj = int(np.argmin(res[s, kk]))
            if jj in (0, T0_GRID.size - 1):
                low.append(res[s, kk, jj])
                continue
            x, v = _parabola(res[s, kk, jj - 1], res[s, kk, jj], res[s, kk, jj + 1])
            low.append(v)
            if kk == k:
                shift = T0_GRID[jj] + x / GRID
        x, v = _parabola(low[0], low[1], low[2]) if low[1] <= low[0] and low[1] <= low[2] else (0.0, low[1])
        sigma[s] = SIGMA_GRID[k] + x * (SIGMA_GRID[1] - SIGMA_GRID[0])
        t0[s], residual[s] = shift, v
    weight = w.sum(axis=1)
    residual = np.sqrt(residual / np.where(weight > 0, weight, 1.0)) * scale      # weighted rms, in counts
    return sigma, t0, residual, on_edge


def fit_edge(t, mean, count):
    """The blurred edge of one sector: t float64 [bins] (limb_profiles'), mean the bin means, count the bin counts (the weights; an
    empty bin does not count) -> (sigma, t0, residual, on_edge).  The model is
        sky + a (step * G_sigma)(t - t0) + b (sqrt(max(-u, 0)) * G_sigma)(t - t0)
    with the step 1 on the disk: (sky, a, b) by linear least squares for every sigma from 0.3 to 5 in steps of 0.1 and every t0 within
    +- 1.5 px in steps of 1/16, the lowest residual refined by a parabola in t0 and then in sigma.  The square-root term is the limb
    darkening, mu ~ sqrt(2 |t| / R) near the limb: without it the width is biased.  residual: the weighted rms of the fit in
    counts; on_edge: the minimum lies on the grid's edge (the edge is not there, or is wider than the grid)."""
    sigma, t0, residual, on_edge = fit_edges(t, np.asarray(mean)[None, :], np.asarray(count)[None, :])
    return float(sigma[0]), float(t0[0]), float(residual[0]), bool(on_edge[0])


def estimate_from_profiles(count, total, t):
    """estimate_psf from the tables of limb_profiles."""
    count = np.asarray(count)
    sectors = count.shape[0]
    theta = sector_angles(sectors)
    mean = np.asarray(total, dtype=np.float64) / np.maximum(count, 1)
    began = time.perf_counter()
    whole = (count == 0).mean(axis=1) <= MAX_EMPTY
    sigma, t0, residual, on_edge = (np.full(sectors, np.nan) for _ in range(4))
    on_edge = np.ones(sectors, dtype=bool)
    if whole.any():
        sigma[whole], t0[whole], residual[whole], on_edge[whole] = fit_edges(t, mean[whole], count[whole])
    fit_seconds = time.perf_counter() - began
    why = np.where(~whole, 'leaves the image', np.where(on_edge, 'minimum on the grid\'s edge', '')).astype(object)
    used = whole & ~on_edge
    cos2, sin2 = np.cos(theta) ** 2, np.sin(theta) ** 2
    design = np.stack([cos2, sin2], axis=1)

    def regress(mask):
        """(isotropic, (sigma_x^2, sigma_y^2) or the median sigma^2 twice, the residuals of every sector)."""
        a, v = design[mask], sigma[mask] ** 2
        eig = np.linalg.eigvalsh(a.T @ a)
        if eig[0] <= 0.0 or eig[1] / eig[0] > MAX_CONDITION:
            both = np.full(2, np.median(v))
            return True, both, np.where(mask, sigma ** 2 - both[0], np.nan)
        sol = np.linalg.solve(a.T @ a, a.T @ v)
        return False, sol, np.where(mask, sigma ** 2 - design @ sol, np.nan)

    if used.sum() < MIN_SECTORS:
        raise ValueError('the limb gives %d usable sectors of %d, fewer than %d: no estimate' % (used.sum(), sectors, MIN_SECTORS))
    isotropic, sol, res = regress(used)
    centre = np.median(res[used])
    spread = max(1.4826 * np.median(np.abs(res[used] - centre)), OUTLIER_FLOOR * np.median(sigma[used] ** 2))
    out = used & (np.abs(res - centre) > OUTLIER_SIGMAS * spread)
    if out.any():
        why[out] = 'beyond %g robust sigma of the regression' % OUTLIER_SIGMAS
        used = used & ~out
        if used.sum() < MIN_SECTORS:
            raise ValueError('the limb gives %d usable sectors of %d, fewer than %d: no estimate' % (used.sum(), sectors, MIN_SECTORS))
        isotropic, sol, res = regress(used)
    if not (sol > 0.0).all():
        raise ValueError('the regression gives a negative sigma^2 (%g, %g): no estimate' % tuple(sol))
    rows = [{'theta': float(theta[s]), 'sigma': None if np.isnan(sigma[s]) else float(sigma[s]),
             't0': None if np.isnan(t0[s]) else float(t0[s]), 'residual': None if np.isnan(residual[s]) else float(residual[s]),
             'used': bool(used[s]), 'why_not': None if used[s] else str(why[s])} for s in range(sectors)]
    return {'sigma_x': float(math.sqrt(sol[0])), 'sigma_y': float(math.sqrt(sol[1])), 'isotropic': bool(isotropic), 'sectors': rows,
            'n_used': int(used.sum()), 'rms': float(np.sqrt(np.mean(res[used] ** 2))), 'fit_seconds': fit_seconds}


def estimate_psf(image, circle, reach=DEFAULT_REACH, sub=DEFAULT_SUB, sectors=DEFAULT_SECTORS):
    """The Gaussian widths of the blur of a uint16 image along its axes, from the limb of `circle` (cx, cy, rad) -> {'sigma_x' (along
    a row), 'sigma_y' (down a column), 'isotropic', 'sectors', 'n_used', 'rms', 'fit_seconds'}.
    Every sector's edge is fitted (fit_edge); sigma^2 is regressed on cos^2 theta and sin^2 theta over the sectors that are used.  A
    sector is dropped when more than 10 % of its bins are empty (the annulus leaves the image), when its minimum lies on the grid's
    edge, or when its sigma^2 lies beyond 3 robust sigma (1.4826 MAD, at least 0.05 of the median sigma^2) of the regression, which is then fitted
    once more; 'sectors' says for each: theta, sigma, t0, residual, used, why_not.  When the used sectors do not span both axes --
    the 2 x 2 normal matrix of the regression has a condition number above 100 -- the answer is one width, the median of theirs, for
    both axes and 'isotropic' is True.  rms: of the regression's residuals, in px^2.  ValueError below 3 used sectors.
    The widths include the pixel's own 1 / sqrt(12) px an axis: they are the blur the image has, returned as measured."""
    count, total, _, t = limb_profiles(image, circle, reach, sub, sectors)
    return estimate_from_profiles(count, total, t)


def model_curve(t, mean, count, sigma, t0):
    """The fitted model of a sector at the bin centres (for <stem>_esf.txt)."""
    u, step, root = _bases(float(math.ceil(np.abs(t).max() + T0_REACH + 1.0)))
    k = int(np.argmin(np.abs(SIGMA_GRID - sigma)))
    basis = np.stack([np.ones_like(t), np.interp(t - t0, u, step[k]), np.interp(t - t0, u, root[k])], axis=1)
    w = np.sqrt(np.asarray(count, dtype=np.float64))
    coef = np.linalg.lstsq(basis * w[:, None], np.asarray(mean, dtype=np.float64) * w, rcond=None)[0]
    return basis @ coef


# ---- command line ---------------------------------------------------------------------------------
def write_esf(path, count, total, t, estimate):
    """<stem>_esf.txt: a line a bin -- sector, theta, t, count, mean, the fitted model (nan where the sector was not fitted)."""
    mean = np.asarray(total, dtype=np.float64) / np.maximum(count, 1)
    with open(path, 'w') as f:
        f.write('# sector theta t count mean model\n')
        for s, row in enumerate(estimate['sectors']):
            model = np.full(t.size, np.nan) if row['sigma'] is None else model_curve(t, mean[s], count[s], row['sigma'], row['t0'])
            for b in range(t.size):
                f.write('%d %.6f %.4f %d %.3f %.3f\n' % (s, row['theta'], t[b], count[s, b], mean[s, b], model[b]))


def main(argv=None):
    from . import disk
    from .deconvolve import _floats
    from .linemaps import _print_json
    from .video_reader import video_reader
    p = argparse.ArgumentParser(
        prog='python -m solex_ser_recon_en_amd.psf',
        usage='%(prog)s INPUT [--shift S] [--circle cx,cy,rad] [--reach Q] [--sub N] [--sectors S] [SHG_MAIN flags]',
        description='Measure the blur of a disk from its limb: the Gaussian sigma along the rows and down the columns.  INPUT is a SER '
                    'or AVI scan (it brings its circle), or a 16-bit grey PNG this package wrote (it needs --circle).')
    p.add_argument('--shift', type=int, default=0, help='pixel shift of a scan\'s disk (the -w shift; default 0: the line centre)')
    p.add_argument('--circle', type=_floats, default=None, help='cx,cy,rad of the disk in a PNG')
    p.add_argument('--reach', type=int, default=DEFAULT_REACH, help='pixels either side of the limb, 1 to 64 (default %d)' % DEFAULT_REACH)
    p.add_argument('--sub', type=int, default=DEFAULT_SUB, help='radial bins a pixel, 1 to 8 (default %d)' % DEFAULT_SUB)
    p.add_argument('--sectors', type=int, default=DEFAULT_SECTORS, help='a multiple of 8 from 8 to 64 (default %d)' % DEFAULT_SECTORS)

    def checks(args):
        if not 1 <= args.reach <= 64:
            p.error('--reach is 1 to 64')
        if not 1 <= args.sub <= 8:
            p.error('--sub is 1 to 8')
        if not (8 <= args.sectors <= 64 and args.sectors % 8 == 0):
            p.error('--sectors is a multiple of 8 from 8 to 64')
        if args.circle is not None and len(args.circle) != 3:
            p.error('--circle is cx,cy,rad')

    def file_checks(args, files):
        if args.circle is None and any(f.lower().endswith('.png') for f in files):
            p.error('a PNG needs --circle cx,cy,rad')

    args, opts, (path,) = disk.parse(p, argv, 'psf', 'measuring the blur', checks, file_checks,
                                     need='exactly one SER, AVI or PNG file is needed', png=True)
    try:
        if path.lower().endswith('.png'):
            img, _, stem = disk.png_input(path, opts)
            res = {'circle': tuple(args.circle), 'shift': None, 'ratio': None, 'phi': None, 'crop': None}
        else:
            if args.circle is not None:
                raise ValueError('--circle goes with a PNG: a scan brings its own limb fit')
            res = disk.scan_disk(video_reader(path), opts, args.shift, 'measuring the blur')
            img = res['image']
            stem = '%s_shift=%d' % (os.path.splitext(path)[0], res['shift'])
        count, total, _, t = limb_profiles(img, res['circle'], args.reach, args.sub, args.sectors)
        est = estimate_from_profiles(count, total, t)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    from .solex_util import output_path
    esf = output_path(stem + '_esf.txt', opts)
    write_esf(esf, count, total, t, est)
    out = {'input': path, 'shape': [int(v) for v in img.shape], 'shift': res['shift'], 'reach': args.reach, 'sub': args.sub,
           'sigma_x': est['sigma_x'], 'sigma_y': est['sigma_y'], 'isotropic': est['isotropic'], 'n_used': est['n_used'],
           'n_sectors': args.sectors, 'rms': est['rms'], 'fit_seconds': est['fit_seconds'], 'sectors': est['sectors'], 'esf': esf}
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
