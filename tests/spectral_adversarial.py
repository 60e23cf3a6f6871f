"""Seeded adversarial configurations for shg_atlas_correlate: an anchor wavelength, an anchor_x, a W, a scales array and a uint16
spectrum each.  The op takes any positive scales, so the scales that put an atlas point exactly on 0, on W, just below W or on a
pixel are constructed: nextafter neighbours of s = (a[k] - lambda_a) / (target - anchor_x) are searched until the reference's own
x[k] equals the target.  records() evaluates every guess on the exact reference (tests/spectral_exact.py); occurrences() counts on
those records which of CLASSES were reached."""
import numpy as np

from tests import spectral_exact as ex
from tests import spectral_ref

CLASSES = ('x_eq_0', 'x_eq_w', 'x_k1_below_w', 'pixel_on_point', 'pixel_at_x_k1', 'anchor_on_point', 'one_point_run',
           'two_point_run', 'partly_empty', 'ax_negative', 'ax_0_5', 'ax_w_minus_1', 'ax_beyond_w', 'constant_row',
           'nearly_constant', 'tie', 'gap_above', 'gap_below')
LAYOUT_W = (511, 512, 513, 1023, 1024, 1025, 1031, 1032, 1033, 2047, 2048, 2049, 4095, 4096, 4097, 8183, 8184, 8185, 8191, 8192)
SWEEP_W = tuple(range(2, 301)) + LAYOUT_W
LINES = (6562.808, 5889.95, 5875.618, 4861.35, 3968.47, 6102.72, 5183.6, 8542.09)
FLAT_255 = 613807          # the atlas's longest flat stretch: 155 points at y = 255 (the row is exactly 1.0, its mean exact)
FLAT_250 = 587101          # 90 points at y = 250: 250 / 255 has an inexact mean over W = 20 pixels


def hit_scale(a, k, target, anchor_wavelength, anchor_x, tries=400):
    """A positive scale s with ((a[k] - lambda_a) / s) + anchor_x == target exactly, or None."""
    if target == anchor_x:
        return None
    s = (a[k] - anchor_wavelength) / (target - anchor_x)
    if not (np.isfinite(s) and s > 0):
        return None
    lo = hi = s
    for _ in range(tries):
        for c in (lo, hi):
            if ex.x_of(a[k], anchor_wavelength, anchor_x, c) == target:
                return float(c)
        lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, np.inf)
    return None


def _hit_near(a, target, lam, ax, s_guess):
    """(k, s): a scale near s_guess that puts atlas point k (one near the guess's) exactly on target, or None."""
    k = int(np.clip(np.searchsorted(a, lam + (target - ax) * s_guess), 6, a.shape[0] - 7))
    for dk in (0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5):
        s = hit_scale(a, k + dk, target, lam, ax)
        if s is not None:
            return k + dk, s
    return None


def _spectrum(a, yv, rng, w, lam, ax, dispersion, noise=0.004):
    """uint16 spectrum: the atlas at `dispersion` around lam with its anchor at pixel ax, a slope and noise (never 0)."""
    p = np.arange(w, dtype=np.float64)
    lo, hi = np.searchsorted(a, [lam + (0 - ax) * dispersion - 1.0, lam + (w - ax) * dispersion + 1.0])
    lo, hi = max(int(lo) - 2, 0), min(int(hi) + 2, a.shape[0])
    prof = np.interp(lam + (p - ax) * dispersion, a[lo:hi], yv[lo:hi])
    prof = prof * (1.0 + 0.1 * (p / w - 0.5)) + rng.normal(0.0, noise, w)
    return np.clip(np.rint(50000.0 * prof), 1, 65535).astype(np.uint16)


def _cfg(name, lam, ax, w, scales, s2, special=(), hits=()):
    scales = np.asarray(scales, dtype=np.float64)
    assert np.all(np.isfinite(scales)) and np.all(scales > 0)
    return dict(name=name, lam=float(lam), ax=float(ax), w=int(w), scales=scales, s2=np.asarray(s2, dtype=np.uint16),
                special=sorted(set(int(i) for i in special)), hits=list(hits))


def _edge_scales(a, rng, lam, ax, w):
    """(scales, adversarial indices, hits): a random guess, then x[k] == 0, x[k] == W, x[k1] just below W, an interior pixel on a
    point, and (points 2 px apart) a pixel exactly at x[k1].  hits: (guess, k, target) of each constructed scale."""
    out = [float(rng.uniform(0.02, 0.12))]
    targets = [(0.0, float(rng.uniform(0.02, 0.12))), (float(w), float(rng.uniform(0.02, 0.12))),
               (float(np.nextafter(float(w), 0.0)), float(rng.uniform(0.02, 0.12)))]
    if w >= 3:
        targets.append((float(rng.integers(1, w - 1)), float(rng.uniform(0.02, 0.12))))
        targets.append((float(w - 1), 0.005))
    hits = []
    for t, s0 in targets:
        h = _hit_near(a, t, lam, ax, s0)
        if h is not None:
            hits.append((len(out), h[0], t))
            out.append(h[1])
    return out, list(range(1, len(out))), hits


def configs(a, y, seed=2026):
    """The configurations, in a fixed order (a = the reference's atlas axis, y its uint8 intensities)."""
    rng = np.random.default_rng(seed)
    yv = y / 255
    n = a.shape[0]
    out = []
    # the W sweep: a few guesses per launch, the run-end hits among them
    for w in SWEEP_W:
        lam = LINES[w % len(LINES)] + float(rng.uniform(-2.0, 2.0))
        ax = float(rng.uniform(0.0, w))
        scales, special, hits = _edge_scales(a, rng, lam, ax, w)
        s2 = _spectrum(a, yv, rng, w, lam, ax, float(rng.uniform(0.03, 0.1)))
        out.append(_cfg('sweep_w%d' % w, lam, ax, w, scales, s2, special, hits))
    # anchors exactly on an atlas point at an integer anchor_x: every guess puts that point on a pixel
    for w, ax in ((64, 20.0), (300, 151.0), (1025, 700.0)):
        k = int(np.searchsorted(a, LINES[w % len(LINES)]))
        true = 0.05
        scales = np.concatenate([np.linspace(0.03, 0.08, 11), [true, np.nextafter(true, 1.0)]])
        out.append(_cfg('anchor_point_w%d' % w, a[k], ax, w, scales, _spectrum(a, yv, rng, w, a[k], ax, true, 0.001),
                        special=range(scales.shape[0])))
    # runs of one and two points: an anchor at the atlas's last point near pixel 0, at its first point near W - 1
    last, first = float(a[n - 1]), float(a[0])
    for name, lam, ax, w, scales in (
            ('last_one_point', last, 0.3, 40, [0.02, 0.0101, 0.005, 0.05]),             # d / s > 0.3: only a[n - 1] inside
            ('last_two_points', last, 2.5, 40, [0.005, 0.0045, 0.02, 0.004]),           # d / s = 2: two points
            ('first_one_point', first, 38.5, 40, [0.006, 0.002, 0.05, 0.0066]),
            ('first_two_points', first, 37.2, 40, [0.005, 0.0041, 0.1, 0.02])):
        out.append(_cfg(name, lam, ax, w, scales, rng.integers(1000, 60000, w), special=range(len(scales))))
    # a run empty for some guesses: the anchor 0.3 A below the atlas's end, anchor_x 20 px left of the frame
    scales = np.linspace(0.005, 0.05, 24)
    out.append(_cfg('partly_empty', last - 0.3, -20.0, 60, scales, rng.integers(1000, 60000, 60), special=range(24)))
    # anchor_x outside or at the edges of the frame: windows clipped, at the reference's W - 1 bound, or empty
    for name, w, ax in (('ax_neg_clipped', 50, -3.7), ('ax_neg_empty', 50, -30.0), ('ax_in_0_5', 50, 2.6),
                        ('ax_w_minus_1', 50, 49.4), ('ax_beyond_w', 50, 52.0), ('ax_far_beyond', 50, 90.0),
                        ('ax_w_minus_1_big', 2049, 2048.0)):
        lam = 6562.808
        scales, special, hits = _edge_scales(a, rng, lam, ax, w)
        out.append(_cfg(name, lam, ax, w, scales + [0.04, 0.06], _spectrum(a, yv, rng, w, lam, ax, 0.05), special, hits))
    # frames inside a flat atlas stretch: exactly constant rows (NaN), and rows whose inexact mean leaves them nearly constant
    for name, k, w in (('flat_255', FLAT_255, 12), ('flat_250', FLAT_250, 20)):
        lam = float(a[k + 45])
        scales = [0.005, 0.01, 0.02, 0.03, 0.2, 0.05]                  # the last two leave the stretch
        for ax in (w / 2.0 + 0.25, w + 4.5):                           # a window, and none
            out.append(_cfg('%s_ax%g' % (name, ax), lam, ax, w, scales, rng.integers(1000, 60000, w), special=range(len(scales))))
    # exact ties and guesses that must not leak into one another: one scale at several positions
    w = 200
    s = [0.05, 0.07, 0.05, 0.031, 0.05, np.nextafter(0.05, 1.0), 0.07]
    out.append(_cfg('repeated_scales', 6562.808, 97.3, w, s, _spectrum(a, yv, rng, w, 6562.808, 97.3, 0.05, 0.0005), special=range(7)))
    return out


def auto_nan_case(a, y):
    """(spectrum2, anchor_x, anchor_wavelength) whose np.linspace guesses give NaN for the small scales only (the frame inside the
    y = 255 stretch) and a correlation for the large ones."""
    w = 12
    rng = np.random.default_rng(7)
    return rng.integers(1000, 60000, w).astype(np.uint16), 2.5, float(a[FLAT_255 + 8])


def records(cfg, a, yv):
    """One dict per guess: k0, k1 (None when empty), lo, hi, row (None when empty), corr (exact Corr or None), numpy (np.corrcoef's
    value), bound, general (np.corrcoef's bound)."""
    w, lam, ax = cfg['w'], cfg['lam'], cfg['ax']
    lspec = spectral_ref.log_spectrum(cfg['s2'], ax)
    sv = ex.Series(lspec.astype(np.float64))
    out = []
    for s in cfg['scales']:
        k0, k1, lo, hi = ex.run_ends(a, lam, ax, float(s), w)
        r = dict(k0=k0, k1=k1, lo=lo, hi=hi, row=None, corr=None, numpy=np.nan, bound=None, general=None)
        if k0 is not None:
            u = ex.row(a, yv, lam, ax, float(s), w, lo, hi)
            c = ex.Corr(ex.Series(u), sv)
            with np.errstate(invalid='ignore', divide='ignore'):
                r.update(row=u, corr=c, numpy=float(np.corrcoef(u, lspec)[0, 1]))
            if not c.nan:
                r.update(bound=ex.kernel_bound(c), general=ex.numpy_bound(c))
        out.append(r)
    return out


def _x(a, cfg, k, s):
    return ex.x_of(a[k], cfg['lam'], cfg['ax'], s)


def occurrences(cfg, recs, a):
    """Class -> count of guesses (or configurations) of cfg where the exact reference reaches it."""
    w, ax = cfg['w'], cfg['ax']
    n = a.shape[0]
    c = dict.fromkeys(CLASSES, 0)
    for s, r in zip(cfg['scales'], recs):
        k0, k1 = r['k0'], r['k1']
        if k0 is None:
            continue
        if _x(a, cfg, k0, s) == 0.0:
            c['x_eq_0'] += 1
        if k1 + 1 < n and _x(a, cfg, k1 + 1, s) == float(w):
            c['x_eq_w'] += 1
        x1 = _x(a, cfg, k1, s)
        if 0 < w - x1 <= 4 * np.spacing(float(w)):
            c['x_k1_below_w'] += 1
        if x1 == np.floor(x1):
            c['pixel_at_x_k1'] += 1
        xs = ex.x_of(a[k0:k1], cfg['lam'], ax, s)
        if np.any((xs == np.floor(xs)) & (xs > 0)):
            c['pixel_on_point'] += 1
        if float(cfg['lam']) in a[k0:k1 + 1] and ax == np.floor(ax) and 0 <= ax < w:
            c['anchor_on_point'] += 1
        c['one_point_run'] += k0 == k1
        c['two_point_run'] += k1 == k0 + 1
        if r['corr'].nan:
            c['constant_row'] += 1
        elif ex.nearly_constant(r['corr']):
            c['nearly_constant'] += 1
    empty = sum(r['k0'] is None for r in recs)
    c['partly_empty'] += 0 < empty < len(recs)
    c['ax_negative'] += ax < 0
    c['ax_0_5'] += 0 <= ax < 5
    c['ax_w_minus_1'] += int(ax) == w - 1
    c['ax_beyond_w'] += ax >= w
    good = [r for r in recs if r['corr'] is not None and not r['corr'].nan]
    for i, r in enumerate(good):
        c['tie'] += any(r['corr'].same(q['corr']) for q in good[i + 1:])
    gap = top_two_gap(recs)
    if gap is not None:
        best = max(good, key=lambda r: r['corr'].value())
        c['gap_above' if gap > 2 * best['bound'] else 'gap_below'] += 1
    return c


def exact_best(recs):
    """Index of the exact maximiser among the guesses with a correlation (the first of exact ties), or None."""
    best = None
    for i, r in enumerate(recs):
        if r['corr'] is not None and not r['corr'].nan and (best is None or r['corr'].value() > recs[best]['corr'].value()):
            best = i
    return best


def top_two_gap(recs):
    """The exact correlation's top-two gap (a Fraction; 0 for a tie), None with fewer than two correlations."""
    vals = sorted((r['corr'].value() for r in recs if r['corr'] is not None and not r['corr'].nan), reverse=True)
    return vals[0] - vals[1] if len(vals) >= 2 else None
