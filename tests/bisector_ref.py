"""NumPy restatement of the line-bisector maps' two kernels (include/shg_hip.h: shg_line_bisector, shg_line_bisector_finish), written
from the arithmetic the header states, not from the kernels: the GPU must match these bit for bit.  Also two synthetic disk scans
(a symmetric Gaussian line with injected shift, width and depth fields, and an asymmetric line of two components with shifts of
their own), reference bisectors found on the analytic profiles, and the accuracy the restatement reaches on them."""
import numpy as np

from tests import doppler_ref, lineprofile_ref

profiles = doppler_ref.profiles
window = lineprofile_ref.window


def level_of(f, core_d, c2):
    """level = ((1.0 - f) * core_d) + (f * (0.5 * (double)C2)), one IEEE operation a step."""
    f = np.float64(f)
    return ((np.float64(1.0) - f) * core_d) + (f * (np.float64(0.5) * np.asarray(c2, dtype=np.float64)))


def measure(p, lo, hi, ref, levels):
    """(bis, chord) float32 [K, n] of the profiles p int64 [n, iw] over the window [lo, hi]; ref = fit[y, 3] + S."""
    p = np.asarray(p, dtype=np.int64)
    n_fr, kk = p.shape[0], len(levels)
    bis = np.full((kk, n_fr), np.nan, dtype=np.float32)
    chord = np.full((kk, n_fr), np.nan, dtype=np.float32)
    seg = p[:, lo:hi + 1]
    m = hi - lo + 1
    c2 = p[:, lo] + p[:, hi]
    jrel = np.argmin(seg, axis=1)                        # first occurrence
    j = lo + jrel
    k = np.flatnonzero((j > lo) & (j < hi))
    if k.size == 0:
        return bis, chord
    jk, rk = j[k], jrel[k]
    a, b, e = p[k, jk - 1], p[k, jk], p[k, jk + 1]
    den = a + e - 2 * b
    core = b.astype(np.float64) - ((a - e) * (a - e)).astype(np.float64) / (8.0 * den.astype(np.float64))
    sk = seg[k]
    idx = np.arange(m)[None, :]
    rows = np.arange(k.size)
    for i, f in enumerate(levels):
        level = level_of(f, core, c2[k])
        ge = sk >= level[:, None]
        jl = np.where(ge & (idx < rk[:, None]), idx, -1).max(axis=1)       # the largest j in [lo, j*) with p >= level
        jr = np.where(ge & (idx > rk[:, None]), idx, m).min(axis=1)        # the smallest j in (j*, hi] with p >= level
        has = (b.astype(np.float64) < level) & (jl >= 0) & (jr < m)
        jl_, jr_ = np.clip(jl, 0, m - 2), np.clip(jr, 1, m - 1)
        pl, pl1 = sk[rows, jl_], sk[rows, jl_ + 1]
        pr, pr1 = sk[rows, jr_], sk[rows, jr_ - 1]
        with np.errstate(invalid='ignore', divide='ignore'):
            xl = (lo + jl_).astype(np.float64) + (pl.astype(np.float64) - level) / (pl - pl1).astype(np.float64)
            xr = (lo + jr_).astype(np.float64) - (pr.astype(np.float64) - level) / (pr - pr1).astype(np.float64)
            bis[i, k] = np.where(has, ((0.5 * (xl + xr)) - ref).astype(np.float32), np.float32(np.nan))
            chord[i, k] = np.where(has, (xr - xl).astype(np.float32), np.float32(np.nan))
    return bis, chord


def line_bisector(frames, fit, half_width, levels, shift=0, flip_x=False, n_cols=None, k_offset=0):
    """planes float32 [2K, ih, n_cols] (bisectors, then chords): frames [n, H, W] (file layout) of the columns k_offset ..
    k_offset + n - 1 (reversed with flip_x); the other columns NaN."""
    frames = np.asarray(frames)
    fit = np.asarray(fit, dtype=np.float64)
    levels = [float(f) for f in levels]
    kk = len(levels)
    n, h, w = frames.shape
    ih, iw = (w, h) if w > h else (h, w)
    n_cols = n if n_cols is None else int(n_cols)
    raw = np.full((2 * kk, ih, n), np.nan, dtype=np.float32)
    for y in range(ih):
        win = window(fit[y, 0], shift, half_width, iw)
        if win is None:
            continue
        bis, chord = measure(profiles(frames, y), win[0], win[1], fit[y, 3] + np.float64(shift), levels)
        raw[:kk, y] = bis
        raw[kk:, y] = chord
    out = np.full((2 * kk, ih, n_cols), np.nan, dtype=np.float32)
    cols = k_offset + np.arange(n)
    out[:, :, n_cols - 1 - cols if flip_x else cols] = raw
    return out


def display(v, kind, half_width, display_range):
    """uint16 display plane of one finished plane: the bisectors as the Dopplergram's shift, the chords as the profile's width."""
    return lineprofile_ref.display(v, 'shift' if kind == 'bisector' else 'width', half_width, display_range)


def line_bisector_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, half_width=None, display_range=None):
    """(maps float32 [2K, out_h, nw], png uint16 [2K, out_h, nw] or None): every plane as doppler_ref.doppler_finish."""
    kk = raw.shape[0] // 2
    maps = np.stack([doppler_ref.doppler_finish(r, h00, h01, h02, out_h, out_w, circle, crop)[0] for r in raw])
    png = None
    if display_range is not None:
        png = np.stack([display(m, 'bisector' if q < kk else 'chord', half_width, display_range) for q, m in enumerate(maps)])
    return maps, png


# ---- synthetic scans with known bisectors ----
def symmetric_scan(ih, n, iw, noise=0.004, seed=3):
    """lineprofile_ref's disk scan (a Gaussian line with injected shift, sigma and depth fields): every bisector of a symmetric
    line is its centre.  -> (frames, centre [ih], on [ih, n], shift [ih, n])."""
    shift, sigma, depth = lineprofile_ref.injected_fields(ih, n)
    frames, centre, on, _ = lineprofile_ref.disk_scan(shift, sigma, depth, iw, noise=noise, seed=seed)
    return frames, centre, on, shift


# the asymmetric line: a narrow deep component and a broad shallow one, each displaced by its own field
NARROW = (0.6, 1.6)          # (depth, sigma px)
BROAD = (0.25, 4.5)


def asym_fields(ih, n):
    """(s1, s2) [ih, n]: the narrow component's shift (doppler_ref's field) and the broad one's (0.5 s1 + 1.2 px, a red wing)."""
    s1 = doppler_ref.injected_field(ih, n)
    return s1, 0.5 * s1 + 1.2


def asym_line(x, c1, c2):
    """The asymmetric line's relative profile at x (broadcast) with the components centred on c1 and c2."""
    return (1.0 - NARROW[0] * np.exp(-0.5 * ((x - c1) / NARROW[1]) ** 2)
            - BROAD[0] * np.exp(-0.5 * ((x - c2) / BROAD[1]) ** 2))


def asym_scan(ih, n, iw, noise=0.004, seed=3):
    """doppler_ref.disk_scan's scene with the asymmetric line -> (frames uint16 in file layout, centre [ih], on [ih, n], s1, s2)."""
    from solex_ser_recon_en_amd import synth
    s1, s2 = asym_fields(ih, n)
    sp = synth.scene_params(n, ih, iw)
    y = np.arange(ih, dtype=np.float64)
    x = np.arange(iw, dtype=np.float64)
    centre = synth.curve_of_row(y, ih, iw)
    lit = ((y > sp['y_lo']) & (y < sp['y_hi'])).astype(np.float64)
    frames = np.empty((n, iw, ih), dtype=np.uint16)
    on = np.zeros((ih, n), dtype=bool)
    for k in range(n):
        r2 = ((k - sp['cx']) / sp['ax']) ** 2 + ((y - sp['cy']) / sp['ay']) ** 2
        on[:, k] = (r2 < 0.9) & (lit > 0)
        bright = np.where(r2 < 1.0, 0.35 + 0.65 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0)), sp['sky']) * lit
        line = asym_line(x[None, :], (centre + s1[:, k])[:, None], (centre + s2[:, k])[:, None])
        img = sp['gain'] * bright[:, None] * line + noise * np.random.default_rng([seed, k]).standard_normal((ih, iw))
        img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
        frames[k] = np.rot90(img, -1)
    return frames, centre, on, s1, s2


def asym_truth(fit, half_width, levels, centre, s1, s2, iters=60):
    """Reference bisectors [K, ih, n] of the asymmetric scan, in pixels from fit[y, 3], found on the analytic profile with the
    kernel's definitions: the window [lo, hi] of fit[y, 0]; continuum = the mean of the profile at lo and hi; core = the profile's
    minimum in the window (golden-section search); level = (1 - f) core + f continuum; the crossings the roots of profile = level
    between lo and the minimum and between the minimum and hi (bisection), NaN where a side does not reach the level."""
    ih, n = s1.shape
    iw_big = 1 << 20
    out = np.full((len(levels), ih, n), np.nan)
    for y in range(ih):
        win = window(fit[y, 0], 0, half_width, iw_big)
        if win is None:
            continue
        lo, hi = float(win[0]), float(win[1])
        c1, c2 = centre[y] + s1[y], centre[y] + s2[y]

        def prof(x):
            return asym_line(x, c1, c2)

        a, b = np.full(n, lo), np.full(n, hi)
        g = (np.sqrt(5.0) - 1.0) / 2.0
        for _ in range(iters):
            x1, x2 = b - g * (b - a), a + g * (b - a)
            left = prof(x1) < prof(x2)
            b = np.where(left, x2, b)
            a = np.where(left, a, x1)
        xm = 0.5 * (a + b)
        core, cont = prof(xm), 0.5 * (prof(np.full(n, lo)) + prof(np.full(n, hi)))
        for i, f in enumerate(levels):
            level = (1.0 - f) * core + f * cont
            roots = []
            for u, v in ((np.full(n, lo), xm), (xm, np.full(n, hi))):
                ok = (prof(u) - level) * (prof(v) - level) <= 0
                uu, vv = u.copy(), v.copy()
                for _ in range(iters):
                    mid = 0.5 * (uu + vv)
                    same = (prof(mid) - level) * (prof(uu) - level) > 0
                    uu = np.where(same, mid, uu)
                    vv = np.where(same, vv, mid)
                roots.append(np.where(ok, 0.5 * (uu + vv), np.nan))
            out[i, y] = 0.5 * (roots[0] + roots[1]) - fit[y, 3]
    return out


def errors(bis, truth, on):
    """{level index: (RMS, max |error| px, NaN count)} of bisector planes [K, ih, n] against the truth [K, ih, n] on the disk."""
    out = {}
    for i in range(bis.shape[0]):
        e = bis[i].astype(np.float64)[on] - truth[i][on]
        out[i] = (float(np.sqrt(np.nanmean(e * e))), float(np.nanmax(np.abs(e))), int(np.isnan(e).sum()))
    return out


def sym_truth(fit, centre, shift, k):
    """The symmetric scan's true bisector of every level [K, ih, n]: the line's centre, from fit[y, 3]."""
    return np.broadcast_to((centre[:, None] + shift) - fit[:, 3:4], (k,) + shift.shape)


# What the restatement achieves at H = 10 on the levels LEVELS, on symmetric_scan(400, 300, 48) and asym_scan(400, 300, 48) (seed 3)
# with the fitted line placed off the true centre by each of FIT_OFFSETS px: the worst (RMS, max) bisector error in pixels on the disk
# over the levels and offsets.  Measured, not assumed (tests/test_bisector_cpu.py re-measures them); the values below are the
# measurements rounded up in their last digit.  Without noise: symmetric 0.0116 / 0.0265 px (the worst at f = 0.8, where the
# linear interpolation between samples is coarsest against the Gaussian's curvature), asymmetric 0.0228 / 0.0466 px; at synth's
# noise 0.004: symmetric 0.0416 / 0.1999 px, asymmetric 0.0711 / 0.511 px (f = 0.8, near the continuum, where the profile is
# flattest and the noise moves the crossings most).  No NaN on the disk in either.
LEVELS = (0.2, 0.4, 0.5, 0.6, 0.8)
FIT_OFFSETS = (-1.0, -0.5, 0.0, 0.5, 1.0)
TOLERANCE = {0.0: {'symmetric': (0.012, 0.027), 'asymmetric': (0.023, 0.047)},
             0.004: {'symmetric': (0.042, 0.201), 'asymmetric': (0.072, 0.52)}}


def scan(kind, ih, n, iw, noise, seed=3):
    """(frames, centre, on, truth(fit, levels) -> [K, ih, n]) of the symmetric or the asymmetric scan."""
    if kind == 'symmetric':
        frames, centre, on, shift = symmetric_scan(ih, n, iw, noise, seed)
        return frames, centre, on, lambda fit, hw, levels: sym_truth(fit, centre, shift, len(levels))
    frames, centre, on, s1, s2 = asym_scan(ih, n, iw, noise, seed)
    return frames, centre, on, lambda fit, hw, levels: asym_truth(fit, hw, levels, centre, s1, s2)
