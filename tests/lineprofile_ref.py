"""NumPy restatement of the line-profile maps' two kernels (include/shg_hip.h: shg_line_profile, shg_line_profile_finish), written
from the arithmetic the header states, not from the kernels: the GPU must match these bit for bit.  Also a synthetic disk scan
with injected fields of line shift, Gaussian sigma and depth, and the accuracy the restatement reaches on it."""
import numpy as np

from tests import doppler_ref

PLANES = ('shift', 'core', 'width', 'cog', 'ew')
profiles = doppler_ref.profiles


def window(f0, shift, half_width, iw):
    """(lo, hi) of a slit row, or None: c = int(fit[y, 0] + S) (truncated), lo = max(c - H, 1), hi = min(c + H, iw - 2), none when
    fit[y, 0] is not finite or hi - lo < 2."""
    if not np.isfinite(f0):
        return None
    c = int(np.clip(np.float64(f0) + np.float64(shift), -2.0 ** 30, 2.0 ** 30))
    lo, hi = max(c - half_width, 1), min(c + half_width, iw - 2)
    return None if hi - lo < 2 else (lo, hi)


def measure(p, lo, hi, ref):
    """The five values (float32, PLANES order) of the profiles p int64 [n, iw] over the window [lo, hi]; ref = fit[y, 3] + S."""
    p = np.asarray(p, dtype=np.int64)
    n_fr = p.shape[0]
    nan = np.full(n_fr, np.nan, dtype=np.float32)
    out = {k: nan.copy() for k in PLANES}
    seg = p[:, lo:hi + 1]
    m = hi - lo + 1
    jj = np.arange(lo, hi + 1, dtype=np.int64)
    c2 = p[:, lo] + p[:, hi]
    s0 = m * c2 - 2 * seg.sum(axis=1)
    s1 = c2 * jj.sum() - 2 * (seg * jj).sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        cog = (s1.astype(np.float64) / s0.astype(np.float64) - ref).astype(np.float32)
        ew = (s0.astype(np.float64) / c2.astype(np.float64)).astype(np.float32)
    out['cog'] = np.where(s0 > 0, cog, np.float32(np.nan))
    out['ew'] = np.where(c2 != 0, ew, np.float32(np.nan))
    jrel = np.argmin(seg, axis=1)                        # first occurrence
    j = lo + jrel
    ok = (j > lo) & (j < hi)
    k = np.flatnonzero(ok)
    if k.size == 0:
        return out
    jk, rk = j[k], jrel[k]
    a, b, e = p[k, jk - 1], p[k, jk], p[k, jk + 1]
    den = a + e - 2 * b
    delta = (a - e).astype(np.float64) / (2 * den).astype(np.float64)
    out['shift'][k] = ((jk.astype(np.float64) + delta) - ref).astype(np.float32)
    core = b.astype(np.float64) - ((a - e) * (a - e)).astype(np.float64) / (8.0 * den.astype(np.float64))
    out['core'][k] = core.astype(np.float32)
    half = 0.5 * (0.5 * c2[k].astype(np.float64) + core)
    sk = seg[k]
    ge = sk >= half[:, None]
    idx = np.arange(m)[None, :]
    jl = np.where(ge & (idx < rk[:, None]), idx, -1).max(axis=1)           # the largest j in [lo, j*) with p >= half
    jr = np.where(ge & (idx > rk[:, None]), idx, m).min(axis=1)            # the smallest j in (j*, hi] with p >= half
    has = (b.astype(np.float64) < half) & (jl >= 0) & (jr < m)
    rows = np.arange(k.size)
    jl_, jr_ = np.clip(jl, 0, m - 2), np.clip(jr, 1, m - 1)
    pl, pl1 = sk[rows, jl_], sk[rows, jl_ + 1]
    pr, pr1 = sk[rows, jr_], sk[rows, jr_ - 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        xl = (lo + jl_).astype(np.float64) + (pl.astype(np.float64) - half) / (pl - pl1).astype(np.float64)
        xr = (lo + jr_).astype(np.float64) - (pr.astype(np.float64) - half) / (pr - pr1).astype(np.float64)
    out['width'][k] = np.where(has, (xr - xl).astype(np.float32), np.float32(np.nan))
    return out


def line_profile(frames, fit, half_width, shift=0, flip_x=False, n_cols=None, k_offset=0):
    """planes float32 [5, ih, n_cols] (PLANES order): frames [n, H, W] (file layout) of the columns k_offset .. k_offset + n - 1
    (reversed with flip_x); the other columns NaN."""
    frames = np.asarray(frames)
    fit = np.asarray(fit, dtype=np.float64)
    n, h, w = frames.shape
    ih, iw = (w, h) if w > h else (h, w)
    n_cols = n if n_cols is None else int(n_cols)
    raw = np.full((len(PLANES), ih, n), np.nan, dtype=np.float32)
    for y in range(ih):
        win = window(fit[y, 0], shift, half_width, iw)
        if win is None:
            continue
        vals = measure(profiles(frames, y), win[0], win[1], fit[y, 3] + np.float64(shift))
        for q, name in enumerate(PLANES):
            raw[q, y] = vals[name]
    out = np.full((len(PLANES), ih, n_cols), np.nan, dtype=np.float32)
    cols = k_offset + np.arange(n)
    out[:, :, n_cols - 1 - cols if flip_x else cols] = raw
    return out


def display(v, name, half_width, display_range):
    """uint16 display plane of one finished plane: 0 for NaN, else clip(rint(e), 1, 65535), e as the header states."""
    v64 = np.asarray(v, dtype=np.float32).astype(np.float64)
    if name in ('shift', 'cog'):
        e = 32768.0 + v64 * (32767.0 / float(display_range))
    elif name == 'core':
        e = v64
    else:
        e = 1.0 + v64 * (65534.0 / float(2 * half_width + 1))
    with np.errstate(invalid='ignore'):
        q = np.clip(np.rint(e), 1, 65535)
    return np.where(np.isnan(v), 0, q).astype(np.uint16)


def line_profile_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, half_width=None, display_range=None):
    """(maps float32 [5, out_h, nw], png uint16 [5, out_h, nw] or None): every plane as doppler_ref.doppler_finish, the display
    planes as display()."""
    maps = np.stack([doppler_ref.doppler_finish(r, h00, h01, h02, out_h, out_w, circle, crop)[0] for r in raw])
    png = None
    if display_range is not None:
        png = np.stack([display(m, name, half_width, display_range) for m, name in zip(maps, PLANES)])
    return maps, png


# ---- a synthetic scan with known line shift, width and depth ----
def injected_fields(ih, n, sigma=3.0, depth=0.8):
    """(shift, sigma, depth) [ih, n]: doppler_ref's shift field; sigma and depth varied by +-20 % / -25 % in two Gaussian patches
    (a 'filament' that broadens the line and a 'plage' that fills it in) and a linear ramp of sigma across the slit."""
    y = np.arange(ih, dtype=np.float64)[:, None]
    k = np.arange(n, dtype=np.float64)[None, :]
    shift = doppler_ref.injected_field(ih, n)
    fil = np.exp(-0.5 * (((y - 0.6 * ih) / (0.06 * ih)) ** 2 + ((k - 0.4 * n) / (0.12 * n)) ** 2))
    plage = np.exp(-0.5 * (((y - 0.45 * ih) / (0.1 * ih)) ** 2 + ((k - 0.55 * n) / (0.1 * n)) ** 2))
    s = sigma * (1.0 + 0.2 * fil + 0.1 * (2.0 * y / max(ih - 1, 1) - 1.0)) + 0.0 * k
    d = depth * (1.0 - 0.25 * plage) + 0.0 * y
    return shift, s, d


def disk_scan(shift, sigma, depth, iw, noise=0.004, seed=0, rotate=True):
    """doppler_ref.disk_scan's scene with the Gaussian line of frame k, slit row y displaced by shift[y, k], of width sigma[y, k] and
    depth depth[y, k] -> (frames uint16 in file layout, true line centre [ih] before the displacement, disk mask [ih, n],
    the noise-free core intensity [ih, n] on the sample scale)."""
    from solex_ser_recon_en_amd import synth
    ih, n = shift.shape
    sp = synth.scene_params(n, ih, iw)
    y = np.arange(ih, dtype=np.float64)
    x = np.arange(iw, dtype=np.float64)
    centre = synth.curve_of_row(y, ih, iw)
    lit = ((y > sp['y_lo']) & (y < sp['y_hi'])).astype(np.float64)
    frames = np.empty((n, iw, ih) if rotate else (n, ih, iw), dtype=np.uint16)
    on = np.zeros((ih, n), dtype=bool)
    core = np.zeros((ih, n))
    for k in range(n):
        r2 = ((k - sp['cx']) / sp['ax']) ** 2 + ((y - sp['cy']) / sp['ay']) ** 2
        on[:, k] = (r2 < 0.9) & (lit > 0)
        bright = np.where(r2 < 1.0, 0.35 + 0.65 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0)), sp['sky']) * lit
        line = 1.0 - depth[:, k:k + 1] * np.exp(-0.5 * ((x[None, :] - (centre + shift[:, k])[:, None]) / sigma[:, k:k + 1]) ** 2)
        img = sp['gain'] * bright[:, None] * line + noise * np.random.default_rng([seed, k]).standard_normal((ih, iw))
        core[:, k] = sp['gain'] * bright * (1.0 - depth[:, k]) * 65535.0
        img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
        frames[k] = np.rot90(img, -1) if rotate else img
    return frames, centre, on, core


def errors(planes, fit, shift, sigma, depth, centre, core, on):
    """(RMS, max) on the disk of: cog's line position against the injected one (px), width against 2 sqrt(2 ln 2) sigma (px), and
    core against the noise-free core intensity (relative)."""
    pos = planes[3].astype(np.float64) + fit[:, 3:4]
    fwhm = 2.0 * np.sqrt(2.0 * np.log(2.0)) * sigma
    out = {}
    with np.errstate(invalid='ignore', divide='ignore'):
        core_err = planes[1] / core - 1.0
    for name, err in (('cog', pos - (centre[:, None] + shift)), ('width', planes[2] - fwhm), ('core', core_err)):
        e = err[on]
        out[name] = (float(np.sqrt(np.mean(e * e))), float(np.abs(e).max()), int(np.isnan(e).sum()))
    return out


# What the restatement achieves on disk_scan(*injected_fields(400, 300), 48, noise, seed=3) at H = 10 with the fitted line placed
# off the true centre by each of -1, -0.5, 0, 0.5, 1 px (a scan's own fit lies within a pixel of it; the window moves with
# int(fit[y, 0]), and a window off-centre on the line biases cog and width): the worst (RMS, max) of errors() on the disk.
# Measured, not assumed (tests/test_lineprofile_cpu.py re-measures them): cog 0.0899 / 0.317 px, width 0.0677 / 0.193 px,
# core 0.0014 / 0.0046 without noise; cog 0.101 / 0.503 px, width 0.0991 / 0.501 px, core 0.0286 / 0.165 at synth's 0.004.
FIT_OFFSETS = (-1.0, -0.5, 0.0, 0.5, 1.0)
TOLERANCE = {0.0: {'cog': (0.09, 0.32), 'width': (0.068, 0.2), 'core': (0.0014, 0.0047)},
             0.004: {'cog': (0.101, 0.51), 'width': (0.1, 0.51), 'core': (0.029, 0.166)}}
