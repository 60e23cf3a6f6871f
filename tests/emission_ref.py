"""NumPy restatement of the emission-line maps' two calls (include/shg_hip.h: shg_line_emission, shg_line_emission_finish), written
from the arithmetic the header states, not from the kernels: the GPU must match these bit for bit.  The window, the column
placement, the warp and the display scales the other line maps share come from tests/linemaps_ref.py.  Also the synthetic scene
(two prominences off opposite limbs of linemaps_ref.disk_scan's disk, each with its own injected shift, width and amplitude) and
the accuracy and gate rates the restatement reaches on it."""
import numpy as np

from tests import linemaps_ref as ref
from tests.linemaps_ref import _map, _warp, display

PLANES = ('shift', 'peak', 'width', 'cog', 'flux')
KINDS = ('shift', 'core', 'width', 'cog', 'flux')            # linemaps_ref.display's scale of each plane; flux has its own


def _planes(p, lo, hi, ref_pos, min_excess):
    """The five PLANES of the profiles p [n, iw] over [lo, hi], float32 [5, n]."""
    seg = p[:, lo:hi + 1]
    n, m = seg.shape
    out = np.full((len(PLANES), n), np.nan, dtype=np.float32)
    jrel = np.argmax(seg, axis=1)                                # the first maximum
    k = np.flatnonzero((jrel > 0) & (jrel < m - 1))
    rk = jrel[k]
    a, b, e = seg[k, rk - 1], seg[k, rk], seg[k, rk + 1]
    den = a + e - 2 * b
    b2 = seg[k, 0] + seg[k, -1]
    peak_d = b.astype(np.float64) - ((a - e) * (a - e)).astype(np.float64) / (8.0 * den.astype(np.float64))
    excess_d = peak_d - 0.5 * b2.astype(np.float64)
    ok = excess_d >= np.float64(min_excess)
    k, rk, a, b, e, den, b2, peak_d, excess_d = (v[ok] for v in (k, rk, a, b, e, den, b2, peak_d, excess_d))
    sk = seg[k]
    out[0, k] = (((lo + rk).astype(np.float64) + (a - e).astype(np.float64) / (2 * den).astype(np.float64)) - ref_pos).astype(np.float32)
    out[1, k] = excess_d.astype(np.float32)
    # the width: the crossings of half, downward either side of the maximum
    half = 0.5 * (0.5 * b2.astype(np.float64) + peak_d)
    le = sk <= half[:, None]
    idx = np.arange(m)[None, :]
    jl = np.where(le & (idx < rk[:, None]), idx, -1).max(axis=1)
    jr = np.where(le & (idx > rk[:, None]), idx, m).min(axis=1)
    has = (b.astype(np.float64) > half) & (jl >= 0) & (jr < m)
    rows = np.arange(sk.shape[0])
    jl, jr = np.clip(jl, 0, m - 2), np.clip(jr, 1, m - 1)
    pl, pl1, pr, pr1 = sk[rows, jl], sk[rows, jl + 1], sk[rows, jr], sk[rows, jr - 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        xl = (lo + jl).astype(np.float64) + (half - pl.astype(np.float64)) / (pl1 - pl).astype(np.float64)
        xr = (lo + jr).astype(np.float64) - (half - pr.astype(np.float64)) / (pr1 - pr).astype(np.float64)
        out[2, k] = np.where(has, (xr - xl).astype(np.float32), np.float32(np.nan))
    # the sums of p - background
    jj = np.arange(lo, lo + m, dtype=np.int64)
    s0 = 2 * sk.sum(axis=1) - m * b2
    s1 = 2 * (sk * jj).sum(axis=1) - b2 * jj.sum()
    with np.errstate(invalid='ignore', divide='ignore'):
        cog = (s1.astype(np.float64) / s0.astype(np.float64) - ref_pos).astype(np.float32)
    out[3, k] = np.where(s0 > 0, cog, np.float32(np.nan))
    out[4, k] = np.where(s0 > 0, (0.5 * s0.astype(np.float64)).astype(np.float32), np.float32(np.nan))
    return out


def check_min_excess(min_excess):
    """The header's rule: finite and >= 0 (else SHG_E_ARG)."""
    if not (np.isfinite(min_excess) and min_excess >= 0):
        raise ValueError('min_excess must be finite and >= 0')
    return float(min_excess)


def line_emission(frames, fit, half_width, shift=0, min_excess=0.0, flip_x=False, n_cols=None, k_offset=0):
    """planes float32 [5, ih, n_cols] (PLANES order) of frames [n, H, W] (file layout)."""
    e = check_min_excess(min_excess)
    return _map(frames, fit, half_width, shift, len(PLANES), lambda p, lo, hi, r: _planes(p, lo, hi, r, e), flip_x, n_cols, k_offset)


def check_ring(ring):
    """The header's rule for ring4 (None: no mask): no NaN, r_out >= 0, r_out >= r_in."""
    if ring is None:
        return None
    cx, cy, r_in, r_out = (float(v) for v in ring)
    if np.isnan([cx, cy, r_in, r_out]).any() or r_out < 0 or r_out < r_in:
        raise ValueError('ring needs numbers and 0 <= r_out >= r_in')
    return cx, cy, r_in, r_out


def ring_keep(out_h, out_w, ring):
    """bool [out_h, out_w]: the pixels the ring keeps, by the circle test's float64 steps."""
    if ring is None:
        return np.ones((out_h, out_w), dtype=bool)
    cx, cy, r_in, r_out = ring
    r = np.arange(out_h, dtype=np.float64)[:, None]
    c = np.arange(out_w, dtype=np.float64)[None, :]
    dx, dy = c - cx, r - cy
    d2 = dx * dx + dy * dy
    with np.errstate(invalid='ignore', over='ignore'):
        off = d2 > r_out * r_out
        if r_in >= 0:
            off |= d2 <= r_in * r_in
    return ~off


def flux_display(v, half_width):
    """The flux plane's display: 0 for NaN, else clip(rint((double)v / (2H + 1)), 1, 65535)."""
    v64 = np.asarray(v, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        q = np.clip(np.rint(v64 / np.float64(2 * half_width + 1)), 1, 65535)
    return np.where(np.isnan(v), 0, q).astype(np.uint16)


def line_emission_finish(raw, h00, h01, h02, out_h, out_w, ring=None, crop=None, half_width=None, display_range=None):
    """(maps float32 [5, out_h, nw], png uint16 [5, out_h, nw] or None): every plane warped as shg_doppler_finish without a circle,
    NaN outside the ring, then the crop."""
    ring = check_ring(ring)
    keep = ring_keep(out_h, out_w, ring)
    maps = []
    for plane in raw:
        v = _warp(plane, h00, h01, h02, out_h, out_w, None, None)
        v[~keep] = np.nan
        if crop is not None:
            nw, lo, dx0, n = (int(q) for q in crop)
            out = np.full((out_h, nw), np.nan, dtype=np.float32)
            out[:, dx0:dx0 + n] = v[:, lo:lo + n]
            v = out
        maps.append(v)
    maps = np.stack(maps)
    if display_range is None:
        return maps, None
    return maps, np.stack([flux_display(m, half_width) if kind == 'flux' else display(m, kind, half_width, display_range)
                           for m, kind in zip(maps, KINDS)])


# ---- the emission scene: two prominences off opposite limbs ----
# (frame, slit row, radius in frames, radius in rows, amplitude on the relative scale, shift px, sigma px), as fractions of (n, ih)
PROMINENCES = ((0.045, 0.46, 0.028, 0.07, 0.10, 1.5, 2.0), (0.955, 0.58, 0.028, 0.09, 0.075, -1.0, 2.8))
SIGMA_ADU = 0.004 * 65535.0                 # the synthetic scans' noise on the sample scale
MIN_EXCESS = 6.0 * SIGMA_ADU                # the gate the rates are measured at


def scene(ih, n, iw, noise=0.004, seed=3, rotate=True, bits=16, flat=False):
    """(frames, dict(centre [ih], amp [ih, n] the injected amplitude on the sample scale, shift, sigma [ih, n] (NaN off the
    prominences), sky bool [ih, n]: lit slit rows off the disk, prom bool [ih, n]: amp > 0)).  The scattered light off the limb keeps
    disk_scan's absorption line; the emission A G(x - centre - shift) is added relative to the sky continuum.  flat: each prominence
    a sharp-edged patch of its full amplitude (for the overlay on the products)."""
    from solex_ser_recon_en_amd import synth
    sp = synth.scene_params(n, ih, iw)
    y = np.arange(ih, dtype=np.float64)[:, None]
    k = np.arange(n, dtype=np.float64)[None, :]
    r2 = ((k - sp['cx']) / sp['ax']) ** 2 + ((y - sp['cy']) / sp['ay']) ** 2
    lit = (y > sp['y_lo']) & (y < sp['y_hi'])
    sky = lit & (r2 >= 1.0) & np.ones((ih, n), dtype=bool)
    cont_sky = sp['gain'] * sp['sky']
    amp = np.zeros((ih, n))
    shift = np.full((ih, n), np.nan)
    sigma = np.full((ih, n), np.nan)
    for fk, fy, rk, ry, a0, s, sg in PROMINENCES:
        g = a0 * np.exp(-0.5 * (((k - fk * n) / (rk * n)) ** 2 + ((y - fy * ih) / (ry * ih)) ** 2))
        g = np.where(sky & (r2 >= 1.04) & (g > 0.05 * a0), g, 0.0)
        if flat:
            g = np.where(g > 0.3 * a0, a0, 0.0)
        amp = amp + g
        shift = np.where(g > 0, s, shift)
        sigma = np.where(g > 0, sg, sigma)
    rel = amp / cont_sky                                         # relative to the sky continuum

    def line(x, c, kk):
        absorb = 1.0 - sp['depth'] * np.exp(-0.5 * ((x - c[:, None]) / sp['sigma']) ** 2)
        on = rel[:, kk] > 0
        sg = np.where(on, sigma[:, kk], 1.0)[:, None]
        sh = np.where(on, shift[:, kk], 0.0)
        return absorb + rel[:, kk:kk + 1] * np.exp(-0.5 * ((x - (c + sh)[:, None]) / sg) ** 2)

    frames, centre, _, _ = ref.disk_scan(line, ih, n, iw, noise, seed, rotate)
    if bits == 8:
        frames = (frames >> 8).astype(np.uint8)
    return frames, dict(centre=centre, amp=amp * 65535.0, shift=shift, sigma=sigma, sky=sky, prom=amp > 0)


def scene_errors(planes, fit, truth, min_amp):
    """{shift, cog (px against the injected line position), width (px against 2 sqrt(2 ln 2) sigma), peak (relative, against the
    injected amplitude)}: (RMS, max, NaN count) over the prominence pixels with injected amplitude > min_amp."""
    sel = truth['prom'] & (truth['amp'] > min_amp)
    pos = truth['centre'][:, None] + truth['shift']
    fwhm = 2.0 * np.sqrt(2.0 * np.log(2.0)) * truth['sigma']
    with np.errstate(invalid='ignore', divide='ignore'):
        errs = (('shift', planes[0].astype(np.float64) + fit[:, 3:4] - pos), ('cog', planes[3].astype(np.float64) + fit[:, 3:4] - pos),
                ('width', planes[2] - fwhm), ('peak', planes[1] / truth['amp'] - 1.0))
    out = {}
    for name, err in errs:
        e = err[sel]
        nans = int(np.isnan(e).sum())
        e = e[~np.isnan(e)]
        out[name] = (float(np.sqrt(np.mean(e * e))), float(np.abs(e).max()), nans)
    return out


def gate_rates(planes, truth, min_excess):
    """(fraction of emission-free sky pixels that come out finite, fraction of prominence pixels with injected amplitude above twice
    min_excess that come out NaN, the number of those prominence pixels that are finite), on the peak plane."""
    finite = np.isfinite(planes[1])
    empty = truth['sky'] & ~truth['prom']
    strong = truth['prom'] & (truth['amp'] > 2.0 * min_excess)
    return (float(finite[empty].mean()), float((~finite[strong]).mean()), int(finite[strong].sum()))


# What the restatement achieves on scene(400, 300, 48, noise) at H = 10 with the exact line centre as the fit, measured (the CPU
# test re-measures them) and rounded up by at most 10 %: (RMS, max) over the prominence pixels with injected amplitude above
# 2 MIN_EXCESS, at min_excess = MIN_EXCESS.  The absorption line of the scattered light under the emission is part of the scene: it
# lowers the peak (by up to 0.8 of the sky continuum) and, displaced from the emission, pulls shift and cog towards itself.
# GATE: the two rates of gate_rates() at MIN_EXCESS with the scans' noise.
# Measured with the fitted line placed off the true centre by each of linemaps_ref.FIT_OFFSETS px (a scan's own fit lies within a
# pixel of it), the worst of them: without noise shift 0.173 / 0.271 px, cog 0.512 / 0.981 px, width 0.287 / 0.473 px, peak 0.189 /
# 0.256; at 0.004 shift 0.450 / 1.981, cog 1.406 / 23.80 (one pixel's S0 falls to <= 0: NaN; cog weights the whole window, the
# absorption dip and the noise included, and is the poorest plane on faint emission), width 0.661 / 2.713, peak 0.171 / 0.437.
# 1894 prominence pixels lie above 2 MIN_EXCESS; all come out finite, and none of the emission-free sky does: both rates are 0.
TOLERANCE = {0.0: {'shift': (0.18, 0.28), 'cog': (0.52, 1.0), 'width': (0.29, 0.48), 'peak': (0.19, 0.26)},
             0.004: {'shift': (0.46, 2.0), 'cog': (1.42, 24.0), 'width': (0.67, 2.75), 'peak': (0.175, 0.44)}}
NAN_ALLOWED = {0.0: {'shift': 0, 'cog': 0, 'width': 0, 'peak': 0}, 0.004: {'shift': 0, 'cog': 1, 'width': 0, 'peak': 0}}
GATE = {'finite_sky': 0.0, 'lost_prominence': 0.0}              # the caps: the measured rates plus 10 %


# ---- the adversarial rows, mirrored ----
def mirrored_profiles(n, ih, iw, bits, half_width, shift=0, seed=0):
    """profile_adversarial.profiles() with every raw sample P replaced by Q - P (Q = 65535 for 16-bit files, 255 for 8-bit ones):
    the absorption classes (ties, plateaus, window edges, exact half levels) as emission -> (P on the sample scale, fit, classes)."""
    from tests import profile_adversarial as adv
    P, fit, cls = adv.profiles(n, ih, iw, bits, half_width, shift, seed)
    q, scale = (65535, 1) if bits == 16 else (255, 256)
    return (q - P // scale) * scale, fit, cls
