"""NumPy restatement of shg_map_plane_moments and shg_map_detrend, written from the arithmetic include/shg_hip.h states, not from
the kernels: NumPy for the per-pixel float64 steps, Python ints for the sums, its own Fraction solve (Gaussian elimination and a
residual sum over centred moments; the package's plane_from_moments uses Cramer's rule), the clipping loop linemaps.detrend_plane
documents, and the accuracy the restatement reaches on the injected-field scan."""
import math
from fractions import Fraction

import numpy as np

Q_SCALE = 4096
MAX_DIM = 8192


def _masked(circle):
    return circle is not None and tuple(float(v) for v in circle) != (-1.0, -1.0, -1.0)


def used_pixels(m, circle=None, prev=None):
    """bool [h, w]: finite and |v| < 64; with a circle not (dx dx + dy dy > rad rad) in float64; with prev = (a, b, g, limit)
    |(double)v - ((a + b c) + g r)| <= limit, one IEEE operation a step."""
    m = np.asarray(m, dtype=np.float32)
    h, w = m.shape
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        used = np.isfinite(m) & (np.abs(m) < np.float32(64.0))
        if _masked(circle):
            cx, cy, rad = (np.float64(v) for v in circle)
            dx, dy = c - cx, r - cy
            used &= ~(dx * dx + dy * dy > rad * rad)
        if prev is not None:
            a, b, g, limit = (np.float64(v) for v in prev)
            res = m.astype(np.float64) - ((a + b * c) + g * r)
            used &= np.abs(res) <= limit
    return used


def plane_moments(m, circle=None, prev=None):
    """The ten moments as Python ints: N, sum c, sum r, sum c^2, sum c r, sum r^2, sum q, sum q c, sum q r, sum q^2 over the used
    pixels, q = rint(4096 (double)v) (ties to even)."""
    m = np.asarray(m, dtype=np.float32)
    used = used_pixels(m, circle, prev)
    rr, cc = np.nonzero(used)
    q = np.rint(m[used].astype(np.float64) * 4096.0).astype(np.int64)
    # int64 holds every product (|q| <= 2^18, c, r < 2^13) and every sum of a map within the limits: the sums themselves as ints
    rr, cc = rr.astype(np.int64), cc.astype(np.int64)
    return [int(v) for v in (q.size, cc.sum(), rr.sum(), (cc * cc).sum(), (cc * rr).sum(), (rr * rr).sum(), q.sum(), (q * cc).sum(),
                             (q * rr).sum(), (q * q).sum())]


def solve(m10):
    """(a, b, g, sigma, n) of the ten moments: Gaussian elimination of the normal equations in Fractions; RSS from the moments
    centred on the means (sum (z - zbar)^2 - b sum (z - zbar)(c - cbar) - g sum (z - zbar)(r - rbar)).  ValueError when N < 4 or the
    system is singular."""
    n, sc, sr, scc, scr, srr, sq, sqc, sqr, sqq = (int(v) for v in m10)
    if n < 4:
        raise ValueError('N = %d' % n)
    F = Fraction
    sz, szc, szr, szz = F(sq, Q_SCALE), F(sqc, Q_SCALE), F(sqr, Q_SCALE), F(sqq, Q_SCALE * Q_SCALE)
    # centred second moments
    ccc, ccr, crr = scc - F(sc * sc, n), scr - F(sc * sr, n), srr - F(sr * sr, n)
    czc, czr, czz = szc - sz * sc / n, szr - sz * sr / n, szz - sz * sz / n
    if ccc == 0:
        # every used pixel in one column: singular
        raise ValueError('singular')
    # eliminate c from the r equation
    k = ccr / ccc
    piv = crr - k * ccr
    if piv == 0:
        raise ValueError('singular')
    g = (czr - k * czc) / piv
    b = (czc - g * ccr) / ccc
    a = (sz - b * sc - g * sr) / n
    rss = czz - b * czc - g * czr
    assert rss >= 0
    return float(a), float(b), float(g), math.sqrt(float(rss / (n - 3))), n


def display(o, display_range):
    """shg_doppler_finish's display rule on float32 o."""
    o = np.asarray(o, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.float64(32768.0) + o.astype(np.float64) * (np.float64(32767.0) / np.float64(display_range))
        q = np.clip(np.rint(e), 1, 65535)
    return np.where(np.isnan(o), 0, q).astype(np.uint16)


def detrend(m, plane, display_range=None):
    """(out float32 [h, w], png uint16 or None): out = (float)((double)v - ((a + b c) + g r))."""
    m = np.asarray(m, dtype=np.float32)
    h, w = m.shape
    a, b, g = (np.float64(v) for v in plane)
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        out = (m.astype(np.float64) - ((a + b * c) + g * r)).astype(np.float32)
    return out, None if display_range is None else display(out, display_range)


def detrend_plane(m, circle=None, clip=3.0, iterations=3, display_range=None):
    """linemaps.detrend_plane's loop on the restatement -> (out, png or None, info, the moments of every pass)."""
    trace = [plane_moments(m, circle)]
    a, b, g, sigma, n = solve(trace[0])
    n_valid = n
    for _ in range(iterations):
        if sigma == 0.0:
            break
        before = n
        trace.append(plane_moments(m, circle, (a, b, g, np.float64(clip) * np.float64(sigma))))
        a, b, g, sigma, n = solve(trace[-1])
        if n == before:
            break
    out, png = detrend(m, (a, b, g), display_range)
    info = {'a': a, 'b': b, 'g': g, 'sigma': sigma, 'n_used': n, 'n_valid': n_valid, 'passes': len(trace), 'gradient': math.hypot(b, g),
            'axis_angle_deg': math.degrees(math.atan2(g, b))}
    if _masked(circle):
        info['limb_amplitude'] = info['gradient'] * float(circle[2])
    return out, png, info, trace


def closed_form_rows(h, w, q_even, q_odd):
    """The ten moments of an h x w map, every pixel used, whose even rows hold q_even and odd rows q_odd: closed forms in Python
    ints (sums of 0..n-1 and of their squares), no pass over the pixels."""
    def s1(n):
        return n * (n - 1) // 2

    def s2(n):
        return (n - 1) * n * (2 * n - 1) // 6

    n_even, n_odd = (h + 1) // 2, h // 2
    r_even = 2 * s1(n_even)                       # sum of the even rows' indices
    r_odd = 2 * s1(n_odd) + n_odd                 # and of the odd ones'
    return [h * w, h * s1(w), w * s1(h), h * s2(w), s1(w) * s1(h), w * s2(h),
            w * (n_even * q_even + n_odd * q_odd), s1(w) * (n_even * q_even + n_odd * q_odd),
            w * (r_even * q_even + r_odd * q_odd), w * (n_even * q_even * q_even + n_odd * q_odd * q_odd)]


# What the restatement achieves on ref.doppler_scan(ref.injected_field(400, 300), 48, noise, seed=3) with the exact line centre as
# the fit: line_core_shift at H = 5, NaN off the disk (`on`), fitted with no circle, clip 3.0 and three clipped passes.  The ramp's
# true slope is 3 / 299 = 0.010033 px a column.  Measured (tests/test_detrend_cpu.py re-measures and prints them):
#   noise 0:     |b - truth| 2.258e-4 clipped (6.527e-4 unclipped); residual RMS of (detrended - blob) on the disk 0.03410 px
#   noise 0.004: |b - truth| 2.863e-4 clipped (6.357e-4 unclipped); residual RMS 0.08552 px
# The tolerances are those figures rounded up in their last digit, as linemaps_ref.TOLERANCE's are.
TOLERANCE = {'slope': {0.0: 2.3e-4, 0.004: 2.9e-4}, 'residual': {0.0: 0.0342, 0.004: 0.0856}}
