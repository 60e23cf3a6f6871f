"""NumPy restatement of shg_wavelet_sharpen_u16 and shg_wavelet_noise_u16, written from the arithmetic include/shg_hip.h states,
not from the kernels: whole planes of int64, the reflection as index arrays, a row pass and a column pass a level, a sort for the
median.  Also an independently written dense form of one level (np.pad(mode='reflect') and the explicit 25 taps in float64), the
derivable quantities the CPU tests hold the restatement to (the layers' noise factors from 1-D kernels, the transfer function), the
synthetic scene the accuracy is measured on, the measures themselves and the bounds (TOLERANCE)."""
import numpy as np

from tests import flatten_ref as fr

MAX_LEVELS = 6
MAX_GAIN_Q8 = 4096
MAX_THRESHOLD_Q6 = 1 << 22
K5 = np.array([1, 4, 6, 4, 1], dtype=np.int64)


# ---- the arithmetic of the header ----
def reflect_index(i, n):
    """R(i, n) for an int64 array i."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)                                                 # (non-negative)
    return np.where(i >= n, p - i, i)


def smooth(c, hole):
    """c_j (int64 [h, w]) from c_(j-1): S by a row pass and a column pass, nothing rounded between them, then (S + 128) >> 8."""
    h, w = c.shape
    rows = np.zeros_like(c)
    for l in range(5):
        rows += K5[l] * c[:, reflect_index(np.arange(w) + (l - 2) * hole, w)]
    s = np.zeros_like(c)
    for k in range(5):
        s += K5[k] * rows[reflect_index(np.arange(h) + (k - 2) * hole, h), :]
    assert s.max(initial=0) < 1 << 30 and s.min(initial=0) >= 0
    return (s + 128) >> 8


def wavelet_planes(img, levels):
    """int32 [L + 1, h, w]: w_1 .. w_L, then c_L."""
    img = np.asarray(img, dtype=np.uint16)
    assert img.ndim == 2 and 1 <= levels <= MAX_LEVELS
    c = img.astype(np.int64) * 64
    out = np.zeros((levels + 1,) + img.shape, dtype=np.int32)
    for j in range(1, levels + 1):
        nxt = smooth(c, 1 << (j - 1))
        out[j - 1] = c - nxt
        c = nxt
    out[levels] = c
    return out


def soft(w, t):
    w = np.asarray(w, dtype=np.int64)
    return np.sign(w) * np.maximum(np.abs(w) - int(t), 0)


def recombine(planes, gain_q8, threshold_q6):
    levels = planes.shape[0] - 1
    gain_q8, threshold_q6 = [int(g) for g in gain_q8], [int(t) for t in threshold_q6]
    assert len(gain_q8) == levels and len(threshold_q6) == levels
    assert all(0 <= g <= MAX_GAIN_Q8 for g in gain_q8) and all(0 <= t <= MAX_THRESHOLD_Q6 for t in threshold_q6)
    acc = 256 * planes[levels].astype(np.int64)
    for j in range(levels):
        acc += gain_q8[j] * soft(planes[j], threshold_q6[j])
    assert np.abs(acc).max(initial=0) < 1 << 37
    return np.clip((acc + 8192) >> 14, 0, 65535).astype(np.uint16)      # (>> on int64: the floor towards -infinity)


def sharpen(img, gain_q8, threshold_q6=None):
    """(out uint16 [h, w], planes int32 [L + 1, h, w])."""
    levels = len(gain_q8)
    planes = wavelet_planes(img, levels)
    return recombine(planes, gain_q8, [0] * levels if threshold_q6 is None else threshold_q6), planes


def noise(img, circle=None):
    """(the lower median of |w_1| over the set, in Q6; the size of the set)."""
    img = np.asarray(img, dtype=np.uint16)
    on = np.ones(img.shape, dtype=bool)
    if circle is not None and tuple(float(t) for t in circle) != (-1.0, -1.0, -1.0):
        on = fr.rings(img.shape[0], img.shape[1], circle)[0]
    v = np.sort(np.abs(wavelet_planes(img, 1)[0].astype(np.int64))[on])
    n = int(v.size)
    return (int(v[(n - 1) // 2]) if n else 0), n


# ---- an independent dense form of one level ----
def dense_smooth(c, hole):
    """c_j from c_(j-1) (integers as float64: every value stays below 2^53, so float64 is exact): the plane padded by 2 holes with
    np.pad(mode='reflect'), then the 25 taps one by one."""
    c = np.asarray(c, dtype=np.float64)
    h, w = c.shape
    p = np.pad(c, 2 * hole, mode='reflect')
    k2 = np.outer(K5, K5).astype(np.float64)
    s = np.zeros((h, w), dtype=np.float64)
    for k in range(5):
        for l in range(5):
            s += k2[k, l] * p[k * hole:k * hole + h, l * hole:l * hole + w]
    return np.floor((s + 128.0) / 256.0)


def dense_planes(img, levels):
    c = np.asarray(img, dtype=np.float64) * 64.0
    out = []
    for j in range(1, levels + 1):
        nxt = dense_smooth(c, 1 << (j - 1))
        out.append(c - nxt)
        c = nxt
    return np.stack(out + [c])


# ---- derivable quantities ----
def smoothing_kernel_1d(j):
    """The 1-D kernel of the unrounded c_j: K / 16 with holes 1, 2, .. 2^(j-1) convolved with one another, float64 [2 (2^(j+1) - 2) + 1]."""
    out = np.array([1.0])
    for i in range(j):
        step = np.zeros(4 * (1 << i) + 1)
        step[::1 << i] = K5 / 16.0
        out = np.convolve(out, step)
    return out


def layer_noise_factors(levels):
    """The standard deviation of unit white noise in w_j, from the 1-D kernels: w_j's 2-D kernel is P_(j-1) x P_(j-1) - P_j x P_j,
    whose sum of squares is a^2 - 2 b^2 + c^2 with a = sum P_(j-1)^2, b = sum P_(j-1) P_j (centres aligned), c = sum P_j^2."""
    out = []
    for j in range(1, levels + 1):
        p0, p1 = smoothing_kernel_1d(j - 1), smoothing_kernel_1d(j)
        pad = (p1.size - p0.size) // 2
        p0 = np.pad(p0, pad)
        a, b, c = (p0 * p0).sum(), (p0 * p1).sum(), (p1 * p1).sum()
        out.append(float(np.sqrt(a * a - 2.0 * b * b + c * c)))
    return out


def transfer(omega, gains):
    """T(omega) of the unrounded transform along one axis: P_L + sum g_j (P_(j-1) - P_j), P_j = prod_(i <= j) cos^4(omega 2^(i-1) / 2)."""
    p = [1.0]
    for i in range(1, len(gains) + 1):
        p.append(p[-1] * np.cos(omega * (1 << (i - 1)) / 2.0) ** 4)
    return p[-1] + sum(g * (p[j] - p[j + 1]) for j, g in enumerate(gains))


def transfer_bound(gain_q8):
    """The bound, in counts, on |amplitude out - T A| for a sinusoid far from the borders: every level rounds
    c_j by at most 1/2 Q6 unit = 1/128 count, and the error e_j of c_j is that plus a weighted mean of e_(j-1): |e_j| <= j / 128.  w_j =
    c_(j-1) - c_j is off by at most (2 j - 1) / 128, c_L by L / 128; the output rounding adds 1/2.  A fitted amplitude of a pure error
    bounded by E is at most 2 E off (the projection on a sinusoid of unit amplitude has norm 2 under the mean)."""
    levels = len(gain_q8)
    err = levels / 128.0 + sum(g / 256.0 * (2 * j + 1) / 128.0 for j, g in enumerate(gain_q8)) + 0.5
    return 2.0 * err


# ---- the accuracy: flatten's synthetic disk with Gaussian noise of known sigma ----
NOISE = 0.004                                # on the relative scale: 262.14 counts
SMOOTH_REGION = 0.6                          # the smooth part of the disk: within 0.6 R, 20 px clear of the spot


def scene():
    """(noisy uint16 [260, 250], the noise-free model in counts float64, circle, sigma in counts, the smooth region bool)."""
    img, circle = fr.synthetic_disk(NOISE, seed=0)
    h, w = fr.SCENE['h'], fr.SCENE['w']
    cx, cy, rad = circle
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    rho = np.sqrt((c - cx) ** 2 + (r - cy) ** 2)
    model = np.where(rho <= rad, fr.SCENE['scale'] * fr.law(rho / rad), fr.SCENE['sky'])
    model = model * (1.0 - 0.4 * np.exp(-0.5 * (((c - (cx + rad / 3.0)) / 5.0) ** 2 + ((r - (cy - rad / 5.0)) / 5.0) ** 2)))
    spot = np.hypot(c - (cx + rad / 3.0), r - (cy - rad / 5.0))
    return img, model * 65535.0, circle, NOISE * 65535.0, (rho <= SMOOTH_REGION * rad) & (spot > 20.0)


def scene_measures(sigma_of, sharpen_of):
    """sigma_of(img, circle) -> the estimated sigma in counts (region 0.9); sharpen_of(img, circle) -> the image sharpened with unity
    gains and the default denoise -> {'sigma': |estimate / planted - 1|, 'residual': the standard deviation of (output - model) over
    the smooth region, as a fraction of the planted sigma}."""
    img, model, circle, sigma, region = scene()
    est = float(sigma_of(img, circle))
    out = np.asarray(sharpen_of(img, circle), dtype=np.float64)
    return {'sigma': abs(est / sigma - 1.0), 'residual': float((out - model)[region].std() / sigma), 'estimate': est}


# What the restatement achieves on scene() (tests/test_sharpen_cpu.py re-measures and prints them).  Each bound is the measured value
# plus a quarter, rounded up to two significant digits; the quarter covers other seeds of the same scene.
#   sigma: the estimate 263.124 counts for 262.14 planted, off by 0.003755 of it (the curvature of the law and the spot add to the
#   finest layer); residual: 0.171951 of the planted noise is left on the smooth part at denoise (3, 1, 0, 0) and unity gains
TOLERANCE = {'sigma': 0.0047, 'residual': 0.22}
