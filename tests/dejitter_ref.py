"""NumPy restatement of shg_column_limb_u16 and shg_column_shift_u16, written from the arithmetic include/shg_hip.h states, not from the
kernels, and of the host steps of solex_ser_recon_en_amd/dejitter.py (the threshold, the crossings, the line with its refits, the
fill, the Keys weights) from DESIGN.md section 24.  Also the scene the accuracy is measured on -- a raw-disk-like image: a sheared
ellipse with limb darkening, a spot, blur, noise and a sub-pixel shift a column planted by supersampling -- and TOLERANCE, what the
restatement achieves on it."""
import numpy as np

ONE = 16384


# ---- the two calls ----
def column_limb(img, window, threshold):
    """shg_column_limb_u16 -> int32 [w, 6]."""
    img = np.asarray(img)
    h, w = img.shape
    k, kt = int(window), int(window) * int(threshold)
    out = np.full((w, 6), -1, np.int32)
    ni = h - k + 1
    if h < k + 2:
        return out
    a = img.astype(np.int64)
    s = np.zeros((ni, w), np.int64)
    for j in range(k):
        s += a[j:j + ni]
    above = s >= kt
    for c in range(w):
        col = above[:, c]
        if col[0] or col[ni - 1] or not col.any():
            continue
        rise = np.flatnonzero(~col[:-1] & col[1:]) + 1              # i >= 1 with !A[i - 1] && A[i]
        fall = np.flatnonzero(col[:-1] & ~col[1:])                  # i <= ni - 2 with A[i] && !A[i + 1]
        i, b = int(rise[0]), int(fall[-1])
        out[c] = (i, s[i - 1, c], s[i, c], b, s[b, c], s[b + 1, c])
    return out


def column_shift(planes, offset, weight):
    """shg_column_shift_u16 on [h, w] or [n, h, w] -> uint16 of that shape."""
    planes = np.asarray(planes)
    stack = planes[None] if planes.ndim == 2 else planes
    n, h, w = stack.shape
    offset, weight = np.asarray(offset, dtype=np.int64), np.asarray(weight, dtype=np.int64)
    assert offset.shape == (w,) and weight.shape == (w, 4)
    rows = np.arange(h, dtype=np.int64)[:, None]
    cols = np.broadcast_to(np.arange(w)[None, :], (h, w))
    acc = np.zeros((n, h, w), np.int64)
    for k in range(4):
        src = np.clip(rows + offset[None, :] + (k - 1), 0, h - 1)
        acc += weight[None, None, :, k] * stack[:, src, cols].astype(np.int64)
    out = np.clip((acc + 8192) >> 14, 0, 65535).astype(np.uint16)
    return out[0] if planes.ndim == 2 else out


# ---- the host steps ----
def threshold(img, level=0.2):
    flat = np.sort(np.asarray(img).ravel())
    lo, hi = int(flat[int(0.05 * (flat.size - 1))]), int(flat[int(0.95 * (flat.size - 1))])
    return lo + int(float(level) * (hi - lo))


def crossings(table, window, threshold):
    """-> (top, bottom) float64 [w], NaN where the table holds -1."""
    kt, half = int(window) * int(threshold), float(int(window) - 1) / 2.0
    top, bot = np.full(len(table), np.nan), np.full(len(table), np.nan)
    for c, (i, p, q, b, u, v) in enumerate(np.asarray(table).tolist()):
        if i < 0:
            continue
        top[c] = (float(i - 1) + float(kt - p) / float(q - p)) + half
        bot[c] = (float(b) + float(u - kt) / float(u - v)) + half
    return top, bot


def line(x, y):
    mx, my = x.mean(), y.mean()
    slope = ((x - mx) * (y - my)).sum() / ((x - mx) * (x - mx)).sum()
    return float(slope), float(my - slope * mx)


def shifts(top, bottom, min_chord=0.3, clip=3.0, max_shift=8.0):
    """The host steps of dejitter.measure -> {'shift', 'measured', 'slope', 'intercept', 'rms', 'max', 'n_measured',
    'rejected_by_max_shift'}; ValueError for fewer than 16 columns at any step."""
    w = top.shape[0]
    x = np.arange(w, dtype=np.float64)
    has = np.isfinite(top) & np.isfinite(bottom)
    if has.sum() < 16:
        raise ValueError('too few columns')
    mid, chord = (top + bottom) / 2.0, bottom - top
    ok = has.copy()
    ok[has] = chord[has] >= float(min_chord) * chord[has].max()
    if ok.sum() < 16:
        raise ValueError('too few columns')
    use = ok.copy()
    slope, intercept = line(x[use], mid[use])
    for _ in range(3):
        res = mid[use] - (slope * x[use] + intercept)
        centre = np.median(res)
        sigma = 1.4826 * np.median(np.abs(res - centre))
        keep = ok.copy()
        keep[ok] = np.abs((mid[ok] - (slope * x[ok] + intercept)) - centre) <= float(clip) * sigma
        if sigma == 0.0 or keep.sum() < 16 or np.array_equal(keep, use):
            break
        use = keep
        slope, intercept = line(x[use], mid[use])
    raw = np.zeros(w)
    raw[has] = mid[has] - (slope * x[has] + intercept)
    measured = ok & (np.abs(raw) <= float(max_shift))
    if measured.sum() < 16:
        raise ValueError('too few columns')
    at = np.flatnonzero(measured)
    shift = np.empty(w)
    for c in range(w):
        j = int(np.searchsorted(at, c))
        if j == 0:
            shift[c] = raw[at[0]]
        elif j == at.size:
            shift[c] = raw[at[-1]]
        elif at[j] == c:
            shift[c] = raw[c]
        else:
            a, b = at[j - 1], at[j]
            shift[c] = raw[a] + (raw[b] - raw[a]) * (c - a) / (b - a)
    return {'shift': shift, 'measured': measured, 'slope': slope, 'intercept': intercept, 'rms': float(np.sqrt(np.mean(raw[measured] ** 2))),
            'max': float(np.abs(raw[measured]).max()), 'n_measured': int(measured.sum()), 'rejected_by_max_shift': int((ok & ~measured).sum()),
            'crossing': int(has.sum())}


def measure(img, threshold_=None, level=0.2, window=5, **rest):
    t = threshold(img, level) if threshold_ is None else int(threshold_)
    top, bottom = crossings(column_limb(img, window, t), window, t)
    rec = shifts(top, bottom, **rest)
    rec.update(top=top, bottom=bottom, threshold=t, window=window)
    return rec


def weights(shift):
    """-> (offset int32 [w], weight int32 [w, 4])."""
    s = np.asarray(shift, dtype=np.float64)
    o = np.floor(s)
    q = np.empty((s.size, 4), np.int64)
    for c, t in enumerate((s - o).tolist()):
        k = (((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * (t * t) + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * (t * t))
        q[c] = [int(np.rint(v * 16384.0)) for v in k]
        q[c, 1] += ONE - q[c].sum()
    return o.astype(np.int32), q.astype(np.int32)


def apply(planes, shift):
    return column_shift(planes, *weights(shift))


# ---- the scene ----
H, W = 200, 260
SHEAR = 0.05
SKY, CENTRE, NOISE = 600.0, 30000.0, 150.0            # (the noise: 0.5 % of the disk's centre)


def planted(w=W, rms=0.8, seed=1):
    """A shift a column, independent, normal with that rms; one column three rows off."""
    jitter = np.random.default_rng(seed).normal(0.0, rms, w)
    jitter[100 % w] = 3.0
    return jitter


def scene(h=H, w=W, jitter=None, noise=NOISE, seed=2, supersample=8, blur=1.2, shear=SHEAR):
    """A raw-disk-like uint16 image [h, w]: an ellipse of semi-axes 0.385 w along the columns and 0.4 h along the rows around
    (0.493 w, 0.488 h), sheared by `shear` rows a column, limb darkening 0.4 .. 1, a spot, every column blurred by a Gaussian of
    `blur` rows and moved down by jitter[c] rows (`supersample` samples a row), plus normal noise."""
    jitter = np.zeros(w) if jitter is None else np.asarray(jitter, dtype=np.float64)
    a, b, cx, cy = 0.385 * w, 0.4 * h, 0.493 * w + 0.1, 0.488 * h
    ss = int(supersample)
    rows = (np.arange(h * ss) + 0.5) / ss - 0.5
    reach = 5 * ss
    taps = np.exp(-0.5 * (np.arange(-reach, reach + 1) / (blur * ss)) ** 2)
    taps /= taps.sum()
    img = np.empty((h, w))
    for c in range(w):
        rr = rows - jitter[c]
        x, y = (c - cx) / a, (rr - cy - shear * (c - cx)) / b
        d2 = x * x + y * y
        v = np.where(d2 < 1.0, CENTRE * (0.4 + 0.6 * np.sqrt(np.clip(1.0 - d2, 0.0, 1.0))), SKY)
        v = v * (1.0 - 0.5 * np.exp(-(((c - 0.58 * w) / 4.0) ** 2 + ((rr - 0.45 * h) / 4.0) ** 2)))
        v = np.convolve(np.pad(v, reach, mode='edge'), taps, 'valid')
        img[:, c] = v.reshape(h, ss).mean(axis=1)
    img = img + np.random.default_rng(seed).normal(0.0, noise, img.shape) if noise else img
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16)


def detrended(err, where):
    """err less the line through its values at `where` (the common mean and slope, which the fitted line absorbs)."""
    x = np.arange(err.shape[0], dtype=np.float64)
    slope, intercept = line(x[where], err[where])
    return err - (slope * x + intercept)


def accuracy(measure_fn=measure, apply_fn=apply):
    """The three measures on the scene, through the given measure and apply -> {'shift_rms', 'shift_max', 'residual', 'floor'} and
    the two conditions' figures ('rejected_by_max_shift', 'measured_fraction')."""
    jitter = planted()
    img = scene(jitter=jitter)
    rec = measure_fn(img)
    m = rec['measured']
    err = detrended(rec['shift'] - jitter, m)[m]
    again = measure_fn(apply_fn(img, rec['shift']))
    both = m & again['measured']
    still = measure_fn(scene())
    return {'shift_rms': float(np.sqrt(np.mean(err ** 2))), 'shift_max': float(np.abs(err).max()),
            'residual': float(np.sqrt(np.mean(detrended(again['shift'], both)[both] ** 2))), 'floor': still['rms'],
            'rejected_by_max_shift': rec['rejected_by_max_shift'] + still['rejected_by_max_shift'],
            'measured_fraction': min(rec['n_measured'] / rec['crossing'], still['n_measured'] / still['crossing']),
            'planted_rms': float(np.sqrt(np.mean(jitter[m] ** 2))), 'slope': rec['slope']}


# What the restatement achieves on the scene (tests/test_dejitter_cpu.py re-measures and prints them); each bound is the measured
# value plus a quarter, rounded up to two digits:
#   the shifts recovered, of 0.772 px rms planted, less their common mean and slope: 0.027745 px rms, the worst column 0.065947 px;
#   the midpoints' residual after apply(), measured again: 0.005340 px rms;
#   the shifts "found" on the scene without jitter, the false-correction floor: 0.025515 px rms;
#   no column rejected by max_shift, 95.5 % of the columns that cross the disk measured; the line's slope 0.04975 for a shear of 0.05.
TOLERANCE = {'shift_rms': 0.035, 'shift_max': 0.083, 'residual': 0.0067, 'floor': 0.032}
