"""NumPy restatement of shg_ring_medians_u16, shg_ring_flatten_u16 and flatten.gain_from_profile, written from the arithmetic
include/shg_hip.h and the function's docstring state, not from the kernels: every per-pixel step in float64 with np.sqrt and
np.rint, a sort of each ring's values for the order statistics, a Python loop for the running mean.  Also the synthetic disk the
accuracy is measured on, the measures themselves and the bounds (TOLERANCE)."""
import numpy as np

MAX_DIM = 16384
MAX_RINGS = 16384


def n_rings(circle):
    return int(np.floor(np.float64(circle[2]))) + 1


def rings(h, w, circle):
    """(on bool [h, w], ring int64 [h, w], d2 float64 [h, w]): on the disk iff not (dx dx + dy dy > rad rad) in float64; the ring is the largest
    integer k with (double)k (double)k <= d2 -- from floor(sqrt(d2)), corrected by one step either way with the two comparisons."""
    cx, cy, rad = (np.float64(v) for v in circle)
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    dx, dy = c - cx, r - cy
    d2 = dx * dx + dy * dy
    on = ~(d2 > rad * rad)
    k = np.floor(np.sqrt(d2)).astype(np.int64)
    k -= (k.astype(np.float64) * k.astype(np.float64) > d2)
    k += ((k + 1).astype(np.float64) * (k + 1).astype(np.float64) <= d2)
    assert (k.astype(np.float64) ** 2 <= d2).all() and ((k + 1).astype(np.float64) ** 2 > d2).all()
    return on, k, d2


def ring_medians(img, circle):
    """(count uint32 [K], lo uint16 [K], hi uint16 [K]): by sorting every ring's values."""
    img = np.asarray(img, dtype=np.uint16)
    on, k, _ = rings(*img.shape, circle)
    kk = n_rings(circle)
    assert not on.any() or k[on].max() < kk
    count, lo, hi = np.zeros(kk, np.uint32), np.zeros(kk, np.uint16), np.zeros(kk, np.uint16)
    order = np.argsort(k[on], kind='stable')
    ring_sorted, values = k[on][order], img[on][order]
    starts = np.searchsorted(ring_sorted, np.arange(kk + 1))
    for i in range(kk):
        v = np.sort(values[starts[i]:starts[i + 1]])
        n = v.size
        count[i] = n
        if n:
            lo[i], hi[i] = v[(n - 1) // 2], v[n // 2]
    return count, lo, hi


def profile_of(count, lo, hi):
    """flatten.ring_profile's dict from the three arrays."""
    lo, hi = np.asarray(lo, np.uint16), np.asarray(hi, np.uint16)
    return {'count': np.asarray(count, np.uint32), 'lo': lo, 'hi': hi, 'median': (lo.astype(np.float64) + hi.astype(np.float64)) / 2.0,
            'radius': np.arange(lo.shape[0], dtype=np.float64) + 0.5}


def ring_flatten(img, circle, gain):
    """out uint16 [h, w]: off the disk the pixel; on it clip(rint((double)v g), 0, 65535), g the gain table read at u = sqrt(d2) - 0.5:
    gain[0] for u <= 0, gain[K - 1] for u >= K - 1, else gain[j] + (gain[j + 1] - gain[j]) (u - j), j = trunc(u)."""
    img = np.asarray(img, dtype=np.uint16)
    gain = np.asarray(gain, dtype=np.float64)
    kk = n_rings(circle)
    assert gain.shape == (kk,)
    on, _, d2 = rings(*img.shape, circle)
    u = np.sqrt(d2) - np.float64(0.5)
    top = np.float64(kk - 1)
    j = np.clip(np.trunc(u), 0, max(kk - 2, 0)).astype(np.int64)
    t = u - j.astype(np.float64)
    g0, g1 = gain[j], gain[np.minimum(j + 1, kk - 1)]
    with np.errstate(over='ignore', invalid='ignore'):
        g = g0 + (g1 - g0) * t
        g = np.where(u <= 0.0, gain[0], np.where(u >= top, gain[kk - 1], g))
        q = np.clip(np.rint(img.astype(np.float64) * g), 0.0, 65535.0)
    return np.where(on, q, img).astype(np.uint16)


def gain_from_profile(profile, smooth=1, level=None, max_gain=8.0):
    """flatten.gain_from_profile restated with Python loops: the fill, the running mean (the window summed in index order, one
    addition at a time, then one division), the level, the gain."""
    count = [int(v) for v in profile['count']]
    p = [np.float64(v) for v in profile['median']]
    kk = len(p)
    have = [i for i in range(kk) if count[i] > 0]
    if not have:
        raise ValueError('no ring holds a pixel')
    filled = []
    for i in range(kk):
        if count[i] > 0:
            filled.append(p[i])
            continue
        best = min(have, key=lambda q: (abs(q - i), q))
        filled.append(p[best])
    if smooth > 1:
        half = smooth // 2
        smoothed = []
        for i in range(kk):
            acc = filled[min(max(i - half, 0), kk - 1)]
            for d in range(-half + 1, half + 1):
                acc = acc + filled[min(max(i + d, 0), kk - 1)]
            smoothed.append(acc / np.float64(smooth))
        filled = smoothed
    if level is None:
        level = np.median(np.array(filled[:max(1, kk // 10)], dtype=np.float64))
    level = np.float64(level)
    out = np.zeros(kk, dtype=np.float64)
    for i in range(kk):
        if filled[i] != 0.0:
            out[i] = min(level / filled[i], np.float64(max_gain))
    return out


def flatten_disk(img, circle, smooth=1, level=None, max_gain=8.0):
    """(flat, profile, gain) as flatten.flatten_disk's."""
    profile = profile_of(*ring_medians(img, circle))
    gain = gain_from_profile(profile, smooth, level, max_gain)
    return ring_flatten(img, circle, gain), profile, gain


# ---- the accuracy: a synthetic disk of the scenes' law ----
def law(x):
    """The synthetic scenes' centre-to-limb law at r / R = x (tests/linemaps_ref.disk_scan)."""
    return 0.35 + 0.65 * np.sqrt(np.clip(1.0 - x * x, 0.0, 1.0))


SCENE = {'h': 260, 'w': 250, 'circle': (124.3, 128.6, 120.4), 'scale': 0.6, 'sky': 0.01}     # 121 rings


def synthetic_disk(noise, seed=0):
    """(img uint16 [260, 250], circle): 0.6 law(rho / R) on the disk with a spot (a Gaussian dip of 40 % at a third of the radius,
    5 px wide), 0.01 off it, additive Gaussian noise on the relative scale, times 65535 and rounded."""
    h, w, circle = SCENE['h'], SCENE['w'], SCENE['circle']
    cx, cy, rad = circle
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    rho = np.sqrt((c - cx) ** 2 + (r - cy) ** 2)
    img = np.where(rho <= rad, SCENE['scale'] * law(rho / rad), SCENE['sky'])
    img = img * (1.0 - 0.4 * np.exp(-0.5 * (((c - (cx + rad / 3.0)) / 5.0) ** 2 + ((r - (cy - rad / 5.0)) / 5.0) ** 2)))
    img = img + noise * np.random.default_rng(seed).standard_normal((h, w))
    return np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16), circle


INNER, OUTER = 4, 2           # rings reported apart: the innermost four (4 to 22 pixels each), the last two (a partial annulus on the
#                               steepest part of the law); 6 of K at the most


def profile_error(profile, rad, scale=None):
    """The recovered profile against the law: |median / (65535 scale) - law((k + 1/2) / R)| / law, relative -> (the worst over rings
    INNER .. K - OUTER - 1, over the inner rings, over the outer ones).  scale None (a scene whose continuum level is not known): the
    mean of median / law over the core rings takes the place of 65535 scale."""
    want = law(profile['radius'] / rad)
    kk = want.shape[0]
    assert INNER + OUTER <= 6 and kk > 6
    unit = 65535.0 * scale if scale is not None else (profile['median'][INNER:kk - OUTER] / want[INNER:kk - OUTER]).mean()
    err = np.abs(profile['median'] / unit - want) / want
    return float(err[INNER:kk - OUTER].max()), float(err[:INNER].max()), float(err[kk - OUTER:].max())


def flatness(flat_profile):
    """The flatness of a flat image's ring medians: max |median / mean of the core rings' medians - 1| -> (over the core rings
    INNER .. K - OUTER - 1, over the inner rings, over the outer ones)."""
    med = flat_profile['median']
    kk = med.shape[0]
    core = med[INNER:kk - OUTER]
    dev = np.abs(med / core.mean() - 1.0)
    return float(dev[INNER:kk - OUTER].max()), float(dev[:INNER].max()), float(dev[kk - OUTER:].max())


# What the restatement achieves on synthetic_disk(noise, seed=0), smooth = 1, default level and max_gain (tests/test_flatten_cpu.py
# re-measures and prints them), as (core rings INNER .. K - OUTER - 1, the inner four, the outer two).  Each bound is the measured value
# plus a quarter, rounded up to two significant digits: the quarter covers other seeds of the same scene.
#   noise 0:     profile 0.000832 / 0.000030 / 0.104390; flatness 0.002629 / 0.000221 / 0.029053
#   noise 0.004: profile 0.002307 / 0.002371 / 0.106352; flatness 0.003527 / 0.000843 / 0.031761
# (the last ring, a partial annulus on the steepest part of the law, reads 10 % off the law at its mid-radius and stays 3 % low in the
# flat image; smooth = 5 has a core flatness of 0.0161 / 0.0162: the running mean smears the limb.)
# 'pipeline': the same measures (profile with scale None) on the image and circle oracle/pipeline_oracle.py makes of
# linemaps_ref.disk_scan(gaussian(0), 400, 300, 48, noise 0.004, seed 3) at shift 0 -- K = 177, the fitted circle a few pixels off the
# scene's limb and the disk cut by the slit's lit rows, hence looser:
#   profile 0.030828 / 0.026782 / 0.493567; flatness 0.006374 / 0.000198 / 0.081255
TOLERANCE = {'profile': {0.0: (0.0011, 0.000039, 0.14), 0.004: (0.0029, 0.0030, 0.14)},
             'flatness': {0.0: (0.0033, 0.00028, 0.037), 0.004: (0.0045, 0.0011, 0.040)},
             'pipeline': {'profile': (0.039, 0.034, 0.62), 'flatness': (0.0080, 0.00025, 0.11)}}


def pipeline_scan():
    """The scan of the 'pipeline' entries: disk_scan's scene with the unshifted Gaussian line (file layout, uint16)."""
    from tests import linemaps_ref as ref
    from tests.linemaps_util import IH, IW, N
    return ref.disk_scan(ref.gaussian(np.zeros((IH, N))), IH, N, IW, noise=0.004, seed=3)[0]
