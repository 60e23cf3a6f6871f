"""NumPy restatement of shg_limb_profile_u16 and shg_rl_deconvolve_xy_u16, written from the arithmetic include/shg_hip.h states, not
from the kernels: whole planes of float64, one operation a step, the sector by the fold and the thresholds with no arctangent; the
deconvolution is deconvolve_ref's with the row pass and the column pass given their own taps.  Also the synthetic limb the accuracy
is measured on (a limb-darkened disk sampled over each pixel's area, then blurred by Gaussian taps an axis), the measures and the
bounds (TOLERANCE)."""
import numpy as np

from tests import deconvolve_ref as dr
from tests.sharpen_ref import reflect_index


# ---- the arithmetic of the header: the tables ----
def thresholds(sectors):
    """tan((k + 1) pi / (4 n)), n = sectors / 8: the doubles ops.sector_thresholds hands the library (the same expression)."""
    n = sectors // 8
    return np.tan(np.arange(1, n, dtype=np.float64) * (np.pi / (4.0 * n)))


def sector_and_bin(h, w, circle, reach, sub, sectors, table):
    """(sector int64 [h, w], bin int64 [h, w], counts bool [h, w]) of every pixel; sector and bin are 0 where the pixel does not count."""
    cx, cy, rad = (np.float64(v) for v in circle)
    table = np.asarray(table, dtype=np.float64)
    n = sectors // 8
    assert table.size == n - 1
    dx = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :] - cx, (h, w))
    dy = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None] - cy, (h, w))
    d2 = dx * dx + dy * dy
    rho = np.sqrt(d2)
    bins = 2 * reach * sub
    v = (rho - (rad - np.float64(reach))) * np.float64(sub)
    counts = (v >= 0.0) & (v < np.float64(bins))
    b = np.where(counts, np.floor(v), 0.0).astype(np.int64)
    ax, ay = np.abs(dx), np.abs(dy)
    swap = ay > ax
    hi, lo = np.where(swap, ay, ax), np.where(swap, ax, ay)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = lo / hi
    i = np.zeros((h, w), np.int64)
    for t in table:
        i += (t <= q)
    o = swap.astype(np.int64)
    rev = swap.copy()
    left = dx < 0.0
    o = np.where(left, 3 - o, o)
    rev = np.where(left, ~rev, rev)
    up = dy < 0.0
    o = np.where(up, 7 - o, o)
    rev = np.where(up, ~rev, rev)
    s = o * n + np.where(rev, n - 1 - i, i)
    return np.where(counts, s, 0), b, counts


def limb_profile(img, circle, reach, sub, sectors, table=None):
    """(count uint32, sum uint64, sumsq uint64), each [sectors, 2 reach sub]."""
    img = np.asarray(img, dtype=np.uint16)
    h, w = img.shape
    s, b, counts = sector_and_bin(h, w, circle, reach, sub, sectors, thresholds(sectors) if table is None else table)
    bins = 2 * reach * sub
    at = (s * bins + b)[counts]
    v = img[counts].astype(np.uint64)
    count = np.bincount(at, minlength=sectors * bins).astype(np.uint32)
    total = np.zeros(sectors * bins, np.uint64)
    sumsq = np.zeros(sectors * bins, np.uint64)
    np.add.at(total, at, v)
    np.add.at(sumsq, at, v * v)
    return count.reshape(sectors, bins), total.reshape(sectors, bins), sumsq.reshape(sectors, bins)


# ---- the arithmetic of the header: a tap set an axis ----
def blur_xy(a, kx, ky):
    """B(a): the row pass with kx, the column pass with ky -- deconvolve_ref.blur with the taps apart."""
    assert a.dtype == np.float32 and kx.dtype == np.float32 and ky.dtype == np.float32
    h, w = a.shape
    rx, ry = kx.size // 2, ky.size // 2
    t = np.zeros((h, w), np.float32)
    for i in range(-rx, rx + 1):
        t = t + kx[rx + i] * a[:, reflect_index(np.arange(w) + i, w)]
    b = np.zeros((h, w), np.float32)
    for i in range(-ry, ry + 1):
        b = b + ky[ry + i] * t[reflect_index(np.arange(h) + i, h), :]
    assert t.dtype == np.float32 and b.dtype == np.float32
    return b


def deconvolve_xy(img, taps_x, taps_y, iterations):
    """(out uint16 [h, w], e_N float32 [h, w])."""
    img = np.asarray(img, dtype=np.uint16)
    (kx, _), (ky, _) = dr.check_taps(taps_x), dr.check_taps(taps_y)
    assert img.ndim == 2 and 1 <= iterations <= dr.MAX_ITERATIONS
    back_x, back_y = np.ascontiguousarray(kx[::-1]), np.ascontiguousarray(ky[::-1])
    d = img.astype(np.float32)
    e = d
    for _ in range(iterations):
        b = blur_xy(e, kx, ky)
        q = d / np.maximum(b, dr.MIN_BLUR)
        c = blur_xy(q, back_x, back_y)
        p = e * c
        e = np.where(p < dr.FLUSH, np.float32(0), np.minimum(p, dr.CLAMP))
        assert e.dtype == np.float32 and np.isfinite(e).all() and (e >= 0).all()
    return dr.finish(e), e


def transpose_bound(kx, ky):
    """How far, relative to the value, ONE iteration on the transposed image with the tap sets swapped may lie from the transposed
    result.  Transposing swaps the order of the two passes, and float32 sums are not associative.  With u = 2^-24: a pass of n
    non-negative terms is within n u of its exact value, so a blur is within g = (nx + ny + 2) u whichever pass comes first, and two
    orders are within 2 g of each other.  b differs by 2 g, q = d / b by 2 g + u, c = B~(q) by that plus 2 g (the blur is linear and
    its terms non-negative), p = e c by u more: 4 g + 3 u, first order in u; doubled for the terms of second order."""
    g = (kx.size + ky.size + 2) * 2.0 ** -24
    return 2.0 * (4.0 * g + 3.0 * 2.0 ** -24)


# ---- the accuracy: a limb-darkened disk, sampled over each pixel's area, blurred an axis ----
SHAPE = (260, 250)
CIRCLE = (124.3, 131.7, 100.4)
DARKENING = 0.6
DISK, SKY = 40000.0, 600.0
NOISE = 260.0
PLANTED = [(1.5, 1.5), (1.0, 2.0), (2.0, 0.8)]
SUPER = 8                                    # sub-samples a pixel and axis


def gaussian64(sigma, radius=None):
    radius = int(np.ceil(5.0 * sigma)) if radius is None else radius
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return k / k.sum()


def blur64_xy(a, kx, ky):
    """The separable blur of a float64 plane, kx along the rows' columns and ky down the columns, reflected."""
    h, w = a.shape
    rx, ry = kx.size // 2, ky.size // 2
    t = sum(kx[rx + i] * a[:, reflect_index(np.arange(w) + i, w)] for i in range(-rx, rx + 1))
    return sum(ky[ry + i] * t[reflect_index(np.arange(h) + i, h), :] for i in range(-ry, ry + 1))


_SHARP = {}


def sharp_disk(shape=SHAPE, circle=CIRCLE):
    """The disk before the blur, float64 counts: SKY + DISK (1 - u (1 - mu)) on the disk, the mean over each pixel's area of 8 x 8
    sub-samples.  Computed once a (shape, circle) and never changed."""
    key = (tuple(shape), tuple(circle))
    if key not in _SHARP:
        h, w = shape
        cx, cy, rad = circle
        off = (np.arange(SUPER, dtype=np.float64) + 0.5) / SUPER - 0.5
        x = (np.arange(w, dtype=np.float64)[:, None] + off[None, :]).reshape(-1)
        y = (np.arange(h, dtype=np.float64)[:, None] + off[None, :]).reshape(-1)
        r2 = ((x[None, :] - cx) ** 2 + (y[:, None] - cy) ** 2) / (rad * rad)
        mu = np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))
        fine = np.where(r2 <= 1.0, DISK * (1.0 - DARKENING * (1.0 - mu)), 0.0) + SKY
        img = fine.reshape(h, SUPER, w, SUPER).mean(axis=(1, 3))
        img.setflags(write=False)
        _SHARP[key] = img
    return _SHARP[key]


def limb_scene(sigma_x, sigma_y, noise=0.0, seed=0, shape=SHAPE, circle=CIRCLE, blob=None):
    """The uint16 image of sharp_disk blurred by (sigma_x, sigma_y), with `noise` counts of seeded Gaussian noise.  blob (theta,
    amplitude): a bright Gaussian blob of 4 px planted on the limb at that angle before the blur."""
    sharp = sharp_disk(shape, circle)
    if blob is not None:
        theta, amplitude = blob
        bx, by = circle[0] + circle[2] * np.cos(theta), circle[1] + circle[2] * np.sin(theta)
        r = np.arange(shape[0], dtype=np.float64)[:, None]
        c = np.arange(shape[1], dtype=np.float64)[None, :]
        sharp = sharp + amplitude * np.exp(-0.5 * ((c - bx) ** 2 + (r - by) ** 2) / 16.0)
    seen = blur64_xy(sharp, gaussian64(sigma_x), gaussian64(sigma_y))
    if noise:
        seen = seen + noise * np.random.default_rng(seed).standard_normal(shape)
    return np.clip(np.rint(seen), 0, 65535).astype(np.uint16)


def expected(sigma):
    """What a planted sigma measures as: the pixel's own area adds 1 / 12 px^2."""
    return float(np.sqrt(sigma * sigma + 1.0 / 12.0))


def estimate(img, circle=CIRCLE, reach=12, sub=4, sectors=32):
    """psf.estimate_psf on the restatement's tables."""
    from solex_ser_recon_en_amd import psf
    count, total, _ = limb_profile(img, circle, reach, sub, sectors)
    return psf.estimate_from_profiles(count, total, psf.bin_centres(reach, sub))


def recovery_errors():
    """{case: (|sigma_x error|, |sigma_y error|)} over the planted pairs, and (1.0, 2.0) with NOISE counts of noise."""
    got = {}
    for sx, sy, noise in [p + (0.0,) for p in PLANTED] + [(1.0, 2.0, NOISE)]:
        est = estimate(limb_scene(sx, sy, noise, seed=1))
        got[(sx, sy, noise)] = (abs(est['sigma_x'] - expected(sx)), abs(est['sigma_y'] - expected(sy)))
    return got


# ---- why it pays: deconvolve_ref's structured scene under an anisotropic blur ----
PAYS_PAIR = (1.0, 2.0)
PAYS_CLEAR = 20.0                            # the measure is taken inside rad - 20


def pays_scene():
    """(the uint16 image of deconvolve_ref's model blurred by PAYS_PAIR, the model in counts, its circle, the region bool)."""
    from tests import sharpen_ref as sr
    _, model, circle, _, _ = sr.scene()
    seen = blur64_xy(model, gaussian64(PAYS_PAIR[0]), gaussian64(PAYS_PAIR[1]))
    h, w = model.shape
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    region = np.hypot(c - circle[0], r - circle[1]) < circle[2] - PAYS_CLEAR
    return np.clip(np.rint(seen), 0, 65535).astype(np.uint16), model, tuple(float(v) for v in circle), region


# What the restatement achieves (tests/test_psf_cpu.py re-measures and prints them).
#   recovery: the largest error of either width against sqrt(sigma^2 + 1/12) over the four cases is 0.0160 px -- (1.5, 1.5): 0.0160,
#   0.0160; (1.0, 2.0): 0.0131, 0.0104; (2.0, 0.8): 0.0099, 0.0106; (1.0, 2.0) with 260 counts of noise: 0.0023, 0.0083 --, and the bound is
#   that plus 0.02 px; it has to stay below 0.1 px whatever is measured.
#   pays: 10 iterations with the estimated pair (1.010, 2.010) leave 1.228 counts rms inside rad - 20, 10 iterations with the default
#   1.2 leave 29.941 (the blurred image: 52.838): a ratio of 0.04101; the bound is the ratio plus a quarter of its distance to 1.
TOLERANCE = {'recovery': 0.036, 'pays': 0.281}
