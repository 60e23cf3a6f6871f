"""NumPy restatement of shg_rl_deconvolve_u16, written from the arithmetic include/shg_hip.h states, not from the kernel: whole
planes of float32, the reflection as index arrays, a tap at a time -- one rounded multiply and one rounded add of float32 arrays --
in increasing order from a plane of zeros, a row pass and then a column pass, the taps reversed for the adjoint.  Also the synthetic
scene the accuracy is measured on (flatten's disk with its spot, blurred by a Gaussian of sigma 1.5 in float64), the measures
themselves and the bounds (TOLERANCE)."""
import numpy as np

from tests import sharpen_ref as sr
from tests.sharpen_ref import reflect_index

MAX_RADIUS = 16
MAX_ITERATIONS = 200
MIN_TAP = np.float32(2.0 ** -30)
MIN_BLUR = np.float32(2.0 ** -10)
FLUSH = np.float32(2.0 ** -20)
CLAMP = np.float32(2.0 ** 20)


# ---- the arithmetic of the header ----
def check_taps(taps):
    """The taps as float32 [2 R + 1] and R; the header's ranges asserted."""
    k = np.asarray(taps, dtype=np.float32).reshape(-1)
    assert k.size % 2 == 1 and k.size // 2 <= MAX_RADIUS
    assert np.isfinite(k).all() and ((k == 0) | ((k >= MIN_TAP) & (k <= 1))).all()
    assert abs(float(k.astype(np.float64).sum()) - 1.0) <= 2.0 ** -10
    return k, k.size // 2


def blur(a, k):
    """B(a, k): a float32 [h, w], k float32 [2 R + 1] standing for k[-R .. R]."""
    assert a.dtype == np.float32 and k.dtype == np.float32
    h, w = a.shape
    radius = k.size // 2
    t = np.zeros((h, w), np.float32)
    for i in range(-radius, radius + 1):
        t = t + k[radius + i] * a[:, reflect_index(np.arange(w) + i, w)]
    b = np.zeros((h, w), np.float32)
    for i in range(-radius, radius + 1):
        b = b + k[radius + i] * t[reflect_index(np.arange(h) + i, h), :]
    assert t.dtype == np.float32 and b.dtype == np.float32
    return b


def iterate(img, taps, iterations, reverse=True):
    """e_N, float32 [h, w].  reverse False: step 3 with the taps as they are -- the mistake the adjoint test tells apart."""
    img = np.asarray(img, dtype=np.uint16)
    k, _ = check_taps(taps)
    assert img.ndim == 2 and 1 <= iterations <= MAX_ITERATIONS
    back = np.ascontiguousarray(k[::-1]) if reverse else k
    d = img.astype(np.float32)
    e = d
    for _ in range(iterations):
        b = blur(e, k)
        q = d / np.maximum(b, MIN_BLUR)
        c = blur(q, back)
        p = e * c
        e = np.where(p < FLUSH, np.float32(0), np.minimum(p, CLAMP))
        assert e.dtype == np.float32 and np.isfinite(e).all() and (e >= 0).all()
    return e


def finish(e):
    return np.clip(np.rint(e), 0, 65535).astype(np.uint16)                     # (np.rint: ties to even)


def deconvolve(img, taps, iterations):
    """(out uint16 [h, w], e_N float32 [h, w])."""
    e = iterate(img, taps, iterations)
    return finish(e), e


def pad_taps(taps, radius):
    """The taps with zeros on both sides, to `radius`."""
    k, r = check_taps(taps)
    assert r <= radius <= MAX_RADIUS
    return np.concatenate([np.zeros(radius - r, np.float32), k, np.zeros(radius - r, np.float32)])


def gaussian(sigma, radius):
    """exp(-i^2 / (2 sigma^2)) in float64 over i = -radius .. radius, normalised to sum 1, as float32."""
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-(i * i) / (2.0 * float(sigma) * float(sigma)))
    return (k / k.sum()).astype(np.float32)


def zero_sky_disk(h, w):
    """A bright disk with a dark spot on a sky of exactly 0, and a faint rim of 2 counts just off the limb: beside the bright limb
    the rim's estimate shrinks by orders of magnitude an iteration, so the flush of step 5 is on the path."""
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    rho = np.hypot(c - 0.47 * w, r - 0.52 * h) / (0.36 * min(h, w))
    img = np.where(rho <= 1.0, 40000.0 * (0.35 + 0.65 * np.sqrt(np.clip(1.0 - rho * rho, 0.0, 1.0))), 0.0)
    img *= 1.0 - 0.5 * np.exp(-0.5 * ((c - 0.55 * w) ** 2 + (r - 0.4 * h) ** 2) / 9.0)
    img = np.where((rho > 1.0) & (rho <= 1.05), 2.0, img)
    return np.rint(img).astype(np.uint16)


# ---- the accuracy: flatten's synthetic disk, blurred ----
BLUR_SIGMA = 1.5
BLUR_RADIUS = 6
SPOT_REGION = 12.0                           # the measures are taken within 12 px of the spot's centre
NOISE = sr.NOISE                             # section 18's: 262.14 counts


def blur64(a, k):
    """The separable blur of a float64 plane by float64 taps, reflected: the scene's instrument."""
    h, w = a.shape
    radius = k.size // 2
    t = sum(k[radius + i] * a[:, reflect_index(np.arange(w) + i, w)] for i in range(-radius, radius + 1))
    return sum(k[radius + i] * t[reflect_index(np.arange(h) + i, h), :] for i in range(-radius, radius + 1))


def scene(noise=0.0, seed=0):
    """(the blurred image uint16 [260, 250], the model before the blur in counts float64, the region bool: within 12 px of the spot)."""
    _, model, circle, _, _ = sr.scene()
    cx, cy, rad = circle
    h, w = model.shape
    i = np.arange(-BLUR_RADIUS, BLUR_RADIUS + 1, dtype=np.float64)
    k = np.exp(-(i * i) / (2.0 * BLUR_SIGMA * BLUR_SIGMA))
    seen = blur64(model, k / k.sum())
    if noise:
        seen = seen + noise * 65535.0 * np.random.default_rng(seed).standard_normal((h, w))
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    region = np.hypot(c - (cx + rad / 3.0), r - (cy - rad / 5.0)) <= SPOT_REGION
    return np.clip(np.rint(seen), 0, 65535).astype(np.uint16), model, region


def rms(a, model, region):
    return float(np.sqrt((((np.asarray(a, dtype=np.float64) - model)[region]) ** 2).mean()))


def scene_measures(deconvolve_of):
    """deconvolve_of(img, taps, iterations) -> the deconvolved uint16 image -> {'clean': the rms error within 12 px of the spot after
    10 iterations on the noise-free scene, as a fraction of the blurred image's; 'flux': |sum out / sum img - 1| there; 'noisy': the
    same fraction after 5 iterations with section 18's noise; and the four rms errors themselves, in counts}."""
    taps = gaussian(BLUR_SIGMA, BLUR_RADIUS)
    img, model, region = scene()
    out = np.asarray(deconvolve_of(img, taps, 10))
    noisy_img, _, _ = scene(NOISE)
    noisy_out = np.asarray(deconvolve_of(noisy_img, taps, 5))
    got = {'blurred_rms': rms(img, model, region), 'clean_rms': rms(out, model, region), 'noisy_blurred_rms': rms(noisy_img, model, region),
           'noisy_rms': rms(noisy_out, model, region), 'flux': abs(float(out.astype(np.float64).sum() / img.astype(np.float64).sum()) - 1.0)}
    got['clean'] = got['clean_rms'] / got['blurred_rms']
    got['noisy'] = got['noisy_rms'] / got['noisy_blurred_rms']
    return got


# What the restatement achieves on scene() (tests/test_deconvolve_cpu.py re-measures and prints them).  Each bound is the measured
# value plus a quarter, rounded up to two significant digits; the quarter covers other seeds of the same scene.
#   clean: 1.830 counts rms within 12 px of the spot after 10 iterations for 361.816 in the blurred image, 0.005057 of it;
#   flux: the sum of the output is off the input's by 6.349e-06 of it;
#   noisy: 305.92 counts after 5 iterations for 439.18 in the blurred image with noise of 262.14 counts, 0.696576 of it
TOLERANCE = {'clean': 0.0064, 'flux': 8.0e-06, 'noisy': 0.88}
