"""NumPy restatement of shg_limb_split_u16 and shg_limb_merge_u16, written from the arithmetic include/shg_hip.h states, not from the
kernels: whole planes of float64, one ufunc an IEEE operation, every pixel through the continuation and np.where for the choice.
Also limbguard.protect restated on top of them, the synthetic scene the gain is measured on (deconvolve's: flatten's disk with its
spot, blurred by a Gaussian of sigma 1.5), the measures themselves and the bounds (TOLERANCE)."""
import numpy as np

from tests import deconvolve_ref as dr
from tests import sharpen_ref as sr

MAX_DIM = 16384


# ---- the arithmetic of the header ----
def check_ring(circle, margin):
    """(cx, cy, rad, E, F) as float64; the header's limits asserted."""
    cx, cy, rad = (np.float64(v) for v in circle)
    margin = np.float64(margin)
    assert np.isfinite([cx, cy, rad, margin]).all() and 0.0 < rad < MAX_DIM and abs(cx) < 65536.0 and abs(cy) < 65536.0
    assert margin >= 0.0 and rad - margin >= 1.0
    return cx, cy, rad, rad - margin, rad + margin


def rays(h, w, circle):
    """(rho, ux, uy), float64 [h, w]."""
    cx, cy = np.float64(circle[0]), np.float64(circle[1])
    dx = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :] - cx, (h, w))
    dy = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None] - cy, (h, w))
    rho = np.sqrt(dx * dx + dy * dy)
    off = rho > 0.0
    safe = np.where(off, rho, 1.0)
    return rho, np.where(off, dx / safe, 1.0), np.where(off, dy / safe, 0.0)


def bilin(img, x, y):
    h, w = img.shape
    x, y = np.clip(x, 0.0, np.float64(w - 1)), np.clip(y, 0.0, np.float64(h - 1))
    x0, y0 = x.astype(np.int64), y.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = x - x0.astype(np.float64), y - y0.astype(np.float64)
    a, b, c, d = (img[yy, xx].astype(np.float64) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    top = a + (b - a) * fx
    bot = c + (d - c) * fx
    return top + (bot - top) * fy


def quantise(v):
    return np.clip(np.rint(v), 0, 65535).astype(np.uint16)                     # (np.rint: ties to even)


def split(img, circle, margin, reach):
    """(inner, outer), uint16 [h, w]."""
    img = np.asarray(img, dtype=np.uint16)
    assert img.ndim == 2 and 1 <= min(img.shape) and max(img.shape) <= MAX_DIM
    cx, cy, _, e, f = check_ring(circle, margin)
    reach = np.float64(reach)
    assert np.isfinite(reach) and 1.0 <= reach <= e
    rho, ux, uy = rays(img.shape[0], img.shape[1], circle)

    def sample(t):
        return bilin(img, cx + ux * t, cy + uy * t)

    s = sample(e)
    inner = np.where(rho > e, quantise((s + s) - sample(np.maximum((e + e) - rho, e - reach))), img)
    s = sample(f)
    outer = np.where(rho < f, quantise((s + s) - sample(np.minimum((f + f) - rho, f + reach))), img)
    return inner.astype(np.uint16), outer.astype(np.uint16)


def merge(img, disk, sky, circle, margin, blend):
    """out, uint16 [h, w]; sky None: the image stays beyond F."""
    img, disk = np.asarray(img, dtype=np.uint16), np.asarray(disk, dtype=np.uint16)
    assert img.ndim == 2 and disk.shape == img.shape and (sky is None or np.asarray(sky).shape == img.shape)
    _, _, _, e, f = check_ring(circle, margin)
    blend = np.float64(blend)
    assert np.isfinite(blend) and blend > 0.0
    rho = rays(img.shape[0], img.shape[1], circle)[0]
    o = img.astype(np.float64)
    wt = np.minimum((e - rho) / blend, 1.0)
    out = np.where(rho < e, quantise(o + wt * (disk.astype(np.float64) - o)), img)
    if sky is not None:
        wt = np.minimum((rho - f) / blend, 1.0)
        out = np.where(rho > f, quantise(o + wt * (np.asarray(sky, dtype=np.uint16).astype(np.float64) - o)), out)
    return out.astype(np.uint16)


def regions(shape, circle, margin, blend):
    """(band: E <= rho <= F; disk_full: wt = 1 inside; sky_full: wt = 1 outside), bool [h, w], by the header's own expressions."""
    _, _, _, e, f = check_ring(circle, margin)
    rho = rays(shape[0], shape[1], circle)[0]
    blend = np.float64(blend)
    return (rho >= e) & (rho <= f), (rho < e) & ((e - rho) / blend >= 1.0), (rho > f) & ((rho - f) / blend >= 1.0)


def protect(img, circle, process, margin, blend=4.0, reach=32.0, sky=True):
    """limbguard.protect: split, process(plane) once or twice, merge; reach clipped to E."""
    e = check_ring(circle, margin)[3]
    inner, outer = split(img, circle, margin, min(np.float64(reach), e))
    return merge(img, process(inner), process(outer) if sky else None, circle, margin, blend)


# ---- the gain: deconvolve's scene, measured beside the limb ----
MARGIN, BLEND, REACH, ITERATIONS, ANNULUS = 6.0, 4.0, 24.0, 30, 30.0
SHARPEN_GAINS, SHARPEN_DENOISE = (1.0, 1.8, 1.4, 1.0), (3.0, 1.0, 0.0, 0.0)


def annuli(shape, circle, region):
    """(the inner annulus [rad - 30, rad - margin - blend], the sky annulus [rad + margin + blend, rad + 30]), both outside the spot's
    region."""
    rad = np.float64(circle[2])
    rho = rays(shape[0], shape[1], circle)[0]
    return ((rho >= rad - ANNULUS) & (rho <= rad - MARGIN - BLEND) & ~region,
            (rho >= rad + MARGIN + BLEND) & (rho <= rad + ANNULUS) & ~region)


def sharpen_arguments(img, circle):
    """(gain_q8, threshold_q6) of the default sharpen on img: the noise measured once, inside 0.9 rad of the original image."""
    from solex_ser_recon_en_amd import sharpen
    median, _ = sr.noise(img, (circle[0], circle[1], circle[2] * sharpen.DEFAULT_REGION))
    return sharpen.quantise_gains(SHARPEN_GAINS), sharpen.thresholds(sharpen.sigma_from_median(median), SHARPEN_DENOISE, len(SHARPEN_GAINS))


def scene_measures(deconvolve_of, sharpen_of, split_merge=None):
    """deconvolve_of(img, taps, iterations, limb) and sharpen_of(img, circle, limb) -> the filtered uint16 image, limb None (plain) or
    {'circle', 'margin', 'blend', 'reach'} -> the rms errors against the model in counts and their ratios, protected over plain:
    'inner', 'sky' (noise-free, 30 iterations), 'noisy_inner', 'noisy_sky' (section 18's noise), 'sharpen' (the largest change of a
    sky-annulus pixel under the default sharpen, noise-free)."""
    circle = sr.scene()[2]
    taps = dr.gaussian(dr.BLUR_SIGMA, dr.BLUR_RADIUS)
    limb = {'circle': circle, 'margin': MARGIN, 'blend': BLEND, 'reach': REACH}
    got = {}
    for tag, noise in (('', 0.0), ('noisy_', dr.NOISE)):
        img, model, region = dr.scene(noise)
        inner, sky = annuli(img.shape, circle, region)
        plain = np.asarray(deconvolve_of(img, taps, ITERATIONS, None))
        guarded = np.asarray(deconvolve_of(img, taps, ITERATIONS, limb))
        for name, where in (('inner', inner), ('sky', sky)):
            got[tag + name + '_blurred_rms'] = dr.rms(img, model, where)
            got[tag + name + '_plain_rms'] = dr.rms(plain, model, where)
            got[tag + name + '_rms'] = dr.rms(guarded, model, where)
            got[tag + name] = got[tag + name + '_rms'] / got[tag + name + '_plain_rms']
    img, _, region = dr.scene()
    sky = annuli(img.shape, circle, region)[1]
    base = img.astype(np.int64)
    got['sharpen_plain_max'] = int(np.abs(np.asarray(sharpen_of(img, circle, None)).astype(np.int64) - base)[sky].max())
    got['sharpen_max'] = int(np.abs(np.asarray(sharpen_of(img, circle, dict(limb, margin=MARGIN))).astype(np.int64) - base)[sky].max())
    got['sharpen'] = got['sharpen_max'] / got['sharpen_plain_max']
    return got


def restated_measures():
    """scene_measures of the restatements composed: protect around deconvolve_ref / sharpen_ref."""
    def deconvolve_of(img, taps, iterations, limb):
        def run(plane):
            return dr.deconvolve(plane, taps, iterations)[0]
        return run(img) if limb is None else protect(img, limb['circle'], run, limb['margin'], limb['blend'], limb['reach'])

    def sharpen_of(img, circle, limb):
        gain_q8, thr = sharpen_arguments(img, circle)

        def run(plane):
            return sr.sharpen(plane, gain_q8, thr)[0]
        return run(img) if limb is None else protect(img, limb['circle'], run, limb['margin'], limb['blend'], limb['reach'])

    return scene_measures(deconvolve_of, sharpen_of)


# What the restatement achieves on the scene (tests/test_limbguard_cpu.py re-measures and prints them), margin 6, blend 4, reach 24,
# 30 iterations of sigma 1.5 / radius 6.  The bounds on the noise-free ratios are the measured value plus a quarter, rounded up to two
# significant digits; those with noise the measured value plus 0.01.  HARD is the condition on top: a ratio above it means the
# continuation was built wrong (plain mirroring, which leaves a cusp, gives about 1).
#   inner: 3.731 counts rms over the annulus [rad - 30, rad - 10] for 21.468 after plain Richardson-Lucy (19.410 in the blurred
#   image), 0.173779 of it; sky: 0.351 counts over [rad + 10, rad + 30] for 7.881 (0.350 in the blurred image), 0.044544 of it;
#   noisy_inner: 438.94 counts for 439.23 with noise of 262.14 counts, 0.999327 of it; noisy_sky: 429.62 for 430.58, 0.997765;
#   sharpen: the default gains move a pixel of the sky annulus by up to 225 counts, and by 0 when protected -- the sky plane is flat
#   there and its continuation, the point reflection of a constant, is the same constant: the bound is 0.
TOLERANCE = {'inner': 0.22, 'sky': 0.056, 'noisy_inner': 1.0094, 'noisy_sky': 1.0078, 'sharpen': 0.0}
HARD = {'inner': 0.5, 'sky': 0.5, 'sharpen': 0.1}
