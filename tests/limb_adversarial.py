"""Hard flood scenes for the limb stage's canny and labelling kernels (csrc/limb.hip, csrc/limb_fused.hip), and the
SciPy reference they are held against (oracle/limb_oracle.canny_masks, scipy.ndimage.label).  CPU only: NumPy + SciPy.

A scene is a boolean image of "flooded" pixels: canny's input is where(flooded, 65000, 0).  The disks the other limb tests use
are one smooth closed contour; the scenes below hold what a disk lacks: exact ties in the suppression's `<=`, pixels on the
axis-aligned and 45-degree sector boundaries (several sectors apply, the later one overwrites the earlier), edges on the
16 x 64 tile borders of the fused kernels, blobs on the image border, thousands of small components, long contours that cross
every tile border, components that meet only far from where they cross a tile border, and images smaller than one tile or
than the Gaussian's radius."""
import functools
import math

import numpy as np
import scipy.ndimage as ndi

from oracle import limb_oracle

TH, TW = 16, 64                                    # the fused kernels' tile (csrc/limb_fused.hip)
# (sh, sw > 2 is what the entry points take); one tile exactly, one short, one over; two tiles a side; the 400-row minimum of
# a scan (100 block means), narrower than a tile; 8 x 4 tiles with ragged last ones
SHAPES = [(3, 3), (3, 70), (70, 3), (16, 64), (15, 63), (17, 65), (32, 128), (33, 129), (100, 40), (120, 200)]
SIGMAS = (2.0, 1.5, 1.0, 0.5)                      # every rung of get_edge_list's retry ladder
KS = (1, 3, 16)                                    # blur windows: the smallest, an odd one, the fused path's largest
K_SCENES = ('checker', 'corner', 'ones')           # the scenes that run with every k (the others: k = 1)
SEED = 7


def scenes(sh, sw, seed=SEED):
    """-> {name: bool [sh, sw]}, in a fixed order."""
    rng = np.random.default_rng([seed, sh, sw])
    yy, xx = np.mgrid[0:sh, 0:sw]
    out = {}
    rect = np.zeros((sh, sw), bool)
    rect[sh // 4:sh // 4 + sh // 2, sw // 4:sw // 4 + sw // 2] = True
    out['rect'] = rect
    corner = np.zeros((sh, sw), bool)
    corner[:sh // 2, :sw // 2] = True               # touches two image borders and one corner
    out['corner'] = corner
    lines = np.zeros((sh, sw), bool)
    lines[TH - 1:TH + 1, :] = True                  # (slices clamp to the image)
    lines[:, TW - 1:TW + 1] = True
    out['tile_lines'] = lines
    out['diamond'] = np.abs(yy - sh // 2) + np.abs(xx - sw // 2) <= min(sh, sw) // 3
    out['checker'] = (yy // 3 + xx // 3) % 2 == 1
    out['squares'] = ((yy // 3) % 2 == 0) & ((xx // 3) % 2 == 0)   # 3 x 3 squares 3 px apart: they do not touch
    out['dots'] = rng.random((sh, sw)) < 0.03
    out['blobs'] = ndi.uniform_filter(rng.random((sh, sw)), 7, mode='reflect') > 0.5
    out['ones'] = np.ones((sh, sw), bool)
    out['zeros'] = np.zeros((sh, sw), bool)
    out['spiral'] = _spiral(sh, sw)
    if sh >= 20:
        comb = np.zeros((sh, sw), bool)
        for x in range(1, sw - 1, 9):               # teeth 3 px wide, 6 px apart, rows 1 .. sh - 3
            comb[1:sh - 2, x:min(x + 3, sw - 1)] = True
        comb[sh - 3, 1:sw - 1] = True               # joined along their bottom row only
        out['comb'] = comb
    return out


def _spiral(sh, sw):
    """A 5-pixel-wide Archimedean band (radius = a * angle) from the centre out to 3 px from the image's sides, with arms
    18 px apart on the short side, closed by one more turn at full size.  The radius is measured in the 16-norm of the image's
    own aspect: turns shaped like the image, which reach into its corner tiles."""
    turns = max(1.0, min(sh, sw) / 36.0)
    t = np.linspace(0.0, 2 * np.pi * (turns + 1), 40 * (sh + sw))
    s = np.minimum(t / (2 * np.pi * turns), 1.0)
    d = (np.abs(np.cos(t)) ** 16 + np.abs(np.sin(t)) ** 16) ** (1 / 16)
    y = np.rint((sh - 1) / 2 + ((sh - 1) / 2 - 3) * s * np.sin(t) / d).astype(int)
    x = np.rint((sw - 1) / 2 + ((sw - 1) / 2 - 3) * s * np.cos(t) / d).astype(int)
    line = np.zeros((sh, sw), bool)
    line[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)] = True
    return ndi.binary_dilation(line, np.ones((5, 5), bool))


def as_inputs(scene, k):
    """-> (keys int32 [sh, sw]: the k x k window sums shg_limb_edges takes; blurred float64: the image shg_canny_masks_f64
    takes; flood_thresh).  Flooded pixels hold K1 = k*k * 2^19, the others K0 = k*k * 2^17; blurred is the product the
    kernels form from a window sum; flood_thresh is the flooded pixels' blurred value itself, so that the kernels'
    `blurred < flood_thresh` is decided at equality (nothing flooded: the next float64 above every value)."""
    K0, K1 = k * k * 2 ** 17, k * k * 2 ** 19
    keys = np.where(scene, K1, K0).astype(np.int64)
    assert keys.max() < 2 ** 31
    keys = keys.astype(np.int32)
    blurred = (keys * 2.0 ** -20) * (1.0 / (k * k))
    if scene.any():
        flood_thresh = float((K1 * 2.0 ** -20) * (1.0 / (k * k)))
    else:
        flood_thresh = float(np.nextafter(blurred.max(), np.inf))
    assert np.array_equal(blurred < flood_thresh, ~scene)
    return keys, blurred, flood_thresh


def flooded(scene):
    """get_flood_image's result for the scene (ellipse_to_circle.py:226-227): canny's input."""
    return np.where(scene, 65000.0, 0.0)


NO_MAXIMA = (1.0, 1.5)                             # thresholds()' third pair where the reference has no local maximum


def thresholds(reference_magnitude, local_maxima):
    """Three (low, high) pairs: both zero; production-like; and two magnitudes of the reference's own local maxima (the
    elements at one third and two thirds of the sorted list), so that the kernels' `>=` is decided at equality."""
    v = np.sort(reference_magnitude[local_maxima])
    own = (float(v[len(v) // 3]), float(v[2 * len(v) // 3])) if len(v) else NO_MAXIMA
    return [(0.0, 0.0), (0.0014, 0.0021), own]


def _hypot_glibc(x, y):
    """glibc 2.35's hypot (sysdeps/ieee754/dbl-64/e_hypot.c, the kernel without FMA) for finite inputs in the normal range,
    in Python floats: what both limb chains evaluate (csrc/limb_math.h: hypot_glibc)."""
    x, y = abs(x), abs(y)
    ax, ay = (y, x) if x < y else (x, y)
    if ax >= ay / 2.0 ** -54:
        return ax + ay
    h = math.sqrt(ax * ax + ay * ay)
    if h <= 2.0 * ay:
        delta = h - ay
        t1 = ax * (2.0 * delta - ax)
        t2 = (delta - 2.0 * (ax - ay)) * delta
    else:
        delta = h - ax
        t1 = 2.0 * delta * (ax - 2.0 * ay)
        t2 = (4.0 * delta - ay) * ay + delta * delta
    return h - (t1 + t2) / (2.0 * h)


hypot_glibc = np.vectorize(_hypot_glibc, otypes=[np.float64])


def gradients(image, sigma):
    """canny's (isobel, jsobel) for a float image, with the very SciPy calls of limb_oracle.canny_masks."""
    def fsmooth(x):
        return ndi.gaussian_filter(x, sigma, mode='constant', cval=0, truncate=4.0)
    smoothed = fsmooth(np.array(image, dtype=float)) / (fsmooth(np.ones(image.shape)) + np.finfo(float).eps)
    return ndi.sobel(smoothed, axis=0), ndi.sobel(smoothed, axis=1)


@functools.lru_cache(maxsize=None)
def gradient_pairs():
    """Every distinct (isobel, jsobel) of every scene, shape and sigma -> float64 [n, 2] (read-only)."""
    pairs = []
    for shape in SHAPES:
        for scene in scenes(*shape).values():
            for sigma in SIGMAS:
                isobel, jsobel = gradients(flooded(scene), sigma)
                pairs.append(np.unique(np.stack([isobel.ravel(), jsobel.ravel()], axis=1), axis=0))
    return _frozen(np.unique(np.concatenate(pairs), axis=0))


def suppression_census(image, sigma):
    """How hard the scene is for the non-maximum suppression, from the reference alone -> (ties, multi): the number of
    exact ties (an interpolated neighbour magnitude equal to the pixel's own: `<=` decided at equality) over the four
    sectors, and the number of interior pixels that more than one sector handles (the later sector overwrites)."""
    isobel, jsobel = gradients(image, sigma)
    mg = np.hypot(isobel, jsobel)
    ai, aj = np.abs(isobel), np.abs(jsobel)
    interior = np.zeros(image.shape, bool)
    interior[1:-1, 1:-1] = True
    eroded = interior & (mg > 0)
    same = ((isobel >= 0) & (jsobel >= 0)) | ((isobel <= 0) & (jsobel <= 0))
    opp = ((isobel <= 0) & (jsobel >= 0)) | ((isobel >= 0) & (jsobel <= 0))
    # (sector, weight numerator, denominator, the four neighbour offsets of skimage's plus1, plus2, minus1, minus2)
    sectors = [(same & (ai >= aj), aj, ai, (1, 0), (1, 1), (-1, 0), (-1, -1)),
               (same & (ai <= aj), ai, aj, (0, 1), (1, 1), (0, -1), (-1, -1)),
               (opp & (ai <= aj), ai, aj, (0, 1), (-1, 1), (0, -1), (1, -1)),
               (opp & (ai >= aj), aj, ai, (-1, 0), (-1, 1), (1, 0), (1, -1))]
    ties, handled = 0, np.zeros(image.shape, int)
    for pts, num, den, p1, p2, m1, m2 in sectors:
        pts = eroded & pts
        handled += pts
        ys, xs = np.nonzero(pts)
        m = mg[ys, xs]
        w = num[ys, xs] / den[ys, xs]
        at = lambda d: mg[ys + d[0], xs + d[1]]
        c_plus = at(p2) * w + at(p1) * (1 - w)
        c_minus = at(m2) * w + at(m1) * (1 - w)
        ties += int(np.count_nonzero((c_plus == m) | (c_minus == m)))
    return ties, int(np.count_nonzero(handled > 1))


def tiles_covered(component):
    """Number of 16 x 64 tiles a boolean image has a pixel in."""
    ys, xs = np.nonzero(component)
    return len(set(zip((ys // TH).tolist(), (xs // TW).tolist())))


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(sh, sw):
    """Every (scene, sigma, threshold pair) of one shape with the reference's answer, computed once and shared: a list of dicts
    name, scene, sigma, low, high, low_mask, high_mask, edges (canny's result), labels and low_labels (scipy.ndimage.label
    of edges and of low_mask, 8-connected)."""
    cases = []
    for name, scene in scenes(sh, sw).items():
        image = flooded(scene)
        _frozen(scene)
        for sigma in SIGMAS:
            _, _, mag, lm = limb_oracle.canny_masks(image, sigma, 0.0, 0.0)
            for low, high in thresholds(mag, lm):
                low_mask, high_mask, _, _ = limb_oracle.canny_masks(image, sigma, low, high)
                edges = limb_oracle.canny(image, sigma, low, high)
                labels, _ = ndi.label(edges, np.ones((3, 3), bool))
                low_labels, _ = ndi.label(low_mask, np.ones((3, 3), bool))
                cases.append(dict(name=name, scene=scene, sigma=sigma, low=low, high=high, low_mask=_frozen(low_mask),
                                  high_mask=_frozen(high_mask), edges=_frozen(edges), labels=_frozen(labels),
                                  low_labels=_frozen(low_labels)))
    return cases
