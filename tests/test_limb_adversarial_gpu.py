"""The limb stage's canny and labelling kernels -- the one-kernel-per-call chain (csrc/limb.hip: shg_canny_masks_f64,
shg_edge_components) and the tiled one (csrc/limb_fused.hip: shg_limb_edges) -- against SciPy (oracle/limb_oracle, pinned to
scikit-image 0.18.3 by tests/test_oracle_golden.py, and scipy.ndimage.label) on the hard scenes of tests/limb_adversarial.py.
Every quantity is a mask or an integer: no pixel is left out of a comparison and there is no tolerance.
Image sizes: the entry points take sh, sw > 2, so 3 x 3, 3 x 70 and 70 x 3 (narrower than every Gaussian radius) run."""
import time

import numpy as np
import pytest
import scipy.ndimage as ndi

from oracle import limb_oracle
from tests import limb_adversarial as adv
from tests.numpy_ref import labels_from_roots

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Findings:
    """Every comparison of a test is made; the test fails at its end with the first differing pixel of each."""

    def __init__(self):
        self.failed, self.made = [], 0

    def same(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        self.made += 1
        if got.shape != want.shape:
            self.failed.append('%s: %d elements, reference %d' % (what, got.size, want.size))
        elif not np.array_equal(got, want):
            bad = np.flatnonzero(got.ravel() != want.ravel())
            i = int(bad[0])
            self.failed.append('%s: %d of %d differ, first at %d: %r, reference %r' % (what, bad.size, got.size, i, got.ravel()[i], want.ravel()[i]))

    def close(self):
        assert not self.failed, '%d of %d comparisons failed:\n%s' % (len(self.failed), self.made, '\n'.join(self.failed[:40]))


def smallest_index_roots(labels, idx):
    """The smallest linear index of each pixel's component, for the pixels idx (raster order) of a labelled image."""
    lab = labels.ravel()[idx]
    _, first = np.unique(lab, return_index=True)                  # idx ascends: the first occurrence is the smallest index
    return idx[first][np.searchsorted(np.unique(lab), lab)] if len(idx) else idx


def check_separate(ops, f, tag, c, blurred_d, flood_thresh):
    low_m, high_m = ops.canny_masks(blurred_d, flood_thresh, c['sigma'], c['low'], c['high'])
    f.same(tag + ' separate low mask', low_m.cpu().numpy().astype(bool), c['low_mask'])
    f.same(tag + ' separate high mask', high_m.cpu().numpy().astype(bool), c['high_mask'])
    idx, root = ops.edge_components(low_m, high_m)
    want_idx = np.flatnonzero(c['edges']).astype(np.int32)
    f.same(tag + ' separate edge pixels', idx, want_idx)
    if np.array_equal(idx, want_idx):
        lab, n = labels_from_roots(root)
        f.same(tag + ' separate component count', n, c['labels'].max())
        f.same(tag + ' separate labels', lab, c['labels'].ravel()[idx])
        f.same(tag + ' separate roots', root, smallest_index_roots(c['labels'], idx))


def check_fused(ops, f, tag, c, keys_d, k, flood_thresh):
    idx, root, strong = ops.limb_edges(keys_d, k, flood_thresh, c['sigma'], c['low'], c['high'])
    want_idx = np.flatnonzero(c['low_mask']).astype(np.int32)
    f.same(tag + ' fused low pixels', idx, want_idx)
    if not np.array_equal(idx, want_idx):
        return
    f.same(tag + ' fused strong', strong, c['high_mask'].ravel()[idx])
    f.same(tag + ' fused roots', root, smallest_index_roots(c['low_labels'], idx))       # every low pixel's, kept or not
    keep = np.isin(root, np.unique(root[strong]))                                     # the hysteresis the stage does on the host
    kept = idx[keep]
    f.same(tag + ' fused edge pixels', kept, np.flatnonzero(c['edges']))
    if np.array_equal(kept, np.flatnonzero(c['edges'])):
        lab, n = labels_from_roots(root[keep])
        f.same(tag + ' fused component count', n, c['labels'].max())
        f.same(tag + ' fused labels', lab, c['labels'].ravel()[kept])


def run_shape(ops, shape, separate):
    t0 = time.perf_counter()
    cases = adv.reference(*shape)
    t1 = time.perf_counter()
    f = Findings()
    inputs = {}
    for c in cases:
        for k in adv.KS if c['name'] in adv.K_SCENES else adv.KS[:1]:
            if (c['name'], k) not in inputs:
                keys, blurred, thresh = adv.as_inputs(c['scene'], k)
                inputs[c['name'], k] = dev(keys), dev(blurred), thresh
            keys_d, blurred_d, thresh = inputs[c['name'], k]
            tag = '%dx%d %s k=%d sigma=%g low=%r high=%r:' % (shape + (c['name'], k, c['sigma'], c['low'], c['high']))
            if separate:
                check_separate(ops, f, tag, c, blurred_d, thresh)
            check_fused(ops, f, tag, c, keys_d, k, thresh)
    print('LIMB ADVERSARIAL %dx%d: %d cases, %d comparisons, reference %.2f s, kernels and checks %.2f s'
          % (shape + (len(cases), f.made, t1 - t0, time.perf_counter() - t1)))
    f.close()


@pytest.mark.parametrize('shape', adv.SHAPES, ids=lambda s: '%dx%d' % s)
def test_canny_and_labelling_match_scipy_on_hard_scenes(ops, shape, monkeypatch):
    """Both paths, every scene, sigma 2 / 1.5 / 1 / 0.5, three threshold pairs (zero, production-like, two magnitudes of the
    reference's own maxima); blur windows 1 (all scenes) and 3, 16 (checker, corner, ones).  Separate: low and high mask ==
    the oracle's; edge pixels == limb_oracle.canny's in raster order; roots -> scipy.ndimage.label's numbering.  Fused: the low
    pixels, their high bits, every root the smallest index of its component, and after the host's hysteresis canny's pixels
    with scipy's labels."""
    monkeypatch.delenv('SHG_LIMB_FENCE', raising=False)
    run_shape(ops, shape, separate=True)


def test_fused_path_matches_scipy_with_the_fence(ops, monkeypatch):
    monkeypatch.setenv('SHG_LIMB_FENCE', '1')
    run_shape(ops, (33, 129), separate=False)


@pytest.mark.parametrize('fence', [None, '1'])
def test_flood_boundary_of_a_real_blurred_image(ops, fence, monkeypatch):
    """The window sums shg_limb_prepare forms of a noisy disk, flooded at a value the blurred image holds (its median
    element): `blurred < flood_thresh` at equality on real data, both paths against the oracle on the same flood."""
    from solex_ser_recon_en_amd import hostmath
    from tests.test_kernels_gpu import _limb_disk
    if fence is None:
        monkeypatch.delenv('SHG_LIMB_FENCE', raising=False)
    else:
        monkeypatch.setenv('SHG_LIMB_FENCE', fence)
    h, w = 420, 640
    sh, sw = 105, 160
    n, k = sh * sw, 1
    lo, hi, gamma = hostmath.percentile_plan(n, 99.0)
    packed, keys_d, ws = ops.limb_prepare(dev(_limb_disk(h, w, 5)), k, [n // 2 - 1, n // 2, lo, hi], gamma)
    torch.cuda.synchronize()
    keys = keys_d.cpu().numpy()
    assert keys.shape == (sh, sw) and keys.min() >= 0
    blurred = (keys * 2.0 ** -20) * (1.0 / (k * k))
    flood_thresh = float(np.sort(blurred.ravel())[n // 2])
    at = int(np.count_nonzero(blurred == flood_thresh))
    print('FLOOD BOUNDARY: %d pixels equal the threshold %r, %d below' % (at, flood_thresh, np.count_nonzero(blurred < flood_thresh)))
    assert at >= 1
    image = np.where(blurred < flood_thresh, 0.0, 65000.0)
    f = Findings()
    blurred_d = dev(blurred)
    for sigma in adv.SIGMAS:
        _, _, mag, lm = limb_oracle.canny_masks(image, sigma, 0.0, 0.0)
        for low, high in adv.thresholds(mag, lm):
            low_mask, high_mask, _, _ = limb_oracle.canny_masks(image, sigma, low, high)
            edges = limb_oracle.canny(image, sigma, low, high)
            c = dict(sigma=sigma, low=low, high=high, low_mask=low_mask, high_mask=high_mask, edges=edges,
                     labels=ndi.label(edges, np.ones((3, 3), bool))[0], low_labels=ndi.label(low_mask, np.ones((3, 3), bool))[0])
            tag = 'disk sigma=%g low=%r high=%r:' % (sigma, low, high)
            check_separate(ops, f, tag, c, blurred_d, flood_thresh)
            check_fused(ops, f, tag, c, keys_d, k, flood_thresh)
    assert f.made >= 12 * 5
    f.close()
