"""Conditions on the reference alone: the scenes of tests/limb_adversarial.py must stress what they are meant to stress, or
tests/test_limb_adversarial_gpu.py holds the canny and labelling kernels to less than it says.  No GPU."""
import numpy as np
import pytest
import scipy.ndimage as ndi

from oracle import limb_oracle
from tests import limb_adversarial as adv

EIGHT = np.ones((3, 3), bool)


@pytest.mark.parametrize('shape', adv.SHAPES, ids=lambda s: '%dx%d' % s)
def test_canny_is_its_masks_plus_hysteresis(shape):
    """limb_oracle.canny == hysteresis(canny_masks), on every scene, sigma and threshold pair the GPU test uses."""
    cases = adv.reference(*shape)
    names = {c['name'] for c in cases}
    assert names >= {'rect', 'corner', 'tile_lines', 'diamond', 'checker', 'dots', 'blobs', 'ones', 'zeros', 'spiral'}
    assert ('comb' in names) == (shape[0] >= 20)
    assert len(cases) == len(names) * len(adv.SIGMAS) * 3
    for c in cases:
        np.testing.assert_array_equal(limb_oracle.hysteresis(c['low_mask'], c['high_mask']), c['edges'], err_msg=c['name'])
        assert c['low_mask'].dtype == bool and not (c['high_mask'] & ~c['low_mask']).any()


def test_scenes_hold_suppression_ties_and_sector_boundaries():
    """At 33 x 129: exact ties in the suppression's `<=` and pixels more than one sector handles, which a flooded disk has
    next to none of."""
    shape = (33, 129)
    total = {}
    for sigma in (2.0, 0.5):
        ties_sum = multi_sum = 0
        for name, scene in adv.scenes(*shape).items():
            ties, multi = adv.suppression_census(adv.flooded(scene), sigma)
            print('CENSUS %dx%d sigma %.1f %-10s ties %5d  multi-sector %5d' % (shape + (sigma, name, ties, multi)))
            total[name, sigma] = ties
            ties_sum += ties
            multi_sum += multi
        print('CENSUS %dx%d sigma %.1f %-10s ties %5d  multi-sector %5d' % (shape + (sigma, 'all', ties_sum, multi_sum)))
        if sigma == 2.0:
            assert ties_sum >= 1000 and multi_sum >= 1000
    for name in ('rect', 'corner', 'tile_lines', 'checker', 'ones'):
        assert total[name, 2.0] > 0, name


def test_reference_thresholds_sit_on_a_local_maximum():
    """The third threshold pair is two magnitudes of the reference's own local maxima: `>=` is decided at equality.  Every
    non-empty scene has local maxima to take them from, at every sigma, from 15 x 63 up (a 3-pixel-wide image has one
    column of interior pixels, which a thin scene may leave without a maximum: there the pair is NO_MAXIMA)."""
    for shape in adv.SHAPES:
        for name, scene in adv.scenes(*shape).items():
            for sigma in adv.SIGMAS:
                _, _, mag, lm = limb_oracle.canny_masks(adv.flooded(scene), sigma, 0.0, 0.0)
                pairs = adv.thresholds(mag, lm)
                assert pairs[:2] == [(0.0, 0.0), (0.0014, 0.0021)]
                low, high = pairs[2]
                if not lm.any():
                    assert not scene.any() or min(shape) == 3, (shape, name, sigma)
                    assert (low, high) == adv.NO_MAXIMA
                    continue
                assert low <= high
                assert np.count_nonzero(lm & (mag == low)) >= 1 and np.count_nonzero(lm & (mag == high)) >= 1


def test_labelling_scenes_have_many_components_and_long_ones():
    """At 120 x 200 (8 x 4 tiles, the last ones ragged).  Many small components: the checker's low mask falls into more than
    500 pieces by scipy.ndimage.label's default (4-connected) structure, but canny's and the kernels' connectivity is 8,
    under which its pieces touch at their corners (245 components); the squares (3 x 3, 3 px apart) are what gives the
    union-find more than 500 components in its own connectivity.  Long ones: a contour of the spiral in 30 of the 32 tiles."""
    by = {}
    for c in adv.reference(120, 200):
        if (c['low'], c['high']) == (0.0, 0.0):
            by[c['name'], c['sigma']] = c['low_mask']
    for name in ('checker', 'squares', 'dots', 'blobs', 'comb', 'spiral'):
        for sigma in adv.SIGMAS:
            lab, n8 = ndi.label(by[name, sigma], EIGHT)
            n4 = ndi.label(by[name, sigma])[1]
            sizes = np.bincount(lab.ravel())[1:]
            widest = max((adv.tiles_covered(lab == i + 1) for i in np.argsort(sizes)[-3:]), default=0)
            print('COMPONENTS 120x200 sigma %.1f %-8s 8-connected %5d  4-connected %5d  tiles of the widest %2d' % (sigma, name, n8, n4, widest))
            by[name, sigma, 'n'] = (n8, n4, widest)
    assert by['checker', 2.0, 'n'][1] > 500
    assert by['squares', 1.0, 'n'][0] > 500 and by['squares', 0.5, 'n'][0] > 500
    for sigma in adv.SIGMAS:
        assert by['spiral', sigma, 'n'][2] >= 30


def test_host_hypot_is_the_kernels_hypot():
    """np.hypot on this host == the glibc 2.35 algorithm the kernels evaluate (csrc/limb_math.h: hypot_glibc), on every
    gradient pair of every scene: a host whose libm differs shows up here, and not as a mask that differs on the GPU."""
    pairs = adv.gradient_pairs()
    print('HYPOT %d distinct gradient pairs' % len(pairs))
    assert len(pairs) > 100000
    got = np.hypot(pairs[:, 0], pairs[:, 1])
    want = adv.hypot_glibc(pairs[:, 0], pairs[:, 1])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(pairs[i, 0], pairs[i, 1], got[i], want[i]) for i in bad[:5]]


def test_as_inputs_decide_the_flood_at_equality():
    scene = adv.scenes(17, 65)['blobs']
    for k in adv.KS:
        keys, blurred, thresh = adv.as_inputs(scene, k)
        assert keys.dtype == np.int32 and blurred.dtype == np.float64 and keys.max() < 2 ** 31
        assert np.count_nonzero(blurred == thresh) == np.count_nonzero(scene) > 0
        np.testing.assert_array_equal(np.where(blurred < thresh, 0.0, 65000.0), adv.flooded(scene))
    keys, blurred, thresh = adv.as_inputs(adv.scenes(17, 65)['zeros'], 3)
    assert thresh == np.nextafter(blurred.max(), np.inf) and (blurred < thresh).all()
