"""The NumPy restatement of the finish (linemaps_ref.doppler_finish, linemaps_ref.line_profile_finish) held bit for bit to the
exact reference written from the header (tests/finish_exact.py) on the adversarial geometries of tests/finish_adversarial.py, every
decision class reached; and the number of pixels where the header's float64 circle test decides otherwise than the exact one."""
from collections import Counter

import numpy as np
import pytest

from tests import finish_adversarial as adv
from tests import finish_exact as ex
from tests import linemaps_ref as ref

# Pixels of the adversarial set (P = 1 and P = 5 alike: the mask does not depend on the planes) where the float64 compare
# (c - cx)^2 + (r - cy)^2 > rad^2 keeps a pixel whose exact distance exceeds the exact radius, or the other way round.  The header
# makes the float64 compare the rule; the count is what that rule costs on these circles, stated in DESIGN (section 11).
MASK_DISAGREEMENTS = 40


def run_exact(case):
    h00, h01, h02, out_h, out_w = case['geometry']
    return ex.finish(case['raw'], h00, h01, h02, out_h, out_w, case['circle'], case['crop'], case['display_range'],
                     case['half_width'])


def restatement(case, P):
    h00, h01, h02, out_h, out_w = case['geometry']
    if P == 1:
        m, png = ref.doppler_finish(case['raw'][0], h00, h01, h02, out_h, out_w, case['circle'], case['crop'],
                                    case['display_range'])
        return m[None], png[None]
    return ref.line_profile_finish(case['raw'], h00, h01, h02, out_h, out_w, case['circle'], case['crop'],
                                   case['half_width'], case['display_range'])


@pytest.mark.parametrize('P', [1, 5])
def test_restatement_matches_the_exact_finish(P):
    cases = adv.cases(P)
    total = Counter()
    disagree = {}
    for case in cases:
        maps, png, cls = run_exact(case)
        total.update(cls)
        disagree[case['name']] = cls['mask_disagree']
        with np.errstate(invalid='ignore', over='ignore'):
            got, got_png = restatement(case, P)
        ex.within(got, maps, case['name'])
        ex.within(got_png, png, case['name'] + ' display')
    print('P=%d classes: %s' % (P, ', '.join('%s %d' % kv for kv in sorted(total.items()))))
    print('P=%d case classes: %s' % (P, adv.case_classes(cases, P)))
    n = sum(disagree.values())
    print('P=%d float64 vs exact circle test: %d pixels differ (%s)' % (P, n, {k: v for k, v in disagree.items() if v}))
    required = adv.REQUIRED + (adv.REQUIRED_PROFILE if P > 1 else ())
    missing = [k for k in required if not total.get(k)]
    assert not missing, 'classes never reached: %s' % missing
    missing = [k for k, v in adv.case_classes(cases, P).items() if not v]
    assert not missing, 'case classes never reached: %s' % missing
    assert n == MASK_DISAGREEMENTS, n


def test_exact_decisions_on_hand_picked_pixels():
    """A few pixels worked out by hand: the whole tap with a NaN neighbour, x = -0.0, t = 0 with an infinite tap, a tie."""
    raw = np.array([[1.5, np.nan, np.inf, 4.0, 2.0 ** -140]], dtype=np.float32)
    m, png, cls = ex.finish(raw, 1.0, 0.0, 0.0, 1, 6, display_range=32767.0 / 256.0)   # scale 256
    assert m[0, 0, 0] == np.float32(1.5)                   # x = 0 whole: one tap, its NaN neighbour unused
    assert np.isnan(m[0, 0, 1]) and np.isnan(m[0, 0, 2])   # the NaN tap; inf with t = 0 gives 1 inf + 0 inf = NaN
    assert m[0, 0, 4] == np.float32(2.0 ** -140) and np.isnan(m[0, 0, 5])    # a denormal kept; x = w outside
    assert png[0, 0, 0] == 32768 + 384 and png[0, 0, 1] == 0
    m, _, cls = ex.finish(raw, -1.0, -1.0, -0.0, 1, 2)
    assert cls['x_neg_zero'] == 1 and m[0, 0, 0] == np.float32(1.5) and np.isnan(m[0, 0, 1])
    m, _, _ = ex.finish(raw, 1.0, 0.0, 2.5, 1, 2)
    assert np.isinf(m[0, 0, 0]) and m[0, 0, 1] == 2.0      # x = 2.5: (1/2) inf + (1/2) 4 = inf; x = 3.5: 2 + (1/2) denormal = 2
    assert cls['x_whole'] == 2                             # (the -0.0 call: x = -0.0 and x = -1)
    assert ex.display_code(2.5, Counter()) == 2 and ex.display_code(3.5, Counter()) == 4
    assert ex.display_code(0.49, Counter()) == 1 and ex.display_code(65535.5, Counter()) == 65535
