"""The cases of tests/test_pitched_rows_gpu.py on the reference alone (no GPU): every warp case has the edge pixels it is
there for, the products discs start and end where they are meant to, and the three route predicates give every GPU case's layout
the kernel the case is about."""
import math

import numpy as np
import pytest

from tests import pitched_cases as pc
from tests.pitched_util import pitch_for


@pytest.mark.parametrize('case', pc.WARP_CASES, ids=pc.WARP_IDS)
def test_warp_case_has_the_positions_it_claims(case):
    pc.assert_warp_case(case)


def test_warp_cases_cover_the_edges_between_them():
    """Each fact the table speaks of belongs to at least one case, and the cases take both launch shapes."""
    claimed = set()
    for case in pc.WARP_CASES:
        claimed.update(case[8])
    everything = set(pc.warp_facts(*pc.WARP_CASES[0][1:8]))
    assert claimed == everything, sorted(everything - claimed)
    shapes = {pc.warp_facts(*c[1:8], only=('four_vectors_a_thread',))['four_vectors_a_thread'] for c in pc.WARP_CASES}
    assert shapes == {False, True}


def test_warp_image_keeps_the_padding_value_out():
    img = pc.warp_image(64, 203, 23131)
    assert img[0, 0] == 31337 and not (img == 23131).any()
    assert img[1:].min() >= 2000 and img.max() <= 60001


def test_warp_cases_are_wide_and_the_unaligned_one_is_not():
    from solex_ser_recon_en_amd._lib import lib
    base = 1 << 20
    for name, h, w, oh, ow, h00, h01, h02, _ in pc.WARP_CASES:
        args = (h, w, pitch_for(w), h00, h01, h02, base, oh, ow, pitch_for(ow))
        assert lib.shg_warp_rows_wide_fits(base, *args) == 1, name
        assert lib.shg_warp_rows_wide_fits(base + 2, h, w, pitch_for(w, 1), h00, h01, h02, base, oh, ow, pitch_for(ow)) == 0, name
        if w % 8:
            assert lib.shg_warp_rows_wide_fits(base, h, w, w, h00, h01, h02, base, oh, ow, pitch_for(ow)) == 0, name   # the dense layout


def test_product_discs_are_what_they_are_meant_to_be():
    """Where the discs' row spans start and end relative to the 8-column vectors."""
    for w in pc.ROW_WIDTHS[1:]:
        for h in pc.ROW_HEIGHTS:
            none, tail, past, left, on_vec, single = pc.product_discs(h, w)
            t0, y0 = (w // 8) * 8, h // 2
            assert none is None and w % 8 != 0
            assert t0 <= tail[0] + tail[2] <= w - 1 and tail[0] - tail[2] < t0         # ends inside the partial last vector
            assert past[0] + past[2] >= w > past[0] - past[2]                          # reaches past the width
            assert left[0] + left[2] < 0                                               # wholly left
            # r = 4: half = 4 on the centre row, isqrt(15) = isqrt(12) = 3 one and two rows off it
            assert on_vec[2] == 4 and math.isqrt(15) == 3 and math.isqrt(12) == 3
            assert (on_vec[0] - 4) % 8 == 0 and (on_vec[0] + 3) % 8 == 7 and on_vec[0] + 4 < w
            m = pc.disc_mask(h, w, single)
            assert m.sum() == 1 and m[y0, w - 1]                                       # one pixel, in the last column
            if h >= 3:
                m = pc.disc_mask(h, w, on_vec)
                assert m[y0, on_vec[0] - 4] and not m[y0 + 1, on_vec[0] - 4] and m[y0 + 1, on_vec[0] + 3] and not m[y0 + 1, on_vec[0] + 4]


def test_row_cases_take_the_vector_kernels_when_pitched():
    from solex_ser_recon_en_amd._lib import lib
    base = 1 << 20
    for w in pc.ROW_WIDTHS:
        for h in pc.ROW_HEIGHTS:
            p = pitch_for(w)
            assert lib.shg_scale_rows_vec_fits(base, h, w, p, base, p) == 1
            assert lib.shg_scale_rows_vec_fits(base + 2, h, w, pitch_for(w, 1), base + 2, pitch_for(w, 1)) == 0
            assert lib.shg_contrast_products_vec_fits(base, p, base, p, h, w, base, base, base, p) == (1 if w >= 9 else 0)
            assert lib.shg_contrast_products_vec_fits(base + 2, pitch_for(w, 1), base, p, h, w, base, base, base, p) == 0
            if w % 8:
                assert lib.shg_scale_rows_vec_fits(base, h, w, w, base, p) == 0
                assert lib.shg_contrast_products_vec_fits(base, w, base, w, h, w, base, base, base, p) == 0
    assert np.all(np.array(pc.ROW_WIDTHS[1:]) % 8 != 0)
