"""The eight-pixels-a-lane row kernels on the layout production gives them: k_warp_rows8 (csrc/warp.hip), k_scale_rows8
(csrc/transversalium.hip) and k_products8 (csrc/post.hip) run only on images whose pitch is a multiple of 8 and whose rows are
16-byte aligned -- what ops.pitched_u16 and the arenas allocate, and what a dense test tensor of an odd width is not.  Every case
here puts its images into pitched stores whose padding holds a known value (tests/pitched_util.py), asserts first which kernel
the library's own route predicate picks for that layout, calls the C entry point on the test's own destination stores, compares
bit for bit with a plain float64 reference, and checks that neither the source's nor the destination's padding changed."""
import numpy as np
import pytest

from tests import pitched_cases as pc
from tests.pitched_util import DST_POISON, POISON, padding_untouched, pitched, pitched_blank, view_to_host

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def orc():
    from oracle import shg_oracle
    return shg_oracle


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- warp -------------------------------------------------------------------------------------------------------------------------
_warp_memo = {}          # case id -> (image, reference): the unaligned and the minmax tests reuse two small cases


def _warp_case_data(orc, case):
    name, h, w, oh, ow, h00, h01, h02, _ = case
    if name not in _warp_memo:
        img = pc.warp_image(h, w, POISON)
        data = img, pc.warp_reference(orc, img, oh, ow, h00, h01, h02)
        if oh * ow > 1 << 20:
            return data
        _warp_memo[name] = data
    return _warp_memo[name]


def _run_warp(lib, monkeypatch, img, oh, ow, h00, h01, h02, expect_wide, col0=0, minmax=None):
    """The warp of `img` out of a pitched store into a poisoned one -> the result; the route and both paddings asserted."""
    monkeypatch.delenv('SHG_WARP_WIDE', raising=False)
    h, w = img.shape
    store, src = pitched(img, col0=col0)
    dstore, dst = pitched_blank(oh, ow)
    fits = lib.lib.shg_warp_rows_wide_fits(src.data_ptr(), h, w, store.stride(0), h00, h01, h02, dst.data_ptr(), oh, ow, dstore.stride(0))
    assert fits == (1 if expect_wide else 0), 'the route predicate says %d for this layout' % fits
    if minmax is None:
        mm = torch.zeros(2, dtype=torch.int32, device='cuda')
        lib.check(lib.lib.shg_warp_rows_u16(src.data_ptr(), h, w, store.stride(0), h00, h01, h02, dst.data_ptr(), oh, ow, dstore.stride(0),
                                            mm.data_ptr(), _stream()), 'shg_warp_rows_u16')
        assert mm.cpu().tolist() == [int(img.min()), int(img.max())]                    # the view's extrema, not the padding's
    else:
        mm = torch.tensor(list(minmax), dtype=torch.int32, device='cuda')
        lib.check(lib.lib.shg_warp_rows_minmax_u16(src.data_ptr(), h, w, store.stride(0), h00, h01, h02, dst.data_ptr(), oh, ow,
                                                   dstore.stride(0), mm.data_ptr(), _stream()), 'shg_warp_rows_minmax_u16')
    got = view_to_host(dst)
    assert padding_untouched(dstore, dst, DST_POISON), 'the warp wrote outside its destination view'
    assert padding_untouched(store, src, POISON), 'the warp wrote into its source store'
    return got


@pytest.mark.parametrize('i', range(6))
def test_warp_golden_transforms_from_a_pitched_source(lib, golden, monkeypatch, i):
    """k_warp_rows8 against scikit-image's own output: the six transforms of g3_warp with the 60 x 84 source in a 128-pixel pitch
    (test_warp_golden_bit_exact hands it over dense, pitch 84, and so pins k_warp_rows)."""
    g = golden('g3_warp')
    img, mat3, want = g['image_u16'], g['c%d_mat3' % i], g['c%d_out' % i]
    assert 0.0 <= mat3[0, 0] <= 1.75 and img.shape[1] % 8 != 0
    got = _run_warp(lib, monkeypatch, img, want.shape[0], want.shape[1], float(mat3[0, 0]), float(mat3[0, 1]), float(mat3[0, 2]), True)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('case', pc.WARP_CASES, ids=pc.WARP_IDS)
def test_warp_eight_pixels_a_lane_against_the_oracle(lib, orc, monkeypatch, case):
    """k_warp_rows8 against oracle.shg_oracle.warp_rows (which tests/test_oracle_golden.py pins to scikit-image) at the widths and
    transforms where its window, its padding columns (w_last, the last_piece clamp, cval for what the pieces read beyond w) and its
    two launch shapes can go wrong.  The padding holds a value inside the image's range: a sample taken from it survives the clip."""
    pc.assert_warp_case(case)
    name, h, w, oh, ow, h00, h01, h02, _ = case
    img, want = _warp_case_data(orc, case)
    got = _run_warp(lib, monkeypatch, img, oh, ow, h00, h01, h02, True)
    np.testing.assert_array_equal(got, want)


def test_warp_falls_back_on_rows_that_are_not_16_byte_aligned(lib, orc, monkeypatch):
    """The same image one column into its store: the predicate must say no, and k_warp_rows must give the oracle's result."""
    case = pc.WARP_CASES[pc.WARP_IDS.index('w17')]
    name, h, w, oh, ow, h00, h01, h02, _ = case
    img, want = _warp_case_data(orc, case)
    got = _run_warp(lib, monkeypatch, img, oh, ow, h00, h01, h02, False, col0=1)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('name', ['w15', 'typical'])
def test_warp_with_given_extrema_clips_to_them(lib, orc, monkeypatch, name):
    """shg_warp_rows_minmax_u16 (the extrema extraction left on the device) with a pair narrower than the image's own: the clip
    bites on both sides, and the reference clips to that pair."""
    case = pc.WARP_CASES[pc.WARP_IDS.index(name)]
    _, h, w, oh, ow, h00, h01, h02, _ = case
    img, plain = _warp_case_data(orc, case)
    lo, hi = 20000, 41000
    want = pc.warp_reference(orc, img, oh, ow, h00, h01, h02, minmax=(lo, hi))
    assert (plain < lo).any() and (plain > hi).any() and want.min() == lo and want.max() == hi
    got = _run_warp(lib, monkeypatch, img, oh, ow, h00, h01, h02, True, minmax=(lo, hi))
    np.testing.assert_array_equal(got, want)


# ---- scale rows -------------------------------------------------------------------------------------------------------------------
# per-row factors: 0, exactly 1, two that saturate, and ones whose products with the planted pixels are whole numbers (0.5 x even,
# 5 x 13107 = 3 x 21845 = 65535 exactly, 1.25 x multiples of four), then ordinary ones
SCALE_C = [0.0, 1.0, 40.0, 0.5, 5.0, 3.0, 1.25, 0.7310585786300049, 2.0, 1.0000000001, 65535.0, 0.9999999999]
SCALE_RF = [1.0, 0.5, 1.03125, 0.9173, 2.0, 1.0 / 3.0, 1.09]


def _scale_image(h, w):
    rng = np.random.default_rng(h * 10007 + w)
    img = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    img[:, ::3] &= 0xfffc                                            # multiples of four
    plant = np.array([13107, 21845, 65535, 0, 2], np.uint16)          # (rotated with a period that shares nothing with SCALE_C's)
    for y in range(h):
        img[y, w - 1] = plant[y % 5]                                 # the row's last pixel: in the partial vector where there is one
        img[y, (w // 8) * 8 - 1] = plant[(y + 3) % 5]                # the last pixel of the last full vector
        img[y, 0] = plant[(y + 1) % 5]
    return img


def _scale_reference(img, c, rf):
    v = img.astype(np.float64)
    if rf is not None:
        v = v * rf[:, None]                                          # the float64 de-vignetted frame first, then the row's factor
    return np.minimum(v * c[:, None], 65535.0).astype(np.uint16)


def _run_scale(lib, img, c, rf, expect_vec, col0=0):
    h, w = img.shape
    store, src = pitched(img, col0=col0)
    dstore, dst = pitched_blank(h, w, col0=col0)
    fits = lib.lib.shg_scale_rows_vec_fits(src.data_ptr(), h, w, store.stride(0), dst.data_ptr(), dstore.stride(0))
    assert fits == (1 if expect_vec else 0), 'the route predicate says %d for this layout' % fits
    cd = torch.from_numpy(np.ascontiguousarray(c)).cuda()
    rfd = None if rf is None else torch.from_numpy(np.ascontiguousarray(rf)).cuda()
    lib.check(lib.lib.shg_scale_rows_u16(src.data_ptr(), h, w, store.stride(0), cd.data_ptr(), None if rfd is None else rfd.data_ptr(),
                                         dst.data_ptr(), dstore.stride(0), _stream()), 'shg_scale_rows_u16')
    got = view_to_host(dst)
    assert padding_untouched(dstore, dst, DST_POISON), 'scale_rows wrote outside its destination view'
    assert padding_untouched(store, src, POISON), 'scale_rows wrote into its source store'
    return got


def _factor_sets(h):
    """Enough factor vectors of length h that every entry of SCALE_C meets every row position at least once."""
    n = max(1, -(-len(SCALE_C) // h))
    for k in range(n):
        c = np.array([SCALE_C[(k * h + y) % len(SCALE_C)] for y in range(h)])
        rf = np.array([SCALE_RF[(k + 2 * y) % len(SCALE_RF)] for y in range(h)])
        yield c, rf


@pytest.mark.parametrize('w', pc.ROW_WIDTHS)
def test_scale_rows_eight_pixels_a_lane_against_numpy(lib, w):
    """k_scale_rows8 against min(img * rf * c, 65535) truncated, in float64 and in that order: widths of one vector, one pixel past
    one and two vectors, one short of two, around a workgroup's span; row counts around the four rows a lane takes; with and
    without the row factor; factors that are 0, 1, saturate, and land on whole numbers."""
    for h in pc.ROW_HEIGHTS:
        img = _scale_image(h, w)
        for c, rf in _factor_sets(h):
            for factor in (None, rf):
                got = _run_scale(lib, img, c, factor, True)
                np.testing.assert_array_equal(got, _scale_reference(img, c, factor), err_msg='h=%d w=%d rf=%s' % (h, w, factor is not None))


def test_scale_rows_falls_back_on_rows_that_are_not_16_byte_aligned(lib):
    h, w = 5, 17
    img = _scale_image(h, w)
    for c, rf in _factor_sets(h):
        for factor in (None, rf):
            got = _run_scale(lib, img, c, factor, False, col0=1)
            np.testing.assert_array_equal(got, _scale_reference(img, c, factor))


# ---- contrast products ------------------------------------------------------------------------------------------------------------
PRODUCT_BOUNDS = [
    [0.0, 65535.0, 0.0, 65535.0, 0.0, 65535.0],              # q = px: every quotient whole -- every lane takes the exact division
    [1000.0, 14107.0, 0.0, 13107.0, 2000.0, 15107.0],        # span 13107 = 65535 / 5: q = 5 (px - lo), whole again
    [100.0, 103.0, 0.0, 3.0, 65000.0, 65535.0],              # tiny spans: quotients far beyond 65535, some beyond int32's reach of a fraction
    [16383.75, 65535.0, 0.0, 11796.3, 12345.0, 65535.0],     # the shape image_process gives them
    [0.5, 65534.5, 0.0, 1e-3, 7.0, 8.0],                     # a span of 1e-3: every quotient but 0 saturates the conversion
    [9000.0, 61000.0, 0.0, 11000.0, 3000.5, 64000.0],        # an ordinary set
]


def _products_images(h, w, bounds):
    rng = np.random.default_rng(h * 10007 + w + int(bounds[1]))
    img = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    img[::3, ::5] = 0
    img[1::4, 2::7] = 65535
    for k, v in enumerate(bounds):                               # pixels equal to the bounds themselves, the last columns included
        img[(5 + k) % h, (2 + k) % 11::11] = np.uint16(min(max(int(v), 0), 65535))
    return img, np.ascontiguousarray(img[::-1, ::-1])


def _rescale(a, lo, hi):                                         # rescale_brightness, solex_util.py:519-524
    v = 65535.0 * (a.astype(np.float64) - lo) / (hi - lo)
    return np.clip(v, 0, 65535).astype(np.uint16)


def _run_products(lib, stores, h, w, bounds, disc, expect_vec):
    (fstore, frame), (cstore, cl1) = stores
    outs = [pitched_blank(h, w) for _ in range(3)]
    ptrs = [v.data_ptr() for _, v in outs]
    dpitch = outs[0][0].stride(0)
    fits = lib.lib.shg_contrast_products_vec_fits(frame.data_ptr(), fstore.stride(0), cl1.data_ptr(), cstore.stride(0), h, w,
                                                  ptrs[0], ptrs[1], ptrs[2], dpitch)
    assert fits == (1 if expect_vec else 0), 'the route predicate says %d for this layout' % fits
    import ctypes
    b6 = (ctypes.c_double * 6)(*bounds)
    x0, y0, r = disc if disc is not None else (0, 0, 0)
    lib.check(lib.lib.shg_contrast_products_u16(frame.data_ptr(), fstore.stride(0), cl1.data_ptr(), cstore.stride(0), h, w, b6,
                                                ptrs[0], ptrs[1], ptrs[2], dpitch, x0, y0, r, _stream()), 'shg_contrast_products_u16')
    got = [view_to_host(v) for _, v in outs]
    for s, v in outs:
        assert padding_untouched(s, v, DST_POISON), 'the products kernel wrote outside a destination view'
    return got


def _check_products(lib, h, w, expect_vec, col0=0):
    for bounds in PRODUCT_BOUNDS:
        img, cl = _products_images(h, w, bounds)
        stores = pitched(img, col0=col0), pitched(cl)
        want_hc, want_p, want_cc = _rescale(img, bounds[0], bounds[1]), _rescale(img, bounds[2], bounds[3]), _rescale(cl, bounds[4], bounds[5])
        for disc in pc.product_discs(h, w):
            hc, protus, cc = _run_products(lib, stores, h, w, bounds, disc, expect_vec)
            msg = 'h=%d w=%d bounds=%s disc=%s' % (h, w, bounds, disc)
            np.testing.assert_array_equal(hc, want_hc, err_msg=msg)
            np.testing.assert_array_equal(cc, want_cc, err_msg=msg)
            p = want_p
            if disc is not None:
                p = want_p.copy()
                p[pc.disc_mask(h, w, disc)] = 80
            np.testing.assert_array_equal(protus, p, err_msg=msg)
        for s, v in stores:
            assert padding_untouched(s, v, POISON), 'the products kernel wrote into a source store'


@pytest.mark.parametrize('w', pc.ROW_WIDTHS[1:])
def test_products_eight_pixels_a_lane_against_numpy(lib, w):
    """k_products8 against rescale_brightness in float64 and cv2.circle's fill by integer square roots: the widths and heights of the
    scale-rows test (two vectors a row at least), bounds that send whole vectors through the exact-division fallback and an
    ordinary set, discs whose row spans end in the partial last vector, run past the width, miss the image, sit on vector
    boundaries, or are one pixel in the last column."""
    for h in pc.ROW_HEIGHTS:
        _check_products(lib, h, w, True)


def test_products_fall_back_on_rows_that_are_not_16_byte_aligned(lib):
    _check_products(lib, 7, 17, False, col0=1)
