"""The NumPy statement of the line filter (tests/linfilter_ref.py) is itself right: bit for bit the oracle's apply_lin_filter at
the product's parameters, its borders true REFLECT_101, and every case the GPU tests run within the kernels' preconditions and
within the cap on undecidable pixels.  No GPU."""
import math

import numpy as np
import pytest

from oracle import shg_oracle as orc
from tests import linfilter_ref as ref


def _product_arguments(circle, borders, h, w):
    """(taper, xa, xb, edge, edge_half, y1, y2) as correct_transversalium2_batch builds them."""
    from solex_ser_recon_en_amd import solex_util as su
    y1 = math.ceil(max(circle[1] - circle[2], borders[1]))
    y2 = math.floor(min(circle[1] + circle[2], borders[3]))
    taper = np.zeros(h)
    taper[y1:y2] = su._tukey(y2 - y1)
    xa, xb, edge, edge_half = su._limb_edge_plan(circle, h, w, su.LIN_LEN + su.LIN_EDGE_FUDGE)
    return taper, xa, xb, edge, edge_half, y1, y2


def _g15(golden):
    g = golden('g15_stubborn')
    img, circle, borders = g['image'], tuple(g['circle']), list(g['borders'])
    with np.errstate(all='ignore'):
        _, flag = orc.correct_transversalium2_stubborn(img, circle, borders, 301)
    assert flag.sum() >= 3
    return img, g['row_factor'], circle, borders, flag


def _synthetic():
    rng = np.random.default_rng(21)
    h, w = 48, 1200
    img = ref._image(rng, h, w)
    flag = np.zeros(h, dtype=bool)
    flag[[0, 1, 9, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 47]] = True       # both ends, an isolated row, a run of 12
    return img, ref._row_factor(rng, h), (612.0, 22.5, 470.0), [0, 0, w - 1, h - 1], flag


@pytest.mark.parametrize('which', ['g15', 'synthetic1200'])
@pytest.mark.parametrize('path', ['u16', 'f64'])
def test_reference_equals_the_oracle_at_the_product_parameters(golden, which, path):
    img, rf, circle, borders, flag = _g15(golden) if which == 'g15' else _synthetic()
    h, w = img.shape
    src = img * rf[:, None] if path == 'f64' else img
    taper, xa, xb, edge, edge_half, y1, y2 = _product_arguments(circle, borders, h, w)
    assert edge.any() and (edge == 0).any()
    up, dn = orc.neighbour_rows(flag)
    hl, hf, pre, expo = ref.lin_filter(src, flag, up, dn, 101, 5, taper, xa, xb, edge, edge_half)
    want = orc.apply_lin_filter(src, flag, y1, y2, circle)
    assert pre.dtype == want.dtype == np.float64 and np.isfinite(want).all()
    np.testing.assert_array_equal(pre, want)
    assert np.count_nonzero(pre != src) > 1000                                       # the filter did something
    np.testing.assert_array_equal(ref.expected_u16(pre), np.minimum(want, 65535).astype(np.uint16))


@pytest.mark.parametrize('n', [1, 2, 3, 4, 7, 40])
def test_reflect101_wraps(n):
    """Against the definition: walk from 0 and turn round at either end, for indices many periods away on both sides."""
    want, i, step = [], 0, 1
    for _ in range(6 * n + 5):
        want.append(i)
        if n > 1:
            if i + step in (-1, n):
                step = -step
            i += step
    k = np.arange(len(want))
    np.testing.assert_array_equal(ref.reflect101(k, n), want)
    np.testing.assert_array_equal(ref.reflect101(-k, n), want)                      # REFLECT_101 is even about 0
    assert ref.reflect101(np.arange(-300, 300), n).min() >= 0 and ref.reflect101(np.arange(-300, 300), n).max() <= n - 1


@pytest.mark.parametrize('shape,k', [((3, 40), 101), ((2, 1), 21), ((2, 2), 9), ((2, 300), 21), ((1, 513), 511), ((2, 7), 1)])
def test_the_oracle_row_sums_pad_is_reflect101(shape, k):
    """np.pad(mode='reflect') wider than the array, as row_box_sums_reflect101 uses it, is the wrapped REFLECT_101."""
    a = np.log(np.random.default_rng(5).integers(1, 65536, shape).astype(np.uint16))
    np.testing.assert_array_equal(orc.row_box_sums_reflect101(a, k), ref.row_box_sums_by_index(a, k))


def test_cases_cover_what_they_are_for():
    cs = {c['name']: c for c in ref.cases()}
    want = {(24, 1100, 101, 5), (12, 1024, 101, 5), (12, 513, 101, 5), (12, 511, 101, 5), (12, 512, 101, 5), (16, 1537, 511, 2),
            (30, 700, 1, 3), (9, 600, 3, 1), (4, 40, 101, 5), (1, 300, 21, 2), (20, 1, 21, 2), (20, 900, 101, 5)}
    assert want <= {(c['h'], c['w'], c['linlen'], c['half_width']) for c in cs.values()}
    assert len(cs) == len(ref.cases())
    for c in cs.values():
        assert c['img'].shape == (c['h'], c['w']) and c['img'].dtype == np.uint16
        assert c['img'].size <= 60000 and c['purpose']
        if c['name'] != 'nonfinite':
            assert c['img'].min() >= 1
        assert set(c['paths']) == ({'u16'} if c['name'] in ('saturation', 'nonfinite') else {'u16', 'f64'})
    # flag patterns
    assert any(not c['flagged'].any() for c in cs.values())
    all_f = [c for c in cs.values() if c['flagged'].all()]
    assert all_f and all((c['up'] == -1).all() and (c['dn'] == -1).all() for c in all_f)
    assert any(c['flagged'][0] and c['flagged'][-1] and not c['flagged'].all() for c in cs.values())
    assert any(((c['up'] == -1) & c['flagged']).any() and ((c['dn'] == -1) & c['flagged']).any() and not c['flagged'].all()
               for c in cs.values())
    run = cs['24x1100']['flagged']
    assert max(len(s) for s in ''.join('x' if f else ' ' for f in run).split()) > 2 * cs['24x1100']['half_width']
    # edge plans: the circle plan's source columns on the seams with the chord ends in different segments; the hand plan on 512 / 511
    c = cs['24x1100']
    both = c['edge'] == 3
    assert (both & (c['xa'] + c['edge_half'] == 512) & ((c['xb'] - c['edge_half'] - 1) % ref.SEG == 511)
            & (c['xa'] // ref.SEG != (c['xb'] - 1) // ref.SEG)).any()
    c = cs['12x1024']
    assert ((c['edge'] == 3) & (c['xa'] + c['edge_half'] == 512)).any() and ((c['edge'] == 3) & (c['xb'] - c['edge_half'] - 1 == 511)).any()
    assert (c['xa'] == c['xb']).any() and (c['edge'] == 1).any() and (c['edge'] == 2).any()
    assert any((c['taper'] == 0).any() and (c['taper'] == 1).any() and ((c['taper'] > 0) & (c['taper'] < 1)).any() for c in cs.values())
    # the view case: a wider zero-filled tensor, an odd element offset
    off, width, sentinel = cs['20x900view']['view']
    assert off * 2 % 16 and off + 900 < width and sentinel == 0
    # linlen 1: hl is the log itself
    hl = ref.reference(cs['30x700'], 'u16')[0]
    np.testing.assert_array_equal(hl, np.log(cs['30x700']['img']).astype(np.float64))
    # all rows flagged: hf == 0
    assert not ref.reference(cs['12x512'], 'u16')[1].any()


@pytest.mark.parametrize('name,path', ref.case_ids())
def test_case_is_within_the_preconditions_and_the_band_cap(name, path):
    c = next(c for c in ref.cases() if c['name'] == name)
    h, w, eh = c['h'], c['w'], c['edge_half']
    xa, xb, edge = c['xa'].astype(np.int64), c['xb'].astype(np.int64), c['edge']
    assert c['linlen'] % 2 == 1 and 1 <= c['linlen'] <= 511 and c['half_width'] >= 1 and eh >= 0 and 0 < h < 65536 and w > 0
    for a in (c['flagged'], c['up'], c['dn'], c['taper'], xa, xb, edge):
        assert a.shape == (h,)
    assert ((0 <= xa) & (xa <= xb) & (xb <= w)).all()
    left, right = (edge & 1) != 0, (edge & 2) != 0
    assert (xa[left] + eh < w).all() and (xb[right] - eh - 1 >= 0).all() and (edge < 4).all()
    assert (xb[left & right] - xa[left & right] >= 2 * eh + 1).all()
    # a one-sided zone lies inside [xa, xb) as well: the kernel writes nothing outside it, a NumPy slice would
    assert (xa[left] + eh < xb[left]).all() and (xb[right] - eh - 1 >= xa[right]).all()
    assert ((c['up'] >= -1) & (c['up'] < h) & (c['dn'] >= -1) & (c['dn'] < h)).all()
    assert (c['up'][c['flagged']] < np.flatnonzero(c['flagged'])).all()
    assert not c['flagged'][c['up'][c['flagged'] & (c['up'] >= 0)]].any() and not c['flagged'][c['dn'][c['flagged'] & (c['dn'] >= 0)]].any()
    assert np.isfinite(c['taper']).all() and (c['taper'] >= 0).all() and (c['taper'] <= 1).all()
    src, rf = ref.source(c, path)
    hl, hf, pre, expo = ref.reference(c, path)
    assert hl.dtype == hf.dtype == pre.dtype == expo.dtype == np.float64 and hl.shape == hf.shape == pre.shape == expo.shape == (h, w)
    exact, decidable, inband = ref.classify(pre, expo)
    assert not (exact & decidable).any() and not (exact & inband).any() and (exact | decidable | inband).all()
    print('LINFILTER %-12s %-3s %6d px  exact %6d  decidable %6d  in band %d' % (name, path, pre.size, exact.sum(), decidable.sum(),
                                                                               inband.sum()))
    assert inband.sum() <= ref.BAND_CAP
    assert decidable.sum() >= pre.size // 4 or name == '20x1'                       # the case tests the exponent, not the identity
    if name != 'nonfinite':
        assert np.isfinite(hl).all() and np.isfinite(hf).all() and np.isfinite(pre).all()
        if rf is not None:
            assert src.max() < 65535


def test_saturation_case_saturates():
    c = next(c for c in ref.cases() if c['name'] == 'saturation')
    assert c['img'].min() >= 60000 and c['flagged'][0] and c['up'][0] == -1
    hl, hf, pre, expo = ref.reference(c, 'u16')
    np.testing.assert_array_equal(hf[0], orc.row_box_sums_reflect101((np.log(c['img'][c['dn'][0]]) / 2)[None], 101)[0])   # half
    kept = (np.arange(c['w'])[None, :] >= c['xa'][:, None]) & (np.arange(c['w'])[None, :] < c['xb'][:, None]) & (c['taper'] != 0)[:, None]
    over = pre > 65535
    assert over[kept].mean() >= 0.05, over[kept].mean()
    assert (ref.expected_u16(pre)[over] == 65535).all() and expo[over].min() > 0
    assert (pre[kept] < 60000).mean() >= 0.05                                       # and the halved hf darkens the rows near the top


def test_nonfinite_case_has_its_three_kinds():
    c = next(c for c in ref.cases() if c['name'] == 'nonfinite')
    hl, hf, pre, expo = ref.reference(c, 'u16')
    want = ref.expected_u16(pre)
    # (a) -inf under hl and under the neighbouring rows' hf
    assert hl[3, 100] == -np.inf and hf[4, 100] == -np.inf and np.isnan(expo[3, 100]) and c['taper'][3] == 1 and want[3, 100] == 0
    assert np.isnan(expo[3, 95:111]).all() and (want[3, 95:111] == 0).all()
    # (b) a flagged row between clean ones: hl = -inf, hf finite, delta = -inf, exp = +inf; the zero pixel itself is 0 * inf
    assert c['flagged'][9] and not c['flagged'][8] and not c['flagged'][10] and c['taper'][9] == 1
    assert (hl[9, 505:526] == -np.inf).all() and np.isfinite(hf[9]).all() and (expo[9, 505:526] == np.inf).all()
    assert (want[9, 505:515] == 65535).all() and (want[9, 516:526] == 65535).all() and np.isnan(pre[9, 515]) and want[9, 515] == 0
    assert np.isfinite(pre[[7, 8, 10, 11]]).all()
    # (c) the same on a row whose taper is 0
    assert c['flagged'][13] and c['taper'][13] == 0 and np.isnan(expo[13, 440:461]).all() and (want[13, 440:461] == 0).all()
    assert (expo[13, :440] == 0).all() and (expo[13, 461:] == 0).all()
    # rows 3 and 4: NaN where both windows overlap (columns 94..110), +inf on the four columns only the row's own window covers
    assert np.isnan(pre).sum() == 17 + 17 + 1 + 21 and np.isposinf(pre).sum() == 4 + 4 + 20


def test_expected_u16_is_the_headers_rule():
    pre = np.array([np.nan, np.inf, 65535.0, 65535.5, 65534.999, 0.0, 0.999, 1.0, 1e300, 12345.678])
    np.testing.assert_array_equal(ref.expected_u16(pre), [0, 65535, 65535, 65535, 65534, 0, 0, 1, 65535, 12345])
    exact, decidable, inband = ref.classify(pre, np.ones_like(pre))
    np.testing.assert_array_equal(inband, [0, 0, 1, 0, 0, 1, 0, 1, 0, 0])
    np.testing.assert_array_equal(ref.classify(np.array([7.0, 7.5, 7.0000001, 65535.0000001]), np.array([0.0, -0.0, 1.0, 1.0]))[0], [1, 1, 0, 0])
    assert ref.classify(np.array([7.0000001, 6.9999999, 65535.0000001, 65534.9999999]), np.ones(4))[2].all()


def test_disk_frame_gets_rows_flagged():
    """The stage-4 frame: circle inside the frame, chords across the seam at 512, and the oracle flags the brightened rows."""
    img, rf, circle, borders = ref.disk_frame()
    assert img.shape == (160, 1100) and img.min() >= 1 and (img * rf[:, None]).max() < 65535
    assert circle[0] - circle[2] > 0 and circle[0] + circle[2] < 1099 and circle[1] - circle[2] > 0 and circle[1] + circle[2] < 159
    assert circle[0] - circle[2] < ref.SEG < circle[0] + circle[2]
    for src in (img, img * rf[:, None]):
        with np.errstate(all='ignore'):
            _, flag = orc.correct_transversalium2_stubborn(src, circle, borders, 301)
        assert flag.sum() >= 3 and flag[78:81].all()
