"""The cases of tests/test_contrast_oracle_gpu.py on the reference alone (no GPU): every image has the histogram, top-bin or
failure property its case names, every case that is not meant to fail leaves rescale_brightness's asserts satisfied, and by the
library's own plan (shg_contrast_plan_query) every case lands on the route its id names -- so that a moved threshold cannot empty
a cell of the GPU matrix unnoticed."""
import numpy as np
import pytest

from oracle import shg_oracle as orc
from tests import contrast_cases as cc
from tests import contrast_ref as ref
from tests import contrast_util as cu


def test_geometry_helpers_are_the_oracles():
    for shape in (cc.A, cc.A1, cc.B, cc.B1, cc.B2, cc.B3):
        for tiles in (1, 2, 3, 4):
            he, we, th, tw = cc.grid(*shape, tiles)
            assert cc.padded(np.zeros(shape, np.uint16), tiles).shape == (he, we) == (th * tiles, tw * tiles)
    for n in (60800, 61305, 274560, 275609, 1048000):
        x = np.random.default_rng(n).permutation(n).astype(np.float64)          # the k-th largest of 0 .. n - 1 is n - k
        k_lo, k_hi = cc.k_tops(n)
        assert k_lo - k_hi == 1 and n - k_lo < np.percentile(x, cc.PCT) < n - k_hi
    assert cc.k_tops(520 * 528) == (2, 1) and cc.k_tops(1000 * 1048) == (3, 2)


def test_crop_plans_are_crop_centers():
    rng = np.random.default_rng(5)
    img = rng.integers(1, 60000, (7, 304)).astype(np.uint16)
    for cx, fixed in ((152, 352), (128, 352), (176, 352), (152, 299), (152, 304), (100, 400), (250, 200), (40, 120)):
        want, _ = orc.crop_center(img, (cx, 3, 2), fixed, False)
        np.testing.assert_array_equal(ref.crop_pad(img, ref.crop_plan(304, cx, fixed)), want, err_msg=str((cx, fixed)))
    # the crops of the case table, as crop_center would have written them: padded on the left, on the right, to an odd width
    assert ref.crop_plan(304, 128, 352) == (352, 0, 48, 304) and ref.crop_plan(304, 176, 352) == (352, 0, 0, 304)
    assert ref.crop_plan(304, 152, 299) == (299, 3, 0, 298)


PLANTED = [(shape, clip, target, layout) for shape, clip in ((cc.A, 1), (cc.A1, 4), (cc.B, 2), (cc.B, 256), (cc.B3, 4), (cc.B3, 256))
           for target in cc.TARGETS for layout in cc.LAYOUTS if not (layout == 'mirror' and shape in (cc.A, cc.B)) and not (layout == 'band' and shape == cc.B3)]


def check_planted(img, tiles, clip, target, seed=0):
    for t, hist in enumerate(cc.tile_hists(img, tiles)):
        v = cc.heavy_value(t, seed)
        assert hist[v] == target + clip, (t, int(hist[v]))
        others = hist.copy()
        others[v] = 0
        assert others.max() <= clip, (t, int(others.max()))
        f = cc.clip_facts(hist, clip)
        assert f == dict(clipped=target, batch=target // 65536, residual=target % 65536,
                         step=65536 // (target % 65536) if target % 65536 else None), (t, f)


@pytest.mark.parametrize('shape,clip,target,layout', PLANTED, ids=['%dx%d-clip%d-%s%d' % (s[0], s[1], c, lay, t) for s, c, t, lay in PLANTED])
def test_planted_histograms_clip_to_their_target(shape, clip, target, layout):
    """Per tile of the PADDED image: the heavy value target + clip times, nothing else above clip, hence clipped = target and the
    batch, residual and step that go with it (1, 2: a count of clip + 1; 21845 | 21846: step 3 -> 2; 32768 | 32769: 2 -> 1; 65535;
    65536: one whole batch, no residual; 65537: a batch and a residual of 1).  What a tile cannot hold is refused, and only that."""
    he, we, th, tw = cc.grid(*shape, 2)
    others = th * tw - target - clip
    holds = others >= 0 and -(-others // clip) + (th + tw if layout == 'mirror' else 0) <= 65535
    if not holds:
        with pytest.raises(cc.Infeasible):
            cc.planted(*shape, 2, clip, target, layout)
        return
    img = cc.planted(*shape, 2, clip, target, layout)
    check_planted(img, 2, clip, target)
    if layout == 'mirror':                                   # the pixels the border repeats went first: rows h - 2 / columns w - 2 are heavy
        h, w = shape
        assert (img[h - 2, :w // 2] == cc.heavy_value(2, 0)).mean() > (0.9 if target > 1000 else 0.002)
        assert img[h - 2, w - 2] == cc.heavy_value(3, 0)
    if layout == 'rows' and target + clip >= th:             # every row of the tile has its share, to within one
        rows = (img[:th, :tw] == cc.heavy_value(0, 0)).sum(axis=1)
        assert rows.max() - rows.min() <= 1 and rows.min() >= 1


def test_planted_refusals_are_the_tiles_that_cannot_hold_the_target():
    """The record of what is skipped: on 200 x 304 (tiles of 15 200 pixels) only targets 1 and 2 fit; on 520 x 528 (68 640) every target
    fits at clip 2 to 256 except where the other pixels would need more than 65535 values."""
    refused = []
    for shape, clip, target, layout in PLANTED:
        _, _, th, tw = cc.grid(*shape, 2)
        if target + clip > th * tw:
            refused.append((shape, target))
    assert {t for s, t in refused if s in (cc.A, cc.A1)} == set(cc.TARGETS) - {1, 2}
    assert not [1 for s, t in refused if s in (cc.B, cc.B3)]


def test_the_model_of_the_clamped_top_on_cases_worked_by_hand():
    """served_from_top on a 521 x 529 image (one border row, one border column) whose brightest value sits c times in the mirrored
    row of one tile, clip 8, k = 2: the tile counts 2c.  2c <= clip: nothing clamped, served.  c = clip: the bin holds min(16, 8) = 8,
    less its 8 border pixels 0 -- the walk passes it and meets a clamped count above where it settles: not served."""
    h, w = cc.B3
    for count, served in ((2, True), (4, True), (8, False), (9, False)):
        img = cc.top_image(h, w, 3, count, 'mirror_row')
        got = cc.served_from_top(img, 2, 8, 2)
        assert (got is not None) == served, (count, got)
        if served:
            assert got == cc.TOP == cc.kth_largest(img, 2)
    img = cc.top_image(*cc.B, 3, 3000, 'scatter')            # no border: always served
    assert cc.served_from_top(img, 2, 8, 2) == cc.TOP and cc.served_from_top(img, 2, 8, 1) == cc.TOP


@pytest.mark.parametrize('c', cc.CASES, ids=cc.IDS)
def test_case_is_what_its_id_says(c, monkeypatch):
    cu.set_knobs(monkeypatch, c['env'])
    p = cu.plan_of(c)
    cu.check_plan(c, p)
    frames = cc.frames_of(c)
    (h, w), tiles, clip, facts = c['shape'], c['tiles'], c['clip'], c['facts']
    assert len(frames) == c['k'] and all(f.shape == (h, w) and f.dtype == np.uint16 for f in frames)
    name, args = c['kind'][0], c['kind'][1:]
    if name == 'planted':
        assert c['crop'] is None and not c['trans']
        for i, img in enumerate(frames):
            check_planted(img, tiles, clip, args[0], c['seed'] + i)
        if facts.get('slices_below_clip'):
            worst = max(cc.heavy_per_slice(img, tiles, p['slice_rows'], c['seed'] + i) for i, img in enumerate(frames))
            assert 0 < worst < clip < args[0] + clip and p['slices'] > 1, (worst, clip, p)
    if name == 'top':
        count, place, second = args
        k_lo, k_hi = cc.k_tops(h * w)
        assert count in (k_lo - 1, k_lo, clip, clip + 1) or count >= 1000, count
        fell = 0
        for i, img in enumerate(frames):
            assert int((img == cc.TOP).sum()) == (count if i % 2 == 0 else 0) and img.max() == (cc.TOP if i % 2 == 0 else 60000)
            if i % 2 == 0:
                a, b = cc.kth_largest(img, k_hi), cc.kth_largest(img, k_lo)
                assert a - b == (0 if facts['top'] == 'one' else 1), (a, b)
                if place == 'mirror_row':
                    assert h % tiles and (img[h - 2] == cc.TOP).sum() == count
                if place == 'mirror_col':
                    assert w % tiles and (img[:, w - 2] == cc.TOP).sum() == count
            for k in (k_lo, k_hi):
                got = cc.served_from_top(img, tiles, clip, k)
                assert got is None or got == cc.kth_largest(img, k)
            fell += cc.falls_back(img, tiles, clip)
        assert fell == c['fallback'], (fell, c['fallback'])
    elif c['fallback'] is not None:
        assert p['from_top'] and sum(cc.falls_back(img, tiles, clip) for img in frames) == c['fallback']
    if facts.get('all_bins'):
        assert all(np.bincount(img.ravel(), minlength=65536).min() >= 1 for img in frames)
    if 'values' in facts:
        assert all(tuple(np.unique(img)) == facts['values'] for img in frames)
    if facts.get('disjoint'):
        for img in frames:
            occupied = cc.tile_hists(img, tiles) > 0
            assert occupied.sum(axis=0).max() == 1 and occupied.any(axis=1).all()        # no value in two tiles
            assert len(np.unique(img // 4096)) == 16
    if facts.get('byte_edges'):
        assert all(np.isin(img & 255, (0, 255)).all() and len(np.unique(img >> 8)) >= 255 for img in frames)
    # the condition on the inputs: rescale_brightness's asserts hold on every disk of every case that is not there to fail
    for i, img in enumerate(frames):
        factors = cu.oracle_transversalium(img)[1] if c['trans'] else None
        bad = ref.raises(img, factors=factors, crop=c['crop'], disc=c['disc'], clip_limit=c['clip_limit'], tiles=tiles)
        want_bad = c['fails'] and (name != 'one_bad' or i == 1)
        assert bad == want_bad, (c['id'], i, bad)


def test_every_cell_of_the_matrix_is_occupied(monkeypatch):
    """Counter widths, slice and chunk structure, disk-count thresholds, image formation, tile grids, discs, the fall-back and the
    failures: each by at least one case, as the plan (asked afresh here) and the table say."""
    table = []
    for c in cc.CASES:
        cu.set_knobs(monkeypatch, c['env'])
        table.append((c, cu.plan_of(c)))
    good = [(c, p) for c, p in table if not c['fails']]

    def some(pred):
        return any(pred(c, p) for c, p in good)
    top = lambda c: cc.k_tops(c['shape'][0] * c['out_w'])[0]
    # counters
    assert some(lambda c, p: p['route'] == 'u16' and p['batched'] and top(c) > p['clip'] and 'SHG_CLAHE_SAT' not in c['env'])
    for clip in (2, 15):
        assert some(lambda c, p: p['route'] == 'nibble' and p['bits'] == 4 and p['clip'] == clip)
    for clip in (16, 255):
        assert some(lambda c, p: p['route'] == 'byte' and p['bits'] == 8 and p['clip'] == clip)
    assert some(lambda c, p: p['route'] == 'byte' and p['clip'] <= 15 and c['env'].get('SHG_CLAHE_SAT') == '8')
    assert some(lambda c, p: p['route'] == 'u16' and p['clip'] == 256 and p['batched'])
    assert some(lambda c, p: p['route'] == 'atomics16' and not p['batched'] and c['clip_limit'] == 0 and c['k'] > 1)
    # slices
    for route in ('u16', 'byte', 'nibble'):
        assert some(lambda c, p: p['route'] == route and p['slices'] == 1) and some(lambda c, p: p['route'] == route and p['slices'] > 1)
    assert some(lambda c, p: p['bits'] == 8 and p['slices'] == 1 and p['slice_rows'] > p['chunk_rows'] and int(c['env'].get('SHG_CLAHE_SAT_PX', 0)) > 65280)
    assert some(lambda c, p: p['bits'] == 4 and p['slices'] == 1 and p['slice_rows'] > p['chunk_rows'] and int(c['env'].get('SHG_CLAHE_SAT_PX', 0)) > 65280)
    for bits in (8, 4):
        assert some(lambda c, p: p['bits'] == bits and c['env'].get('SHG_CLAHE_SAT_PX') == '5000' and p['slices'] >= 6)
    # disk counts and what hangs on them
    assert {c['k'] for c, p in good if p['batched']} >= {1, 2, 4, 5, 8}
    for k, px, window, lut_all in ((2, 4, 0, 0), (4, 8, 1, 0), (5, 8, 1, 0), (8, 8, 1, 1)):
        assert some(lambda c, p: c['k'] == k and not c['env'] and (p['blend_px'], p['window'], p['lut_all']) == (px, window, lut_all)), k
    assert some(lambda c, p: p['route'] == 'u16' and c['k'] >= 4 and p['slice_rows'] > 32768 // cc.grid(c['shape'][0], c['out_w'], c['tiles'])[3])
    assert some(lambda c, p: p['route'] == 'u16' and c['k'] < 4 and p['slices'] > 1)
    # image formation
    pads = lambda c: None if not c['crop'] else ('left' if c['crop'][2] > 0 else '') + ('right' if c['crop'][2] + c['crop'][3] < c['crop'][0] else '') + \
        ('odd' if c['crop'][0] % 2 else '')
    for fused in (1, 0):
        for trans in (True, False):
            assert some(lambda c, p: p['fused'] == fused and c['trans'] == trans and p['batched']), (fused, trans)
        assert some(lambda c, p: p['fused'] == fused and c['crop'] is None)
        for side in ('left', 'right', 'odd'):
            assert some(lambda c, p: p['fused'] == fused and c['crop'] and side in pads(c)), (fused, side)
    assert some(lambda c, p: c['keep'] and c['trans'] and not p['fused'])
    # tile grids
    for tiles in (1, 2, 3, 4):
        kinds = {(c['shape'][0] % tiles != 0, c['out_w'] % tiles != 0) for c, p in good if c['tiles'] == tiles}
        assert kinds >= ({(False, False)} if tiles == 1 else {(False, False), (True, False), (False, True), (True, True)}), (tiles, kinds)
    # discs
    h_w = lambda c: (c['shape'][0], c['out_w'])
    for kind in ('none', 'inside', 'cover', 'off', 'r1'):
        assert some(lambda c, p: c['disc'] == cc.discs(*h_w(c))[kind]), kind
    # the frame percentile: from the top, by the reduction's own ranks, by the select over the image
    assert some(lambda c, p: p['from_top'] and c['fallback'] == 0) and some(lambda c, p: p['from_top'] and (c['fallback'] or 0) > 0)
    assert some(lambda c, p: p['from_top'] and c['fallback'] and 0 < c['fallback'] < c['k'])             # served and fall-back disks in one launch
    assert some(lambda c, p: p['batched'] and not p['from_top'])
    # the failures: alone and inside a stack, batched and disk by disk
    bad = [c for c in cc.CASES if c['fails']]
    assert {c['kind'][0] for c in bad} == {'const', 'zero', 'one_bad'} and {c['k'] for c in bad} >= {1, 2, 3}
    assert len(set(cc.IDS)) == len(cc.IDS)


def test_the_series_through_one_workspace_is_what_it_says():
    """The same image twice, a much brighter and a much darker one, back, a stack of mixed levels (from four disks: the window's
    default), back: by the 10th percentile of the image, which is what the window follows."""
    p10 = [[float(np.percentile(f, 10)) for f in cc.series_frames(s)] for s in range(len(cc.SERIES))]
    assert np.array_equal(cc.series_frames(0)[0], cc.series_frames(1)[0]) and np.array_equal(cc.series_frames(0)[0], cc.series_frames(4)[0])
    assert p10[2][0] > 20 * p10[0][0] and p10[3][0] < p10[0][0] / 5
    assert len(p10[5]) == 4 and max(p10[5]) > 20 * min(p10[5])
    for s in range(len(cc.SERIES)):
        for f in cc.series_frames(s):
            assert not ref.raises(f, clip_limit=cc.clip_limit_for(cc.SERIES_CLIP, 260 * 264), tiles=2)
