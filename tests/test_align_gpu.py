"""Local alignment points on the GPU: shg_patch_ssd_u16 and shg_stack_combine_field_u16 bit for bit against the restatement written
from the header (tests/align_ref.py).  Patch SSD: images in buffers with odd pitches and a skewed base pointer, the smallest and the
largest patch and search, centres in the corners, on the edges and outside the image, circles that cut a patch and that leave none
of it, one point and more points than a wave of workgroups, equal points, the largest sums, equal images, the refusals.  Field
combine: null and all-zero fields against shg_stack_combine_u16 itself, every capacity, null and non-null fields mixed, random fields
on grids that exercise both store paths, the clamp of the last lattice row and steps that do not divide the size, samples pushed off
a source, a NaN node, odd pitches, the refusals.  End to end: local_fields, stack_disks and stack_scans on the synthetic series and
on three scans against the restatement, and the command line with and without --local."""
import functools
import math
import shutil

import numpy as np
import pytest

from tests import align_ref as ar
from tests import stack_ref as sr
from tests import stack_util as su
from tests.linemaps_util import run_json, write_scan
from tests.stack_util import (E_ARG, E_UNSUPPORTED, GRIDS, LAYOUTS, MODES, PAD, SPECIAL, SSD_FILL, H, W, bits, combine, down16, mods,  # noqa: F401
                              planted_table, random_fields, random_sources, same_fields, same_records, skewed, up16)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

check = functools.partial(su.check, ar.stack_combine_field)


# ---- patch SSD ----
def patch_ssd(lib, ref, img, points, half, search, circle='none', extra=(1, 3), **over):
    """shg_patch_ssd_u16 on skewed, padded buffers into a planted table -> (status, table uint64 [n, words], guards and padding
    intact)."""
    h, w = ref.shape
    a, a_ptr = skewed(ref, extra[0])
    b, b_ptr = skewed(img, extra[1], skew=3)
    pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
    n = over.get('n', len(pts))
    words = (2 * search + 1) ** 2 + 3 if 0 <= search <= 8 else 4
    dev_pts = torch.from_numpy(pts).cuda()
    table, c3 = planted_table(len(pts) * words), su.circle3(circle)
    st = lib.shg_patch_ssd_u16(over.get('ref_ptr', a_ptr), over.get('ref_pitch', w + extra[0]), over.get('img_ptr', b_ptr),
                               over.get('img_pitch', w + extra[1]), over.get('h', h), over.get('w', w), over.get('points_ptr', dev_pts.data_ptr()), n,
                               half, search, None if c3 is None else c3.ctypes.data, over.get('table', table.data_ptr()), None)
    torch.cuda.synchronize()
    got = table.cpu().numpy().view(np.uint64)
    intact = (got[len(pts) * words if st == 0 else 0:] == SSD_FILL).all()
    for dev, src, e, skew in ((a, ref, extra[0], 1), (b, img, extra[1], 3)):
        back = down16(dev)
        assert (back[:skew] == PAD).all() and (back[skew:].reshape(h, w + e)[:, w:] == PAD).all()
        assert np.array_equal(back[skew:].reshape(h, w + e)[:, :w], src)
    return st, got[:len(pts) * words].reshape(len(pts), words), bool(intact)


def check_patch_ssd(lib, ref, img, points, half, search, circle='none'):
    want = ar.patch_ssd(ref, img, points, half, search, None if circle == 'none' else circle)
    st, got, intact = patch_ssd(lib, ref, img, points, half, search, circle)
    assert st == 0 and intact
    su.same(got, want, 'words')
    return want


@pytest.fixture(scope='module')
def pair():
    rng = np.random.default_rng(70)
    ref, img = rng.integers(0, 65536, (H, W)).astype(np.uint16), rng.integers(0, 65536, (H, W)).astype(np.uint16)
    ref.setflags(write=False), img.setflags(write=False)
    return ref, img


@pytest.mark.parametrize('circle', ['none', 'cuts'])
@pytest.mark.parametrize('half, search', [(1, 0), (1, 1), (1, 8), (32, 0), (32, 1), (32, 8), (16, 4)])
def test_patch_ssd_matches_the_restatement(mods, pair, half, search, circle):
    """Every special centre.  'cuts': a disk of 24 px around row 33.4, column 41.7 -- it cuts the larger patches around the inner
    points and, up to a half-size of 16, leaves nothing of those around the corners."""
    _, _, lib = mods
    ref, img = pair
    disk = 'none' if circle == 'none' else (41.7, 33.4, 24.0)
    want = check_patch_ssd(lib, ref, img, SPECIAL, half, search, disk)
    n_off = (2 * search + 1) ** 2
    assert np.array_equal(want[15], want[16]) and want[15, n_off] > 0                            # the equal points
    assert (want[[9, 10, 12, 13, 14]] == 0).all()                                                # outside, beyond any patch
    if circle == 'cuts':
        assert (half > 16 or (want[:4] == 0).all()) and 0 < want[17, n_off] and (half == 1 or want[15, n_off] < (2 * half + 1) ** 2)
    elif half == 1 and search == 0:
        assert want[:8, n_off].tolist() == [4, 4, 4, 4, 6, 6, 6, 6] and want[8, n_off] == 1 and want[15, n_off] == 9


@pytest.mark.parametrize('n', [1, 300])
def test_patch_ssd_one_point_and_more_than_a_wave_of_workgroups(mods, pair, n):
    _, ops, lib = mods
    ref, img = pair
    rng = np.random.default_rng(n)
    points = np.stack([rng.integers(-8, H + 8, n), rng.integers(-8, W + 8, n)], axis=1)
    want = check_patch_ssd(lib, ref, img, points, 5, 2, (44.0, 36.0, 30.0))
    assert n == 1 or ((want[:, 25] == 0).any() and (want[:, 25] == 121).any())
    # the wrapper on pitched views, host points and the caller's table
    a, b = up16(np.pad(ref, ((0, 0), (0, 3))))[:, :W], up16(np.pad(img, ((0, 0), (0, 5))))[:, :W]
    got = ops.patch_ssd_u16(a, b, points, 5, 2, (44.0, 36.0, 30.0))
    assert got.dtype == torch.int64 and tuple(got.shape) == (n, 28) and np.array_equal(got.cpu().numpy().view(np.uint64), want)
    again = ops.patch_ssd_u16(a, b, torch.from_numpy(points.astype(np.int32)).cuda(), 5, 2, (44.0, 36.0, 30.0), out=got.zero_())
    assert again is got and np.array_equal(got.cpu().numpy().view(np.uint64), want)
    for bad in (dict(half=0), dict(half=33), dict(search=9)):
        with pytest.raises(ValueError):
            ops.patch_ssd_u16(a, b, points, **dict(dict(half=5, search=2), **bad))
    with pytest.raises(ValueError):
        ops.patch_ssd_u16(a, b[:-1], points, 5, 2)
    with pytest.raises(ValueError):
        ops.patch_ssd_u16(a, b, points, 5, 2, out=got[:, :-1])


def test_patch_ssd_of_the_largest_sums_and_of_equal_images(mods):
    _, _, lib = mods
    zero, full = np.zeros((90, 95), np.uint16), np.full((90, 95), 65535, np.uint16)
    want = check_patch_ssd(lib, zero, full, [(44, 47)], 32, 8)                                   # a whole 65 x 65 patch, every offset
    assert (want[0, :289] == 65535 ** 2 * 4225).all() and want[0, 289:].tolist() == [4225, 0, 0]
    want = check_patch_ssd(lib, full, zero, [(44, 47), (45, 46)], 32, 8)
    assert (want[:, :289] == 65535 ** 2 * 4225).all() and want[0, 289:].tolist() == [4225, 65535 * 4225, 65535 ** 2 * 4225]
    img = np.random.default_rng(2).integers(0, 65536, (50, 45)).astype(np.uint16)
    want = check_patch_ssd(lib, img, img, [(25, 22), (10, 30)], 7, 4, (22.0, 25.0, 18.0))
    assert (want[:, 40] == 0).all() and (np.delete(want[:, :81], 40, axis=1) > 0).all()
    shifted = np.roll(img, (2, -3), axis=(0, 1))                                  # shifted[r + 2][c - 3] = img[r][c]: the minimum at (-3, 2)
    want = check_patch_ssd(lib, img, shifted, [(25, 22)], 7, 4)
    assert int(np.argmin(want[0, :81])) == (2 + 4) * 9 + (-3 + 4) and want[0, (2 + 4) * 9 + 1] == 0


def test_patch_ssd_refusals_leave_the_table_untouched(mods, pair):
    _, _, lib = mods
    ref, img = pair
    points = [(35, 45), (3, 4)]
    for over, code in ((dict(h=0), E_UNSUPPORTED), (dict(w=16385), E_UNSUPPORTED), (dict(ref_ptr=None), E_ARG), (dict(img_ptr=None), E_ARG),
                       (dict(points_ptr=None), E_ARG), (dict(table=None), E_ARG), (dict(ref_pitch=W - 1), E_ARG), (dict(img_pitch=W - 1), E_ARG),
                       (dict(n=0), E_ARG), (dict(n=-2), E_ARG), (dict(n=(1 << 23) + 1), E_ARG)):
        st, _, intact = patch_ssd(lib, ref, img, points, 4, 2, **over)
        assert st == code and intact, over
    for half, search in ((0, 2), (33, 2), (4, -1), (4, 9)):
        st, _, intact = patch_ssd(lib, ref, img, points, half, search)
        assert st == E_ARG and intact, (half, search)
    for circle in ((float('nan'), 1.0, 5.0), (1.0, float('inf'), 5.0), (1.0, 1.0, float('nan'))):
        st, _, intact = patch_ssd(lib, ref, img, points, 4, 2, circle)
        assert st == E_ARG and intact
    # a table on one of the inputs
    a = up16(ref)
    pts = torch.from_numpy(np.array(points, np.int32)).cuda()
    other = up16(img)
    for table in (a.data_ptr(), a.data_ptr() + 2 * (H * W - 1) - 6, pts.data_ptr()):
        assert lib.shg_patch_ssd_u16(a.data_ptr(), W, other.data_ptr(), W, H, W, pts.data_ptr(), 2, 4, 2, None, table, None) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(down16(a), ref) and pts.cpu().numpy().tolist() == [list(p) for p in points]


# ---- field combine ----
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n', [3, 5, 9, 17])
def test_null_and_zero_fields_are_the_plain_combine(mods, mode, n):
    """Against shg_stack_combine_u16 itself, every capacity; both store paths (pitch 72 from 16-byte rows, and skewed)."""
    _, _, lib = mods
    srcs, xforms = random_sources(n, [(60, 80), (75, 50), (40, 64)], 7 + n, spread=6.0)
    shape = (70, 67)
    zero = np.zeros(ar.lattice_shape(shape, 16) + (2,))
    for how in (dict(out_extra=5, count_extra=5), dict(out_extra=2, count_extra=1, skew=1)):
        st, want, want_count, intact = combine(lib, srcs, xforms, shape, [None] * n, None, 16, mode, 1.3, 2, plain=True, **how)
        assert st == 0 and intact and want_count.max() > 1
        for fields in ([None] * n, [zero] * n, [zero if j % 2 else None for j in range(n)], [-zero] * n):
            st, got, got_count, intact = combine(lib, srcs, xforms, shape, fields, None, 16, mode, 1.3, 2, **how)
            assert st == 0 and intact and np.array_equal(got, want) and np.array_equal(got_count, want_count)


@pytest.mark.parametrize('step', [8, 16])
@pytest.mark.parametrize('shape, layout', GRIDS, ids=['%dx%d_%s' % (g[0] + (g[1],)) for g in GRIDS])
def test_random_fields_match_the_restatement(mods, shape, layout, step):
    """Fields of up to three pixels; 37 and 263 are no multiples of either step (the last cells are partial, the last lattice row
    and column lie beyond the grid), 64 and 256 are (the last row and column of nodes are the clamp's: j1 = gh - 1 is never read with
    a weight); aligned: rows on 16 bytes, the 16-byte stores; the others by element.  A mix of null and non-null fields."""
    _, _, lib = mods
    how = LAYOUTS[layout]
    srcs, xforms = random_sources(5, [(70, 270), (66, 260)], step + shape[1], spread=2.0, scale=0.01)
    fields = random_fields(5, shape, step, 3 * step + shape[0], none=(1, 3))
    for mode in MODES:
        want, count = check(lib, srcs, xforms, shape, mode, 1.2, 2, fields=fields, step=step, **how)
    if shape[0] > 1:
        plain = sr.stack_combine(srcs, xforms, shape, 'mean')[0]
        assert (ar.stack_combine_field(srcs, xforms, fields, step, shape, 'mean')[0] != plain).mean() > 0.5         # the fields do something


@pytest.mark.parametrize('n', [3, 5, 9, 17, 32])
def test_every_capacity_with_fields(mods, n):
    _, _, lib = mods
    srcs, xforms = random_sources(n, [(23, 21), (19, 26)], 100 + n)
    fields = random_fields(n, (20, 19), 8, n, 2.0, none=(0, n - 2))
    for mode in MODES if n < 32 else ('sigma',):
        for iterations in (1, 3) if mode == 'sigma' else (2,):
            want, count = check(lib, srcs, xforms, (20, 19), mode, 1.3, iterations, fields=fields, step=8)
            assert count.max() <= n


def test_a_field_that_pushes_samples_off_a_source_and_a_nan_node(mods):
    _, _, lib = mods
    rng = np.random.default_rng(5)
    img = rng.integers(0, 65536, (24, 40)).astype(np.uint16)
    shape, step = (24, 40), 8
    gh, gw = ar.lattice_shape(shape, step)
    assert (gh, gw) == (4, 6)
    push = np.zeros((gh, gw, 2))
    push[:, 3:, 0] = 30.0                                                        # columns from 24 on read 30 px to the right: off the source
    want, count = check(lib, [img, img], [(1.0, 0.0, 0.0, 1.0)] * 2, shape, 'mean', fields=[push, None], step=step)
    assert (count[:, :17] == 2).all() and (count[:, 24:] == 1).all() and np.array_equal(want[:, 24:], img[:, 24:])
    assert sorted(set(count[:, 17:24].ravel().tolist())) == [1, 2]               # the ramp between the nodes at 16 and 24 crosses the edge
    want, count = check(lib, [img], [(1.0, 0.0, 0.0, 1.0)], shape, 'sigma', fields=[push], step=step)
    assert (count[:, 24:] == 0).all() and (want[:, 24:] == 0).all()
    for bad in (np.nan, np.inf, -np.inf):
        field = np.zeros((gh, gw, 2))
        field[1, 2, 1] = bad                                                     # the node at (8, 16): the four cells around it
        want, count = check(lib, [img, img], [(1.0, 0.0, 0.0, 1.0)] * 2, shape, 'median', fields=[field, None], step=step, out_extra=0, count_extra=0)
        # (on row 0 and column 8 the node's weight is 0, yet 0 * inf is no number: the four cells are absent whole)
        assert (count[0:16, 8:24] == 1).all() and (count[16:, :] == 2).all() and (count[:, 24:] == 2).all() and (count[:, :8] == 2).all()
        assert np.array_equal(want, img)


def test_field_combine_refusals_leave_the_outputs_untouched(mods):
    _, _, lib = mods
    srcs, xforms = random_sources(2, [(20, 22)], 1)
    shape = (18, 20)
    fields = random_fields(2, shape, 8, 4)

    def refused(code, step=8, **over):
        st, _, _, intact = combine(lib, srcs, xforms, shape, fields, None, step, 'sigma', over.pop('kappa', 2.5), over.pop('iterations', 2), **over)
        assert st == code and intact, (step, over)

    for step in (7, 129, 0, -8):
        refused(E_ARG, step)
    for over in (dict(gh=3), dict(gh=5), dict(gw=3), dict(gw=5), dict(no_fields=True), dict(out=None), dict(kappa=0.5), dict(iterations=0)):
        refused(E_ARG, **over)
    # an output or a count plane on a field, a field off 16 bytes
    field = torch.from_numpy(fields[0]).cuda()
    last = field.data_ptr() + field.numel() * 8 - 2
    for over in (dict(out=field.data_ptr()), dict(out=last), dict(count=field.data_ptr() + 64), dict(count=last + 1),
                 dict(field_ptr={1: field.data_ptr() + 8})):
        if 'field_ptr' not in over:
            over['field_ptr'] = {0: field.data_ptr()}
        refused(E_ARG, **over)
    torch.cuda.synchronize()
    assert np.array_equal(bits(field.cpu().numpy()), bits(fields[0]))


def test_ops_wrapper(mods):
    _, ops, _ = mods
    srcs, xforms = random_sources(3, [(30, 33), (28, 36)], 21)
    views = [up16(np.pad(s, ((0, 0), (0, 2))))[:, :s.shape[1]] for s in srcs]
    shape = (29, 31)
    fields = random_fields(3, shape, 8, 9, none=(2,))
    dev = [None if f is None else torch.from_numpy(f).cuda() for f in fields]
    want, want_count = ar.stack_combine_field(srcs, xforms, fields, 8, shape, 'sigma', 1.2, 2)
    out, count = ops.stack_combine_field_u16(views, xforms, dev, 8, shape, 'sigma', 1.2, 2)
    assert out.dtype == torch.uint16 and count.dtype == torch.uint8
    assert np.array_equal(down16(out), want) and np.array_equal(count.cpu().numpy(), want_count)
    # the caller's pitched views
    big, big_c = up16(np.zeros((29, 40))), torch.zeros((29, 37), dtype=torch.uint8, device='cuda')
    again, again_c = ops.stack_combine_field_u16(views, xforms, dev, 8, shape, 'sigma', 1.2, 2, out=big[:, 3:34], count=big_c[:, 1:32])
    assert np.array_equal(down16(again), want) and np.array_equal(again_c.cpu().numpy(), want_count) and (down16(big)[:, :3] == 0).all()
    _, none = ops.stack_combine_field_u16(views, xforms, dev, 8, shape, want_count=False)
    assert none is None
    with pytest.raises(ValueError, match='field'):
        ops.stack_combine_field_u16(views, xforms, [dev[0][:-1], dev[1], None], 8, shape)
    with pytest.raises(ValueError, match='field'):
        ops.stack_combine_field_u16(views, xforms, [dev[0].float(), dev[1], None], 8, shape)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.stack_combine_field_u16(views, xforms, [dev[0].cpu(), dev[1], None], 8, shape)
    with pytest.raises(RuntimeError, match='kappa'):
        ops.stack_combine_field_u16(views, xforms, dev, 8, shape, kappa=0.5)


# ---- end to end: the synthetic series ----
@pytest.fixture(scope='module')
def series():
    """The synthetic series, its records and its fields by the restatement: computed once, never written to."""
    images, true, given = ar.synthetic_series()
    records = sr.register_disks(images, given)
    fields, stats, masks = ar.local_fields(images, records, given, want_measured=True)
    for f in fields[1:]:
        f.setflags(write=False)
    return images, given, records, fields, stats, masks


def test_local_fields_and_stack_disks_match_the_restatement(mods, series):
    stack, _, _ = mods
    images, given, want_records, want_fields, want_stats, masks = series
    dev = [up16(img) for img in images]
    records = stack.register_disks(dev, given)
    same_records(records, want_records)
    fields, stats = stack.local_fields(dev, records, given)
    same_fields(fields, want_fields)
    assert stats == want_stats and stats[0] is None and fields[0] is None and stats[1]['points'] == 18 * 17 and stats[1]['used'] == int(masks[1].sum())
    rows = [(r['s'], r['tx'], r['ty'], r['gain']) for r in want_records]
    for mode, kappa in (('mean', 2.5), ('median', 2.5), ('sigma', 1.0)):
        out, count = stack.stack_disks(dev, records, mode, kappa, 2, fields=fields, step=16)
        want, want_count = ar.stack_combine_field(images, rows, want_fields, 16, images[0].shape, mode, kappa, 2)
        assert np.array_equal(down16(out), want) and np.array_equal(count.cpu().numpy(), want_count)
    # the accuracy on the GPU's results: the restatement's figures to the last digit
    def stack_of(imgs, circles, local):
        rec = stack.register_disks(dev, circles)
        f = None if local is None else stack.local_fields(dev, rec, circles, **local)[0]
        return (down16(stack.stack_disks(dev, rec, 'mean', fields=f, step=None if f is None else 16)[0]), None, rec)

    def fields_of(imgs, rec, circles):
        f, s = stack.local_fields(dev, rec, circles)
        return [None if t is None else t.cpu().numpy() for t in f], s, masks

    got = ar.series_measures(stack_of, fields_of)
    want = ar.series_measures(lambda im, ci, local: ar.stack_series(im, ci, 0, 'mean', local=local), lambda im, rec, ci: (want_fields, want_stats, masks))
    print('on the GPU: rms %.6f px, worst %.6f px, noise %.6f with the fields, %.6f without' %
          (got['rms'], got['worst'], got['noise_local'] / got['frame'], got['noise_global'] / got['frame']))
    for key in ('rms', 'worst', 'noise_local', 'noise_global', 'rejected_inside'):
        assert got[key] == want[key], key
    assert got['rms'] <= ar.TOLERANCE['rms'] and got['worst'] <= ar.TOLERANCE['worst'] and got['rejected_inside'] == 0
    assert got['noise_local'] / got['frame'] <= ar.TOLERANCE['noise'] and got['noise_local'] < got['noise_global']
    # other parameters, another reference, a contrast that leaves nodes out: the same against the restatement
    local = dict(step=24, size=21, search=3, region=0.8, min_contrast=0.055)
    rec = stack.register_disks(dev, given, reference=1)
    fields, stats = stack.local_fields(dev, rec, given, 1, **local)
    want_f, want_s = ar.local_fields(images, sr.register_disks(images, given, 1), given, 1, **local)
    same_fields(fields, want_f)
    assert stats == want_s and fields[1] is None and 0 < stats[0]['used'] < ar.local_fields(images, sr.register_disks(images, given, 1), given, 1,
                                                                                           **dict(local, min_contrast=0.0))[1][0]['used']
    # a rejected frame has no field
    rec[2] = dict(rec[2], rejected=True)
    assert stack.local_fields(dev, rec, given, 1, **local)[0][2] is None


# ---- end to end: three scans ----
LOCAL = {'step': 32, 'size': 25, 'search': 3}


@pytest.fixture(scope='module')
def scans(mods, tmp_path_factory):
    stack = mods[0]
    paths = [write_scan(tmp_path_factory, 'align%d' % i, frames) for i, frames in enumerate(sr.pipeline_series())]
    return {'paths': paths, 'plain': stack.stack_scans(paths), 'local': stack.stack_scans(paths, local=LOCAL)}


def test_stack_scans_is_the_restatement_of_its_disks(mods, scans):
    res, plain = scans['local'], scans['plain']
    images, circles = [down16(t) for t in res['images']], res['circles']
    want, want_count, want_records, want_fields, want_stats = ar.stack_series(images, circles, local=LOCAL)
    same_records(res['records'], want_records)
    same_fields(res['local']['fields'], want_fields)
    assert res['local']['frames'] == want_stats and want_stats[0] is None and want_stats[1]['used'] > 0
    assert {k: res['local'][k] for k in ar.DEFAULTS} == dict(ar.DEFAULTS, **LOCAL)
    assert np.array_equal(down16(res['stack']), want) and np.array_equal(res['count'].cpu().numpy(), want_count)
    assert res['used'] == [0, 1, 2] and (down16(res['stack']) != down16(plain['stack'])).any()
    # without `local`: today's path and today's result
    assert plain['local'] is None
    want, want_count, want_records = sr.stack_series([down16(t) for t in plain['images']], plain['circles'])
    same_records(plain['records'], want_records)
    assert np.array_equal(down16(plain['stack']), want) and np.array_equal(plain['count'].cpu().numpy(), want_count)


def test_command_line_with_and_without_local(mods, scans, tmp_path, capsys):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.png_io import read_png_gray
    stack = mods[0]
    work = []
    for i, path in enumerate(scans['paths']):
        work.append(str(tmp_path / ('scan%d.ser' % i)))
        shutil.copy(path, work[-1])
    k = SHG_MAIN.default_options()['img_rotate'] // 90
    base = work[0][:-4] + '_shift=0_stack'
    out = run_json(stack.main, capsys, work)
    assert out['png'] == base + '.png' and all('local' not in frame for frame in out['frames'])
    assert np.array_equal(read_png_gray(out['png']), np.rot90(down16(scans['plain']['stack']), k))
    plain_keys = sorted(out)
    out = run_json(stack.main, capsys, work + ['--local', '--ap-step', '32', '--ap-size', '25', '--ap-search', '3', '--coverage'])
    assert out['png'] == base + '.png' and out['count_png'] == base + '_count.png' and sorted(out) == plain_keys  # the names do not change
    assert np.array_equal(read_png_gray(out['png']), np.rot90(down16(scans['local']['stack']), k))
    assert np.array_equal(read_png_gray(out['count_png']), np.rot90(scans['local']['count'].cpu().numpy(), k))
    assert [frame['local'] for frame in out['frames']] == scans['local']['local']['frames']
    assert out['frames'][0]['local'] is None and out['frames'][1]['local']['points'] > out['frames'][1]['local']['used'] > 0
    for frame, rec in zip(out['frames'], scans['local']['records']):
        assert frame['offset'] == list(rec['offset']) and frame['rms'] == math.sqrt(rec['ssd_per_pixel'])
    # the defaults
    out = run_json(stack.main, capsys, work + ['--local', '--mode', 'median'])
    other = stack.stack_scans(work, mode='median', local={})
    assert np.array_equal(read_png_gray(out['png']), np.rot90(down16(other['stack']), k))
    assert [frame['local'] for frame in out['frames']] == other['local']['frames'] and other['local']['step'] == 16
