"""Ranking scans by sharpness on the GPU: shg_patch_sharpness_u16 and shg_stack_combine_weighted_u16 bit for bit against the restatement
written from the header (tests/quality_ref.py), in the buffer style of tests/test_align_gpu.py (the helpers are tests/stack_util.py's): odd
pitches, skewed base pointers, planted guard words, inputs verified untouched.  Sharpness: the special centres, the smallest and the
largest patch and arm, circles that cut and that empty, one point and more points than a wave of workgroups, images smaller than
the Laplacian, the largest sums, a constant image, the wrapper, the refusals.  Weighted combine: every capacity, the grids of both
store paths, null and non-null fields and lattices mixed, mean and sigma; the three exact properties against the existing kernels
themselves; NaN, negative and all-zero nodes; the refusals; the wrapper.  End to end: disk_quality, local_quality and stack_disks on
the quadrant series, stack_scans on three scans with and without `quality`, and the command line."""
import functools
import shutil

import numpy as np
import pytest

from tests import align_ref as ar
from tests import quality_ref as qr
from tests import stack_ref as sr
from tests import stack_util as su
from tests.linemaps_util import run_json, write_scan
from tests.stack_util import (E_ARG, E_UNSUPPORTED, GRIDS, LAYOUTS, PAD, SPECIAL, SSD_FILL, H, W, bits, combine, down16, mods,  # noqa: F401
                              planted_table, random_fields, random_sources, random_weights, same_fields, same_records, skewed, up16)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

IDENTITY = (1.0, 0.0, 0.0, 1.0)
check_weighted = functools.partial(su.check, qr.stack_combine_weighted)


# ---- sharpness ----
def sharpness(lib, img, points, half, arm, circle='none', extra=3, **over):
    """shg_patch_sharpness_u16 on a skewed, padded buffer into a planted table -> (status, table uint64 [n, 4], guards and padding
    intact); the image and the points are verified untouched."""
    h, w = img.shape
    a, a_ptr = skewed(img, extra, skew=3)
    pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
    n = over.get('n', len(pts))
    dev_pts = torch.from_numpy(pts).cuda()
    table, c3 = planted_table(len(pts) * 4), su.circle3(circle)
    st = lib.shg_patch_sharpness_u16(over.get('img_ptr', a_ptr), over.get('pitch', w + extra), over.get('h', h), over.get('w', w),
                                     over.get('points_ptr', dev_pts.data_ptr()), n, half, arm, None if c3 is None else c3.ctypes.data,
                                     over.get('table', table.data_ptr()), None)
    torch.cuda.synchronize()
    got = table.cpu().numpy().view(np.uint64)
    intact = (got[len(pts) * 4 if st == 0 else 0:] == SSD_FILL).all()
    back = down16(a)
    assert (back[:3] == PAD).all() and (back[3:].reshape(h, w + extra)[:, w:] == PAD).all()
    assert np.array_equal(back[3:].reshape(h, w + extra)[:, :w], img) and np.array_equal(dev_pts.cpu().numpy(), pts)
    return st, got[:len(pts) * 4].reshape(len(pts), 4), bool(intact)


def check_sharpness(lib, img, points, half, arm, circle='none'):
    want = qr.patch_sharpness(img, points, half, arm, None if circle == 'none' else circle)
    st, got, intact = sharpness(lib, img, points, half, arm, circle)
    assert st == 0 and intact
    su.same(got, want, 'words')
    return want


@pytest.fixture(scope='module')
def image():
    img = np.random.default_rng(71).integers(0, 65536, (H, W)).astype(np.uint16)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize('circle', ['none', 'cuts'])
@pytest.mark.parametrize('half, arm', [(1, 1), (1, 8), (32, 1), (32, 8), (16, 3)])
def test_sharpness_matches_the_restatement(mods, image, half, arm, circle):
    """Every special centre of test_align_gpu.  'cuts': a disk of 24 px around row 33.4, column 41.7 -- it cuts the larger patches
    around the inner points and, up to a half-size of 16, leaves nothing of those around the corners."""
    _, _, lib = mods
    disk = 'none' if circle == 'none' else (41.7, 33.4, 24.0)
    want = check_sharpness(lib, image, SPECIAL, half, arm, disk)
    assert np.array_equal(want[15], want[16]) and want[15, 0] > 0 and want[15, 3] > 0            # the equal points
    assert (want[[9, 10, 12, 13, 14]] == 0).all()                                                # outside, beyond any patch
    if circle == 'cuts':
        assert (half > 16 or (want[:4] == 0).all()) and 0 < want[17, 0] and (half == 1 or want[15, 0] < (2 * half + 1) ** 2)
    elif half == 1 and arm == 1:
        assert want[:8, 0].tolist() == [1, 1, 1, 1, 3, 3, 3, 3] and want[8, 0] == 0 and want[15, 0] == 9
    elif half == 1 and arm == 8:
        assert (want[:9] == 0).all() and want[15, 0] == 9                                        # the corners and edges lie within the arm


@pytest.mark.parametrize('n', [1, 300])
def test_sharpness_of_one_point_and_of_more_than_a_wave_of_workgroups(mods, image, n):
    _, ops, lib = mods
    rng = np.random.default_rng(n)
    points = np.stack([rng.integers(-8, H + 8, n), rng.integers(-8, W + 8, n)], axis=1)
    want = check_sharpness(lib, image, points, 5, 2, (44.0, 36.0, 30.0))
    assert n == 1 or ((want[:, 0] == 0).any() and (want[:, 0] == 121).any())
    # the wrapper on a pitched view, with host points, with device points and the caller's table
    a = up16(np.pad(image, ((0, 0), (0, 3))))[:, :W]
    got = ops.patch_sharpness_u16(a, points, 5, 2, (44.0, 36.0, 30.0))
    assert got.dtype == torch.int64 and tuple(got.shape) == (n, 4) and np.array_equal(got.cpu().numpy().view(np.uint64), want)
    again = ops.patch_sharpness_u16(a, torch.from_numpy(points.astype(np.int32)).cuda(), 5, 2, (44.0, 36.0, 30.0), out=got.zero_())
    assert again is got and np.array_equal(got.cpu().numpy().view(np.uint64), want)
    none = ops.patch_sharpness_u16(a, points, 5, 2)
    assert np.array_equal(none.cpu().numpy().view(np.uint64), qr.patch_sharpness(image, points, 5, 2))
    for bad in (dict(half=0), dict(half=33), dict(arm=0), dict(arm=9)):
        with pytest.raises(ValueError):
            ops.patch_sharpness_u16(a, points, **dict(dict(half=5, arm=2), **bad))
    with pytest.raises(ValueError):
        ops.patch_sharpness_u16(a, points, 5, 2, out=got[:, :-1])
    with pytest.raises(ValueError):
        ops.patch_sharpness_u16(a, points.astype(np.int32).reshape(-1), 5, 2, out=torch.zeros((n, 4), dtype=torch.int32, device='cuda'))


def test_sharpness_of_small_images_of_the_largest_sums_and_of_a_constant(mods):
    _, _, lib = mods
    rng = np.random.default_rng(4)
    for shape, arm in (((6, 40), 3), ((40, 6), 3), ((2, 2), 1), ((16, 16), 8), ((1, 1), 1)):     # smaller than 2 D + 1 one way or both
        img = rng.integers(1, 65536, shape).astype(np.uint16)
        points = [(0, 0), (shape[0] // 2, shape[1] // 2), (shape[0] - 1, shape[1] - 1)]
        assert (check_sharpness(lib, img, points, 32, arm) == 0).all()
    board = ((np.add.outer(np.arange(90), np.arange(95)) % 2) * 65535).astype(np.uint16)          # 0 / 65535: at an odd arm |L| = 4 x 65535
    for arm in (1, 3, 7):
        want = check_sharpness(lib, board, [(44, 47), (45, 47)], 32, arm)
        assert (want[:, 0] == 4225).all() and (want[:, 3] == 4225 * 262140 ** 2).all()
        assert want[0, 1] == 2113 * 65535 and want[1, 1] == 2112 * 65535 and want[0, 2] == 2113 * 65535 ** 2
    assert (check_sharpness(lib, board, [(44, 47)], 32, 2)[:, 3] == 0).all()                     # an even arm sees equal pixels
    want = check_sharpness(lib, np.full((50, 45), 65535, np.uint16), [(25, 22), (2, 2)], 7, 3, (22.0, 25.0, 18.0))
    assert (want[:, 3] == 0).all() and want[0].tolist() == [225, 225 * 65535, 225 * 65535 ** 2, 0]


def test_sharpness_refusals_leave_the_table_untouched(mods, image):
    _, _, lib = mods
    points = [(35, 45), (3, 4)]
    for over, code in ((dict(h=0), E_UNSUPPORTED), (dict(w=16385), E_UNSUPPORTED), (dict(img_ptr=None), E_ARG), (dict(points_ptr=None), E_ARG),
                       (dict(table=None), E_ARG), (dict(pitch=W - 1), E_ARG), (dict(n=0), E_ARG), (dict(n=-2), E_ARG),
                       (dict(n=(1 << 23) + 1), E_ARG)):
        st, _, intact = sharpness(lib, image, points, 4, 2, **over)
        assert st == code and intact, over
    for half, arm in ((0, 2), (33, 2), (4, 0), (4, 9), (4, -1)):
        st, _, intact = sharpness(lib, image, points, half, arm)
        assert st == E_ARG and intact, (half, arm)
    for circle in ((float('nan'), 1.0, 5.0), (1.0, float('inf'), 5.0), (1.0, 1.0, float('nan'))):
        st, _, intact = sharpness(lib, image, points, 4, 2, circle)
        assert st == E_ARG and intact
    # a table on one of the inputs
    a = up16(image)
    pts = torch.from_numpy(np.array(points, np.int32)).cuda()
    for table in (a.data_ptr(), a.data_ptr() + 2 * (H * W - 1) - 6, pts.data_ptr()):
        assert lib.shg_patch_sharpness_u16(a.data_ptr(), W, H, W, pts.data_ptr(), 2, 4, 2, None, table, None) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(down16(a), image) and pts.cpu().numpy().tolist() == [list(p) for p in points]


# ---- weighted combine ----
@pytest.mark.parametrize('step', [8, 16])
@pytest.mark.parametrize('shape, layout', GRIDS, ids=['%dx%d_%s' % (g[0] + (g[1],)) for g in GRIDS])
def test_random_weights_match_the_restatement(mods, shape, layout, step):
    """The grids of test_align_gpu: partial last cells and nodes beyond the grid (37 x 263), the clamp's last row and column (64 x
    256), the 16-byte stores (aligned) and the stores by element; null and non-null fields and lattices mixed, and no field at all."""
    _, _, lib = mods
    how = LAYOUTS[layout]
    srcs, xforms = random_sources(5, [(70, 270), (66, 260)], step + shape[1], spread=2.0, scale=0.01)
    fields = random_fields(5, shape, step, 3 * step + shape[0], none=(1, 3))
    weights = random_weights(5, shape, step, 5 * step + shape[0], none=(0, 3))
    for mode, kappa, iterations in (('mean', 2.5, 2), ('sigma', 1.2, 1), ('sigma', 1.2, 3)):
        want, count = check_weighted(lib, srcs, xforms, shape, mode, kappa, iterations, fields=fields, weights=weights, step=step, **how)
    check_weighted(lib, srcs, xforms, shape, 'sigma', 1.2, 2, fields=None, weights=weights, step=step, **how)
    if shape[0] > 1:
        plain = ar.stack_combine_field(srcs, xforms, fields, step, shape, 'mean')[0]
        assert (qr.stack_combine_weighted(srcs, xforms, fields, weights, step, shape, 'mean')[0] != plain).mean() > 0.5    # the weights do something


@pytest.mark.parametrize('n', [3, 5, 9, 17, 32])
def test_every_capacity_and_the_three_properties_against_the_existing_kernels(mods, n):
    _, _, lib = mods
    shape, step = (20, 19), 8
    srcs, xforms = random_sources(n, [(23, 21), (19, 26)], 100 + n)
    fields = random_fields(n, shape, step, n, 2.0, none=(0, n - 2))
    weights = random_weights(n, shape, step, 200 + n, none=(1,))
    gh, gw = ar.lattice_shape(shape, step)
    ones, zeros = np.ones((gh, gw)), np.zeros((gh, gw))
    for mode, kappa, iterations in (('mean', 2.5, 2), ('sigma', 1.3, 1), ('sigma', 1.3, 3)):
        want, count = check_weighted(lib, srcs, xforms, shape, mode, kappa, iterations, fields=fields, weights=weights, step=step)
        assert count.max() <= n
        # (a) null lattices, or ones: shg_stack_combine_field_u16 itself
        st, field_out, field_count, intact = combine(lib, srcs, xforms, shape, fields, None, step, mode, kappa, iterations)
        assert st == 0 and intact
        for lattices in ([None] * n, [ones] * n, [ones if j % 2 else None for j in range(n)]):
            st, got, got_count, intact = combine(lib, srcs, xforms, shape, fields, lattices, step, mode, kappa, iterations)
            assert st == 0 and intact and np.array_equal(got, field_out) and np.array_equal(got_count, field_count)
        # (b) a lattice of zeros: the field combine (unit weights elsewhere) without that source
        for gone in (0, n // 2, n - 1):
            rest = [j for j in range(n) if j != gone]
            st, less, less_count, intact = combine(lib, [srcs[j] for j in rest], [xforms[j] for j in rest], shape, [fields[j] for j in rest],
                                                   None, step, mode, kappa, iterations)
            assert st == 0 and intact
            # (the padded buffers' pitches follow the position: the sources are the same images either way)
            st, got, got_count, intact = combine(lib, srcs, xforms, shape, fields, [zeros if j == gone else None for j in range(n)], step,
                                                 mode, kappa, iterations)
            assert st == 0 and intact and np.array_equal(got, less) and np.array_equal(got_count, less_count)
        # (c) a common power of two changes no bit (a null lattice is one of ones)
        for factor in (2.0 ** -3, 2.0 ** 4):
            st, got, got_count, intact = combine(lib, srcs, xforms, shape, fields, [factor * (ones if w is None else w) for w in weights], step,
                                                 mode, kappa, iterations)
            assert st == 0 and intact and np.array_equal(got, want) and np.array_equal(got_count, count)


def test_nan_negative_and_zero_nodes(mods):
    _, _, lib = mods
    img = np.random.default_rng(5).integers(0, 65536, (24, 40)).astype(np.uint16)
    shape, step = (24, 40), 8
    gh, gw = ar.lattice_shape(shape, step)
    assert (gh, gw) == (4, 6)
    for bad in (np.nan, -1.0e9, -np.inf):
        lattice = np.ones((gh, gw))
        lattice[1, 2] = bad                                                      # the node at (8, 16): the four cells around it
        for mode in ('mean', 'sigma'):
            want, count = check_weighted(lib, [img, img], [IDENTITY] * 2, shape, mode, fields=None, weights=[lattice, None], step=step, out_extra=0, count_extra=0)
            assert (count[16:, :] == 2).all() and (count[:, 24:] == 2).all() and (count[:, :8] == 2).all()
            # (a NaN, or a weight that is not > 0; on row 0 and column 8 of the cells the node has the share 0, yet 0 * nan and
            # 0 * inf are no numbers; a finite negative node leaves that rim to the other three nodes)
            lost = count[0:16, 8:24] == 1
            assert lost[1:, 1:].all() and (lost.all() if not np.isfinite(bad) else (~lost[0, :]).all() and (~lost[:, 0]).all())
            assert np.array_equal(want, img)
    # a pixel where every weight is 0: value 0, count 0; beside it the weights come back
    zero = np.ones((gh, gw))
    zero[:, :3] = 0.0
    for mode in ('mean', 'sigma'):
        want, count = check_weighted(lib, [img, img, img], [IDENTITY] * 3, shape, mode, fields=None, weights=[zero] * 3, step=step)
        assert (count[:, :17] == 0).all() and (want[:, :17] == 0).all() and (count[:, 17:] == 3).all() and np.array_equal(want[:, 17:], img[:, 17:])


def test_weighted_combine_refusals_leave_the_outputs_untouched(mods):
    _, _, lib = mods
    srcs, xforms = random_sources(2, [(20, 22)], 1)
    shape = (18, 20)
    fields, weights = random_fields(2, shape, 8, 4), random_weights(2, shape, 8, 6)

    def refused(code, step=8, mode='sigma', **over):
        st, _, _, intact = combine(lib, srcs, xforms, shape, fields, weights, step, mode, over.pop('kappa', 2.5), over.pop('iterations', 2), **over)
        assert st == code and intact, (step, mode, over)

    refused(E_ARG, mode='median')
    refused(E_ARG, mode=3)
    for step in (7, 129, 0, -8):
        refused(E_ARG, step)
    for over in (dict(gh=3), dict(gh=5), dict(gw=3), dict(gw=5), dict(no_weights=True), dict(out=None), dict(kappa=0.5), dict(iterations=0),
                 dict(iterations=4)):
        refused(E_ARG, **over)
    # an output or a count plane on a lattice, a lattice off 8 bytes, a field off 16 bytes
    lattice = torch.from_numpy(weights[0]).cuda()
    last = lattice.data_ptr() + lattice.numel() * 8 - 2
    for over in (dict(out=lattice.data_ptr()), dict(out=last), dict(count=lattice.data_ptr() + 64), dict(count=last + 1),
                 dict(weight_ptr={1: lattice.data_ptr() + 4}), dict(weight_ptr={1: lattice.data_ptr() + 2})):
        if 'weight_ptr' not in over:
            over['weight_ptr'] = {0: lattice.data_ptr()}
        refused(E_ARG, **over)
    field = torch.from_numpy(fields[0]).cuda()
    refused(E_ARG, field_ptr={0: field.data_ptr() + 8})
    refused(E_ARG, field_ptr={0: field.data_ptr()}, out=field.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(lattice.cpu().numpy()), bits(weights[0])) and np.array_equal(bits(field.cpu().numpy()), bits(fields[0]))


def test_ops_wrapper(mods):
    _, ops, _ = mods
    srcs, xforms = random_sources(3, [(30, 33), (28, 36)], 21)
    views = [up16(np.pad(s, ((0, 0), (0, 2))))[:, :s.shape[1]] for s in srcs]
    shape = (29, 31)
    fields, weights = random_fields(3, shape, 8, 9, none=(2,)), random_weights(3, shape, 8, 10, none=(0,))
    dev = [None if f is None else torch.from_numpy(f).cuda() for f in fields]
    dev_w = [None if w is None else torch.from_numpy(w).cuda() for w in weights]
    want, want_count = qr.stack_combine_weighted(srcs, xforms, fields, weights, 8, shape, 'sigma', 1.2, 2)
    out, count = ops.stack_combine_weighted_u16(views, xforms, dev, dev_w, 8, shape, 'sigma', 1.2, 2)
    assert out.dtype == torch.uint16 and count.dtype == torch.uint8
    assert np.array_equal(down16(out), want) and np.array_equal(count.cpu().numpy(), want_count)
    # the caller's pitched views; no field at all
    big, big_c = up16(np.zeros((29, 40))), torch.zeros((29, 37), dtype=torch.uint8, device='cuda')
    again, again_c = ops.stack_combine_weighted_u16(views, xforms, dev, dev_w, 8, shape, 'sigma', 1.2, 2, out=big[:, 3:34], count=big_c[:, 1:32])
    assert np.array_equal(down16(again), want) and np.array_equal(again_c.cpu().numpy(), want_count) and (down16(big)[:, :3] == 0).all()
    out, none = ops.stack_combine_weighted_u16(views, xforms, None, dev_w, 8, shape, 'mean', want_count=False)
    assert none is None and np.array_equal(down16(out), qr.stack_combine_weighted(srcs, xforms, None, weights, 8, shape, 'mean')[0])
    with pytest.raises(ValueError, match='weight'):
        ops.stack_combine_weighted_u16(views, xforms, dev, [None, dev_w[1][:-1], dev_w[2]], 8, shape)
    with pytest.raises(ValueError, match='weight'):
        ops.stack_combine_weighted_u16(views, xforms, dev, [None, dev_w[1].float(), dev_w[2]], 8, shape)
    with pytest.raises(ValueError, match='median'):
        ops.stack_combine_weighted_u16(views, xforms, dev, dev_w, 8, shape, 'median')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.stack_combine_weighted_u16(views, xforms, dev, [None, dev_w[1].cpu(), dev_w[2]], 8, shape)
    with pytest.raises(RuntimeError, match='kappa'):
        ops.stack_combine_weighted_u16(views, xforms, dev, dev_w, 8, shape, kappa=0.5)


# ---- end to end: the quadrant series ----
def same_maps(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None) and (w is None or (g.dtype == np.float64 and np.array_equal(bits(g), bits(w))))


def test_quality_maps_and_the_lucky_stack_on_the_quadrant_series(mods):
    stack, _, _ = mods
    images, circle, _ = qr.quadrant_series()
    dev = [up16(img) for img in images]
    for i in (0, 3):
        got, want = stack.disk_quality(dev[i], circle), qr.disk_quality(images[i], circle)
        same_maps([got['map']], [want['map']])
        assert got['quality'] == want['quality'] and got['nodes'] == want['nodes'] > 0
    got, want = stack.disk_quality(dev[1], circle, 24, 21, 1, 0.8), qr.disk_quality(images[1], circle, 24, 21, 1, 0.8)
    same_maps([got['map']], [want['map']])
    assert got['quality'] == want['quality']

    def stack_of(imgs, records, weights, step):
        out, count = stack.stack_disks(dev, records, 'mean', step=step, weights=weights)
        return down16(out), count.cpu().numpy()

    got = qr.quadrant_measures(lambda imgs, records, circles, reference: stack.local_quality(dev, records, circles, reference), stack_of)
    want = qr.restated_measures()
    print('on the GPU: %d nodes, the blurred frame last at %d; residual lucky %.6f, all %.6f counts; ratio %.6f' %
          (got['nodes'], got['last'], got['lucky'], got['all'], got['ratio']))
    same_maps(got['maps'], want['maps'])
    assert all(np.array_equal(a, b) for a, b in zip(got['weights'], want['weights']))
    assert np.array_equal(got['stack'], want['stack']) and np.array_equal(got['count'], want['count'])
    for key in ('nodes', 'last', 'lucky', 'all', 'ratio'):
        assert got[key] == want[key], key
    assert got['last'] == got['nodes'] == 72 and got['ratio'] < 1.0 and got['ratio'] <= qr.TOLERANCE['lucky']
    # with transforms and fields: the points move with the scan; a rejected scan has no map
    series, _, given = ar.synthetic_series()
    records = sr.register_disks(series, given)
    fields, _ = ar.local_fields(series, records, given)
    sdev = [up16(img) for img in series]
    for f in (None, fields, [None if t is None else torch.from_numpy(t).cuda() for t in fields]):
        host = None if f is None else fields
        same_maps(stack.local_quality(sdev, records, given, 0, f, 16, 33, 3, 0.9), qr.local_quality(series, records, given, 0, host, 16, 33, 3, 0.9))
    records[2] = dict(records[2], rejected=True)
    assert stack.local_quality(sdev, records, given, 0)[2] is None
    # weights with fields through stack_disks, sigma, weighted by quality
    records = sr.register_disks(series, given)
    maps = qr.local_quality(series, records, given, 0, fields)
    weights = qr.quality_weights(maps, 2, 1.5)
    rows = [(r['s'], r['tx'], r['ty'], r['gain']) for r in records]
    out, count = stack.stack_disks(sdev, records, 'sigma', 1.0, 2, fields=[None if t is None else torch.from_numpy(t).cuda() for t in fields],
                                   step=16, weights=weights)
    want, want_count = qr.stack_combine_weighted(series, rows, fields, weights, 16, series[0].shape, 'sigma', 1.0, 2)
    assert np.array_equal(down16(out), want) and np.array_equal(count.cpu().numpy(), want_count)
    with pytest.raises(ValueError, match='median'):
        stack.stack_disks(sdev, records, 'median', step=16, weights=weights)
    with pytest.raises(ValueError, match='lattice'):
        stack.stack_disks(sdev, records, 'mean', step=16, weights=[w * np.nan for w in weights])


# ---- end to end: three scans ----
LOCAL = {'step': 32, 'size': 25, 'search': 3}


@pytest.fixture(scope='module')
def scans(mods, tmp_path_factory):
    stack = mods[0]
    paths = [write_scan(tmp_path_factory, 'quality%d' % i, frames) for i, frames in enumerate(sr.pipeline_series())]
    return {'paths': paths, 'plain': stack.stack_scans(paths), 'lucky': stack.stack_scans(paths, quality={'lucky': 2}),
            'both': stack.stack_scans(paths, local=LOCAL, quality={'lucky': 2, 'power': 1.0}, reference='best')}


def check_result(res, want, n=3):
    same_records(res['records'], want['records'])
    assert res['reference'] == want['reference'] and res['used'] == want['used'] and res['unselected'] == want['unselected']
    assert res['rejected'] == [i for i in range(n) if i not in want['used']]
    q = res['quality']
    assert q['figures'] == want['figures'] and q['selected'] == [i in want['used'] for i in range(n)]
    same_maps(q['maps'], want['maps'])
    if want['weights'] is None:
        assert q['weights'] is None and q['shares'] is None
    else:
        assert all(np.array_equal(q['weights'][i], w) for i, w in zip(want['used'], want['weights']))
        assert [q['shares'][i] for i in want['used']] == want['shares']
    assert np.array_equal(down16(res['stack']), want['stack']) and np.array_equal(res['count'].cpu().numpy(), want['count'])


def test_stack_scans_with_quality_is_the_restatement_of_its_disks(mods, scans):
    stack = mods[0]
    res = scans['lucky']
    images, circles = [down16(t) for t in res['images']], res['circles']
    check_result(res, qr.stack_series(images, circles, quality={'lucky': 2}))
    assert {k: res['quality'][k] for k in qr.DEFAULTS} == dict(qr.DEFAULTS, lucky=2) and res['local'] is None
    # (two of three where the four nodes around a pixel keep the same pair, three where they differ or have no figure)
    assert res['count'].cpu().numpy().max() == 3 and (res['count'].cpu().numpy() == 2).any()
    assert (down16(res['stack']) != down16(scans['plain']['stack'])).any()
    res = scans['both']
    want = qr.stack_series(images, circles, 'best', local=LOCAL, quality={'lucky': 2, 'power': 1.0})
    check_result(res, want)
    assert res['quality']['step'] == 32 and res['reference'] == max(range(3), key=lambda i: (want['figures'][i], -i))
    same_fields(res['local']['fields'], ar.local_fields(images, want['records'], circles, want['reference'], **dict(ar.DEFAULTS, **LOCAL))[0])
    # the selection: the two best of three, and a threshold that keeps all
    res = stack.stack_scans(scans['paths'], quality={'best': 2})
    want = qr.stack_series(images, circles, quality={'best': 2})
    check_result(res, want)
    assert len(res['used']) == 2 and len(res['unselected']) == 1 and res['count'].cpu().numpy().max() == 2
    res = stack.stack_scans(scans['paths'], quality={'min_quality': 0.5, 'arm': 2, 'size': 21, 'step': 24})
    check_result(res, qr.stack_series(images, circles, quality={'min_quality': 0.5, 'arm': 2, 'size': 21, 'step': 24}))
    assert len(set(res['quality']['figures'])) == 3
    with pytest.raises(ValueError, match='nothing to stack'):
        stack.stack_scans(scans['paths'], quality={'min_quality': 1.0})


def test_without_quality_everything_is_what_it_was(mods, scans, tmp_path, capsys):
    """No `quality` argument and an integer reference: the stack, the count and the records are stack_ref's, as before, and the new
    keys say nothing; no new flag: the JSON line has the keys it had."""
    stack = mods[0]
    plain = scans['plain']
    assert plain['quality'] is None and plain['unselected'] == [] and plain['local'] is None and plain['reference'] == 0
    want, want_count, want_records = sr.stack_series([down16(t) for t in plain['images']], plain['circles'])
    same_records(plain['records'], want_records)
    assert np.array_equal(down16(plain['stack']), want) and np.array_equal(plain['count'].cpu().numpy(), want_count)
    res = stack.stack_scans(scans['paths'], reference=1, mode='median', local=LOCAL)
    want, want_count, want_records, want_fields, _ = ar.stack_series([down16(t) for t in res['images']], res['circles'], 1, 'median', local=LOCAL)
    same_records(res['records'], want_records)
    same_fields(res['local']['fields'], want_fields)
    assert np.array_equal(down16(res['stack']), want) and np.array_equal(res['count'].cpu().numpy(), want_count) and res['quality'] is None
    work = []
    for i, path in enumerate(scans['paths']):
        work.append(str(tmp_path / ('scan%d.ser' % i)))
        shutil.copy(path, work[-1])
    out = run_json(stack.main, capsys, work)
    assert sorted(out) == sorted(['shape', 'mode', 'kappa', 'iterations', 'shift', 'reference', 'files', 'rejected', 'frames', 'png', 'fits',
                                  'count_png', 'circle', 'ratio', 'phi', 'crop'])
    assert all(sorted(frame) == ['file', 'gain', 'offset', 'rejected', 'rms', 'scale'] for frame in out['frames']) and out['reference'] == 0


def test_command_line_with_the_quality_flags(mods, scans, tmp_path, capsys):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.png_io import read_png_gray
    stack = mods[0]
    work = []
    for i, path in enumerate(scans['paths']):
        work.append(str(tmp_path / ('scan%d.ser' % i)))
        shutil.copy(path, work[-1])
    k = SHG_MAIN.default_options()['img_rotate'] // 90
    base = work[0][:-4] + '_shift=0_stack'
    figures = scans['lucky']['quality']['figures']
    # --quality: measured and reported, the stack the usual one
    out = run_json(stack.main, capsys, work + ['--quality'])
    assert out['png'] == base + '.png' and [frame['quality'] for frame in out['frames']] == figures
    assert out['quality']['arm'] == 3 and out['quality']['shares'] is None and out['quality']['reference'] == 0 and out['rejected'] == []
    assert np.array_equal(read_png_gray(out['png']), np.rot90(down16(scans['plain']['stack']), k))
    # --best 2
    out = run_json(stack.main, capsys, work + ['--best', '2'])
    worst = min(range(3), key=lambda i: (figures[i], i))
    assert out['rejected'] == [work[worst]] == out['quality']['unselected'] and len(out['files']) == 2 and len(out['frames']) == 3
    assert not out['frames'][worst]['rejected'] and out['frames'][worst]['quality'] == figures[worst]
    # --lucky 2 --coverage: the count plane shows the kept scans
    out = run_json(stack.main, capsys, work + ['--lucky', '2', '--coverage'])
    assert out['png'] == base + '.png' and out['count_png'] == base + '_count.png' and out['quality']['lucky'] == 2
    assert np.array_equal(read_png_gray(out['png']), np.rot90(down16(scans['lucky']['stack']), k))
    assert np.array_equal(read_png_gray(out['count_png']), np.rot90(scans['lucky']['count'].cpu().numpy(), k))
    assert out['quality']['shares'] == scans['lucky']['quality']['shares'] and abs(sum(out['quality']['shares']) - 1.0) < 1e-12
    # --reference best with the local alignment and a power
    out = run_json(stack.main, capsys, work + ['--reference', 'best', '--lucky', '2', '--quality-power', '1', '--local', '--ap-step', '32',
                                               '--ap-size', '25', '--ap-search', '3'])
    best = scans['both']['reference']
    assert out['reference'] == best == out['quality']['reference'] and out['png'] == work[best][:-4] + '_shift=0_stack.png'
    assert out['quality']['step'] == 32 and out['quality']['power'] == 1.0
    assert np.array_equal(read_png_gray(out['png']), np.rot90(down16(scans['both']['stack']), k))
