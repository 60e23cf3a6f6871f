"""The quality ranking without a GPU: the restatement's exact properties, the host steps of solex_ser_recon_en_amd/stack.py against
hand-computed cases and against the restatement, the accuracy on the quadrant series, and the refusals that come before any
device work."""
import ctypes

import numpy as np
import pytest

from tests import align_ref as ar
from tests import quality_ref as qr
from tests import stack_ref as sr

E_ARG, E_UNSUPPORTED = -1, -3
IDENTITY = (1.0, 0.0, 0.0, 1.0)


def test_error_codes_are_the_headers():
    import re
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'shg_hip.h')).read()
    assert int(re.search(r'#define\s+SHG_E_ARG\s+\(?(-?\d+)', text).group(1)) == E_ARG
    assert int(re.search(r'#define\s+SHG_E_UNSUPPORTED\s+\(?(-?\d+)', text).group(1)) == E_UNSUPPORTED


# ---- the restatement ----
def test_patch_sharpness_by_hand():
    img = np.zeros((9, 11), dtype=np.uint16)
    img[4, 5] = 10
    # arm 1, half 1 around (4, 5): the 3 x 3 set sees L = 40 at the centre, -10 at the four neighbours, 0 at the corners
    assert qr.patch_sharpness(img, [(4, 5)], 1, 1).tolist() == [[9, 10, 100, 1600 + 4 * 100]]
    # arm 2: the neighbours at distance 1 see nothing of the centre
    assert qr.patch_sharpness(img, [(4, 5)], 1, 2).tolist() == [[9, 10, 100, 1600]]
    # a corner centre: the set is cut to the pixels at least D from every edge; outside: empty; a circle that cuts
    assert qr.patch_sharpness(img, [(0, 0)], 1, 1).tolist() == [[1, 0, 0, 0]]
    assert qr.patch_sharpness(img, [(-5, 3), (2 ** 31 - 1, -2 ** 31)], 2, 1).tolist() == [[0] * 4] * 2
    assert qr.patch_sharpness(img, [(4, 5)], 1, 1, (5.0, 4.0, 1.0)).tolist() == [[5, 10, 100, 1600 + 4 * 100]]
    assert qr.patch_sharpness(img, [(4, 5)], 1, 1, (-1, -1, -1)).tolist() == [[9, 10, 100, 2000]]
    assert qr.patch_sharpness(np.full((2, 9), 7, np.uint16), [(1, 4)], 3, 1).tolist() == [[0] * 4]


def _random_case(seed, n=4, shape=(21, 26), step=8):
    rng = np.random.default_rng(seed)
    srcs = [rng.integers(0, 65536, (shape[0] + 3, shape[1] + 2), dtype=np.uint16) for _ in range(n)]
    xforms = [(1.0 + 0.01 * rng.standard_normal(), rng.uniform(0, 2), rng.uniform(0, 2), rng.uniform(0.8, 1.2)) for _ in range(n)]
    gh, gw = ar.lattice_shape(shape, step)
    fields = [None if k % 2 else rng.uniform(-1, 1, (gh, gw, 2)) for k in range(n)]
    weights = [rng.uniform(0.0, 2.0, (gh, gw)) for _ in range(n)]
    return srcs, xforms, fields, weights, shape, step


@pytest.mark.parametrize('mode, kappa, iterations', [('mean', 2.5, 2), ('sigma', 1.0, 1), ('sigma', 1.1, 3)])
def test_restatement_properties(mode, kappa, iterations):
    srcs, xforms, fields, weights, shape, step = _random_case(5, n=5)
    gh, gw = ar.lattice_shape(shape, step)
    want = ar.stack_combine_field(srcs, xforms, fields, step, shape, mode, kappa, iterations)
    # (a) no lattice, or ones: the field combine
    for lattices in ([None] * 5, [np.ones((gh, gw))] * 5, [None, np.ones((gh, gw))] * 2 + [None]):
        got = qr.stack_combine_weighted(srcs, xforms, fields, lattices, step, shape, mode, kappa, iterations)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # (b) a lattice of zeros removes its source
    for gone in (0, 2, 4):
        lattices = [np.zeros((gh, gw)) if k == gone else w for k, w in enumerate(weights)]
        rest = [k for k in range(5) if k != gone]
        got = qr.stack_combine_weighted(srcs, xforms, fields, lattices, step, shape, mode, kappa, iterations)
        less = qr.stack_combine_weighted([srcs[k] for k in rest], [xforms[k] for k in rest], [fields[k] for k in rest],
                                         [weights[k] for k in rest], step, shape, mode, kappa, iterations)
        assert np.array_equal(got[0], less[0]) and np.array_equal(got[1], less[1])
    # (c) a common power of two changes no bit
    base = qr.stack_combine_weighted(srcs, xforms, fields, weights, step, shape, mode, kappa, iterations)
    assert not np.array_equal(base[0], want[0])                      # (the weights do something)
    for factor in (2.0 ** -3, 2.0 ** 4):
        got = qr.stack_combine_weighted(srcs, xforms, fields, [w * factor for w in weights], step, shape, mode, kappa, iterations)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


def test_weighted_restatement_by_hand():
    """Two constant sources of 100 and 200 on a lattice of one cell (nodes at columns 0 and 8): weights 1 -> 3 along x for the first, 1
    for the second."""
    shape, step = (1, 9), 8
    srcs = [np.full((1, 9), 100, np.uint16), np.full((1, 9), 200, np.uint16)]
    w0 = np.array([[1.0, 3.0]])
    out, count = qr.stack_combine_weighted(srcs, [IDENTITY] * 2, None, [w0, None], step, shape, 'mean')
    for c in range(9):
        w = 1.0 + 2.0 * (c / 8.0)
        assert out[0, c] == int(np.rint((w * 100.0 + 200.0) / (w + 1.0))) and count[0, c] == 2
    # a node that is not a number takes the source out of its cells whatever its share (nan * 0 is not a number), a negative one
    # where the interpolated weight is not > 0; all-zero: nothing
    out, count = qr.stack_combine_weighted(srcs, [IDENTITY] * 2, None, [np.array([[1.0, np.nan]]), None], step, shape, 'mean')
    assert count[0].tolist() == [1] * 9 and (out[0] == 200).all()
    out, count = qr.stack_combine_weighted(srcs, [IDENTITY] * 2, None, [np.array([[1.0, -1.0]]), None], step, shape, 'mean')
    assert count[0].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1]           # 1 - 2 c / 8 > 0 for c < 4
    out, count = qr.stack_combine_weighted(srcs, [IDENTITY] * 2, None, [np.zeros((1, 2)), np.zeros((1, 2))], step, shape, 'sigma')
    assert not out.any() and not count.any()


# ---- the host steps against hand-computed cases and the restatement ----
def test_patch_quality_by_hand():
    from solex_ser_recon_en_amd import stack
    table = np.array([[9, 90, 1000, 360], [4, 90, 1000, 360], [5, 90, 1000, 360], [9, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int64)
    q = stack.patch_quality(table, 1)
    assert q[0] == (360.0 * 9.0) / (90.0 * 90.0) and q[2] == (360.0 * 5.0) / 8100.0                # 2 x 5 >= 9; 2 x 4 < 9
    assert np.isnan(q[[1, 3, 4]]).all()
    big = np.array([[4225, 4225 * 65535, 0, 4225 * 262140 ** 2]], dtype=np.uint64)
    assert stack.patch_quality(big, 32)[0] == (float(4225 * 262140 ** 2) * 4225.0) / (float(4225 * 65535) * float(4225 * 65535))
    rng = np.random.default_rng(2)
    table = rng.integers(0, 2 ** 40, (50, 4))
    table[:, 0] = rng.integers(0, 1090, 50)
    assert np.array_equal(stack.patch_quality(table, 16), qr.patch_quality(table, 16), equal_nan=True)


def test_quality_weights_by_hand():
    from solex_ser_recon_en_amd import stack
    nan = np.nan
    #                 tie      NaN last   one valid   all NaN   zero best
    maps = [np.array([[2.0,    nan,       nan,        nan,      0.0]]),
            np.array([[2.0,    1.0,       nan,        nan,      0.0]]),
            np.array([[1.0,    4.0,       3.0,        nan,      nan]])]
    assert [w.tolist() for w in stack.quality_weights(maps)] == [[[1.0] * 5]] * 3                   # keep None keeps all
    assert [w.tolist() for w in stack.quality_weights(maps, 1)] == [[[1, 0, 0, 1, 1]], [[0, 0, 0, 1, 0]], [[0, 1, 1, 1, 0]]]
    assert [w.tolist() for w in stack.quality_weights(maps, 2)] == [[[1, 0, 1, 1, 1]], [[1, 1, 0, 1, 1]], [[0, 1, 1, 1, 0]]]
    got = stack.quality_weights(maps, None, 2.0)
    assert got[0].tolist() == [[1.0, 0.0, 0.0, 1.0, 1.0]] and got[1].tolist() == [[1.0, 0.0625, 0.0, 1.0, 1.0]]
    assert got[2].tolist() == [[0.25, 1.0, 1.0, 1.0, 1.0]]
    assert stack.quality_weights(maps, 2, 0.5)[2].tolist() == [[0.0, 1.0, 1.0, 1.0, 0.0]]
    assert stack.node_shares(maps) == [0.5, 0.0, 0.5]
    rng = np.random.default_rng(3)
    maps = [np.where(rng.random((6, 7)) < 0.2, nan, np.round(rng.random((6, 7)), 1)) for _ in range(5)]
    for keep, power in ((None, 0.0), (1, 0.0), (3, 0.0), (2, 1.5), (None, 0.5), (7, 2.0)):
        assert all(np.array_equal(a, b) for a, b in zip(stack.quality_weights(maps, keep, power), qr.quality_weights(maps, keep, power)))
    assert stack.node_shares(maps) == qr.node_shares(maps)
    for bad in (dict(keep=0), dict(power=-1.0), dict(power=nan)):
        with pytest.raises(ValueError):
            stack.quality_weights(maps, **bad)


def test_select_scans_by_hand():
    from solex_ser_recon_en_amd import stack
    q = [0.5, 0.9, 0.7, 0.9, 0.1]
    assert stack.select_scans(q) == [0, 1, 2, 3, 4]
    assert stack.select_scans(q, best=2) == [1, 3] and stack.select_scans(q, best=3) == [1, 2, 3] and stack.select_scans(q, best=9) == [0, 1, 2, 3, 4]
    assert stack.select_scans(q, min_quality=0.7) == [1, 2, 3] and stack.select_scans(q, min_quality=0.0) == [0, 1, 2, 3, 4]
    assert stack.select_scans(q, best=2, min_quality=0.5) == [1, 3]
    assert stack.select_scans([1.0, 1.0, 1.0], best=2) == [0, 1]                                    # ties to the lower index
    for bad in (dict(best=1), dict(best=0)):
        with pytest.raises(ValueError):
            stack.select_scans(q, **bad)
    with pytest.raises(ValueError, match='nothing to stack'):
        stack.select_scans([1.0, 0.2, 0.1], min_quality=0.5)
    with pytest.raises(ValueError):
        stack.select_scans([1.0], best=2)
    for kw in (dict(best=2), dict(min_quality=0.6), dict(best=3, min_quality=0.2)):
        assert stack.select_scans(q, **kw) == qr.select_scans(q, **kw)


def test_check_weights():
    from solex_ser_recon_en_amd import stack
    ok = np.ones((3, 4))
    assert stack.check_weights([ok, None], (3, 4))[1] is None
    for bad in (np.ones((4, 3)), ok * np.nan, -ok, ok * 2.0 ** 21, np.where(np.eye(3, 4) > 0, np.inf, 1.0)):
        with pytest.raises(ValueError):
            stack.check_weights([bad], (3, 4))
    assert stack.check_weights([ok * 2.0 ** 20, ok * 0.0], (3, 4))[0].dtype == np.float64


# ---- the accuracy on the quadrant series ----
def test_accuracy_on_the_quadrant_series():
    m = qr.restated_measures()
    print('quadrant series: %d nodes, the blurred frame last at %d; residual lucky %.6f, all %.6f, frame %.6f counts; ratio %.6f (bound %.2f)'
          % (m['nodes'], m['last'], m['lucky'], m['all'], m['frame'], m['ratio'], qr.TOLERANCE['lucky']))
    assert m['nodes'] == 72
    assert m['last'] == m['nodes']                                   # a condition, not a tolerance
    assert m['ratio'] < 1.0
    assert m['ratio'] <= qr.TOLERANCE['lucky']
    counts = np.bincount(m['count'].ravel(), minlength=5)
    assert counts[:3].sum() == 0 and counts[3] > 0 and counts[4] > 0          # three of four on the disk, all four at the limb and the sky


def test_the_quadrant_series_is_what_it_claims():
    images, circle, model = qr.quadrant_series()
    assert len(images) == 4 and all(img.shape == (260, 250) and img.dtype == np.uint16 for img in images)
    assert circle == sr.series_circle(0) and np.array_equal(model, ar.frame_model(0) * 65535.0)
    assert qr.quadrant_of([0, 0, 259, 259], [0, 249, 0, 249], circle).tolist() == [0, 1, 2, 3]
    figures = [qr.disk_quality(img, circle)['quality'] for img in images]
    assert max(figures) / min(figures) < 1.1                         # globally the four are alike: only the map tells them apart


def test_arm_three_separates_texture_from_noise():
    """What DESIGN section 21 says of the arm: on align_ref's series the figures at arm 1 follow the gain, at arm 3 the texture."""
    images, _, given = ar.synthetic_series()
    one = [qr.disk_quality(img, c, arm=1)['quality'] for img, c in zip(images, given)]
    three = [qr.disk_quality(img, c, arm=3)['quality'] for img, c in zip(images, given)]
    print('median node quality, arm 1: %s; arm 3: %s' % (', '.join('%.5f' % t for t in one), ', '.join('%.5f' % t for t in three)))
    assert max(one) / min(one) > 1.5 and max(three) / min(three) < 1.1


# ---- the C ABI without a device ----
def test_quality_calls_refuse_bad_arguments_before_any_device_work():
    """Every refusal comes before the first HIP call: made-up addresses are never touched."""
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    p, pts, out = (ctypes.c_void_p(v) for v in (4096, 1 << 16, 1 << 20))
    ok = (ctypes.c_double * 3)(10.0, 10.0, 4.5)
    nan, inf = float('nan'), float('inf')

    def sharp(img=p, pitch=20, h=20, w=20, points=pts, n=5, b=4, d=2, c3=ok, table=out):
        return lib.shg_patch_sharpness_u16(img, pitch, h, w, points, n, b, d, c3, table, None)

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385, pitch=16385)):
        assert sharp(**over) == E_UNSUPPORTED, over
    for over in (dict(img=None), dict(points=None), dict(table=None), dict(pitch=19), dict(n=0), dict(n=-1), dict(n=(1 << 23) + 1),
                 dict(b=0), dict(b=33), dict(d=0), dict(d=9), dict(d=-1), dict(c3=(ctypes.c_double * 3)(nan, 10.0, 4.5)),
                 dict(c3=(ctypes.c_double * 3)(10.0, 10.0, inf)), dict(table=ctypes.c_void_p(4096 + 2 * (19 * 20 + 19))),
                 dict(table=ctypes.c_void_p(4096 - 8 * 5 * 4 + 8)), dict(table=ctypes.c_void_p((1 << 16) + 4 * 9))):
        assert sharp(**over) == E_ARG, over
    assert 'overlaps' in _lib.last_error()

    cnt, field, weight = ctypes.c_void_p(1 << 21), 1 << 22, 1 << 23

    def combine(n=2, dims=(20, 20, 20), xform=IDENTITY, fields=(field, None), weights=(None, weight), gh=4, gw=4, step=8, mode=2, kappa=2.5,
                iterations=2, out=out, oh=20, ow=20, out_pitch=20, count=cnt, count_pitch=20, have_fields=True, have_weights=True,
                have_srcs=True):
        ptrs = (ctypes.c_void_p * 32)(*([4096] * 32))
        d = (ctypes.c_int64 * 96)(*(list(dims) * 32))
        x = (ctypes.c_double * 128)(*(list(xform) * 32))
        f = (ctypes.c_void_p * 32)(*(list(fields) + [None] * (32 - len(fields))))
        w = (ctypes.c_void_p * 32)(*(list(weights) + [None] * (32 - len(weights))))
        return lib.shg_stack_combine_weighted_u16(ptrs if have_srcs else None, d, x, f if have_fields else None, w if have_weights else None,
                                                  gh, gw, step, n, mode, kappa, iterations, out, oh, ow, out_pitch, count, count_pitch, None)

    for over in (dict(oh=0), dict(dims=(0, 20, 20))):
        assert combine(**over) == E_UNSUPPORTED, over
    for over in (dict(have_weights=False), dict(have_srcs=False), dict(mode=1), dict(mode=3), dict(step=7), dict(step=129), dict(gh=3),
                 dict(gw=5), dict(n=0), dict(n=33), dict(out=None), dict(out_pitch=19), dict(kappa=0.5), dict(iterations=4),
                 dict(xform=(1.0, nan, 0.0, 1.0)), dict(fields=(field + 8, None)), dict(weights=(None, weight + 4)),
                 dict(weights=(weight + 2, None)), dict(out=ctypes.c_void_p(field)), dict(have_fields=False, mode=1),
                 dict(out=ctypes.c_void_p(weight)), dict(out=ctypes.c_void_p(weight + 8 * 16 - 2)),
                 dict(out=ctypes.c_void_p(weight - 2 * (19 * 20 + 19))), dict(count=ctypes.c_void_p(weight + 8)),
                 dict(weights=(weight, None), count=ctypes.c_void_p(weight + 127))):
        assert combine(**over) == E_ARG, over
    assert 'overlaps' in _lib.last_error()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from solex_ser_recon_en_amd import ops
    img = torch.zeros((8, 8), dtype=torch.uint16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.patch_sharpness_u16(img, [(4, 4)], 2, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.stack_combine_weighted_u16([img], [IDENTITY], None, [None], 8, (8, 8))
    with pytest.raises(ValueError, match='mode'):
        ops.stack_combine_weighted_u16([img], [IDENTITY], None, [None], 8, (8, 8), mode='best')
    with pytest.raises(ValueError, match='median'):
        ops.stack_combine_weighted_u16([img], [IDENTITY], None, [None], 8, (8, 8), mode='median')
    with pytest.raises(ValueError, match='weight'):
        ops.stack_combine_weighted_u16([img, img], [IDENTITY] * 2, None, [None], 8, (8, 8))
    with pytest.raises(ValueError, match='step'):
        ops.stack_combine_weighted_u16([img], [IDENTITY], None, [None], 4, (8, 8))


# ---- stack_scans', stack_disks' and the command line's refusals ----
def test_stack_scans_refuses_a_bad_quality():
    from solex_ser_recon_en_amd import stack
    two = ['no-such-a.ser', 'no-such-b.ser']
    for quality in (dict(step=4), dict(step=129), dict(size=34), dict(size=67), dict(arm=0), dict(arm=9), dict(best=1), dict(min_quality=1.5),
                    dict(lucky=0), dict(power=-1.0), dict(sharpness=3)):
        with pytest.raises(ValueError):
            stack.stack_scans(two, quality=quality)
    with pytest.raises(ValueError, match='local'):
        stack.stack_scans(two, local={}, quality=dict(step=16))
    for quality in (dict(lucky=2), dict(power=1.0)):
        with pytest.raises(ValueError, match='median'):
            stack.stack_scans(two, mode='median', quality=quality)
    with pytest.raises(ValueError, match='reference'):
        stack.stack_scans(two, reference='worst')
    with pytest.raises(ValueError, match='median'):
        stack.stack_disks([], [], mode='median', step=16, weights=[])
    with pytest.raises(ValueError, match='step'):
        stack.stack_disks([], [], weights=[])


@pytest.mark.parametrize('argv, message', [
    (['a.ser', 'b.ser', '--lucky', '2', '--mode', 'median'], 'weighted median'),
    (['a.ser', 'b.ser', '--quality-power', '1', '--mode', 'median'], 'weighted median'),
    (['a.ser', 'b.ser', '--quality-step', '16', '--local'], '--quality-step cannot be given with --local'),
    (['a.ser', 'b.ser', '--best', '1'], '--best'),
    (['a.ser', 'b.ser', '--quality-arm', '0'], '--quality-arm'),
    (['a.ser', 'b.ser', '--quality-arm', '9'], '--quality-arm'),
    (['a.ser', 'b.ser', '--quality-size', '32'], '--quality-size'),
    (['a.ser', 'b.ser', '--quality-size', '1'], '--quality-size'),
    (['a.ser', 'b.ser', '--quality-size', '67'], '--quality-size'),
    (['a.ser', 'b.ser', '--quality-step', '7'], '--quality-step'),
    (['a.ser', 'b.ser', '--quality-step', '129'], '--quality-step'),
    (['a.ser', 'b.ser', '--min-quality', '1.5'], '--min-quality'),
    (['a.ser', 'b.ser', '--lucky', '0'], '--lucky'),
    (['a.ser', 'b.ser', '--quality-power', '-1'], '--quality-power'),
    (['a.ser', 'b.ser', '--reference', 'worst'], '--reference'),
    (['a.ser', 'b.ser', '--reference', 'best', '--lucky', '2', '--quality-arm', '8', '--quality-size', '65', '--quality-step', '128'],
     'no such file'),
])
def test_command_line_refusals(monkeypatch, capsys, argv, message):
    from solex_ser_recon_en_amd import stack
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(SystemExit) as exit_info:
        stack.main(argv)
    assert exit_info.value.code == 2
    assert message in capsys.readouterr().err
