"""Stacking a series of scans, without a GPU: the restatement (tests/stack_ref.py) against hand-worked cases, the parabola
refinement on known quadratics, the host registration step of stack.py against its restatement bit for bit, a disk resampled by a
known transform registering back to it, the accuracy on a series of five synthetic disks -- re-measured here, printed, and held to
stack_ref.TOLERANCE --, the argument refusals of the two entry points that need no device, and the refusals of stack_scans and of
the command line."""
import ctypes

import numpy as np
import pytest

from tests import flatten_ref as fr
from tests import stack_ref as sr

E_ARG, E_UNSUPPORTED = -1, -3
IDENTITY = (1.0, 0.0, 0.0, 1.0)


# ---- the restatement against hand-worked cases ----
@pytest.mark.parametrize('mode', ['mean', 'median', 'sigma'])
@pytest.mark.parametrize('n', [1, 2, 3, 5])
def test_identity_transforms_return_the_image(mode, n):
    img = np.random.default_rng(n).integers(0, 65536, (9, 13)).astype(np.uint16)
    out, count = sr.stack_combine([img] * n, [IDENTITY] * n, img.shape, mode)
    assert out.dtype == np.uint16 and count.dtype == np.uint8
    assert np.array_equal(out, img) and (count == n).all()


def test_a_half_pixel_shift_rounds_ties_to_even():
    """One row (0, 1, 2) read half a pixel to the right: 0.5 -> 0, 1.5 -> 2, and 2.5 lies beyond the last column: absent."""
    src = np.array([[0, 1, 2]], np.uint16)
    out, count = sr.stack_combine([src], [(1.0, 0.5, 0.0, 1.0)], (1, 3), 'mean')
    assert out.tolist() == [[0, 2, 0]] and count.tolist() == [[1, 1, 0]]
    out, count = sr.stack_combine([src.T.copy()], [(1.0, 0.0, 0.5, 1.0)], (3, 1), 'mean')           # the same down a column
    assert out.ravel().tolist() == [0, 2, 0] and count.ravel().tolist() == [1, 1, 0]


def test_the_last_column_is_present_and_clamps_its_neighbour():
    src = np.array([[10, 20, 30], [40, 50, 60]], np.uint16)
    out, count = sr.stack_combine([src], [(1.0, 2.0, 1.0, 1.0)], (1, 2), 'mean')                    # sx = 2 = w - 1, sy = 1 = h - 1
    assert out.tolist() == [[60, 0]] and count.tolist() == [[1, 0]]
    below = (1.0, np.nextafter(0.0, -1.0), 0.0, 1.0)
    assert sr.stack_combine([src], [below], (1, 1), 'mean')[1].tolist() == [[0]]
    above = (1.0, np.nextafter(2.0, 3.0), 0.0, 1.0)
    assert sr.stack_combine([src], [above], (1, 1), 'mean')[1].tolist() == [[0]]


def _pixel(values, mode, kappa=2.5, iterations=2, present=None):
    v = np.array(values, dtype=np.float64)[:, None]
    p = np.ones(v.shape, bool) if present is None else np.array(present, bool)[:, None]
    m, count = sr.combine_samples(p, v, sr.MODES[mode], kappa, iterations)
    return float(m[0]), int(count[0])


def test_median_of_odd_and_even_counts():
    assert _pixel([5.0, 1.0, 9.0], 'median') == (5.0, 3)
    assert _pixel([5.0, 1.0, 9.0, 7.0], 'median') == (6.0, 4)
    assert _pixel([4.0], 'median') == (4.0, 1)
    assert _pixel([4.0, 100.0, 9.0], 'median', present=[True, False, True]) == (6.5, 2)            # the absent sample is no sample
    assert _pixel([4.0, 100.0, 9.0], 'median', present=[False, False, False]) == (0.0, 0)


def test_sigma_rejects_one_planted_outlier_of_five():
    """Among five samples none deviates by more than 4 / sqrt(5) = 1.79 standard deviations: kappa = 2.5 keeps all, 1.5 rejects the
    outlier; a second pass, on the four that are left, takes 98 as well (2.25 from their mean against a limit of 2.22), a third
    finds nothing more."""
    values = [100.0, 102.0, 98.0, 101.0, 500.0]
    assert _pixel(values, 'sigma', 2.5) == (sum(values) / 5.0, 5)
    assert _pixel(values, 'sigma', 1.5, 1) == (100.25, 4)
    assert _pixel(values, 'sigma', 1.5, 2) == (101.0, 3) and _pixel(values, 'sigma', 1.5, 3) == (101.0, 3)
    # two outliers, one pass each: m = 300, sigma = 371 keeps all but 1000 at kappa 1; then m = 125 and 200 goes
    assert _pixel([100.0, 100.0, 100.0, 200.0, 1000.0], 'sigma', 1.0, 1) == (125.0, 4)
    assert _pixel([100.0, 100.0, 100.0, 200.0, 1000.0], 'sigma', 1.0, 2) == (100.0, 3)


def test_sigma_special_cases():
    assert _pixel([7.0, 7.0, 7.0, 7.0], 'sigma', 1.0, 3) == (7.0, 4)                                # q = 0: the limit is 0, all are on it
    assert _pixel([1.0, 1000.0], 'sigma', 1.0) == (500.5, 2)                                        # n < 3: the mean
    assert _pixel([1.0, 5.0, 1000.0], 'sigma', 1.0, present=[True, False, True]) == (500.5, 2)
    # a pass that leaves fewer than three ends the passes: 1, 2, 1000 at kappa 1 drops 1000, and 1 and 2 are not clipped again
    assert _pixel([1.0, 2.0, 1000.0], 'sigma', 1.0, 3) == (1.5, 2)
    # keep-none: a sample that overflowed makes the mean infinite and every deviation NaN or infinite -- the set stays as it was
    m, count = _pixel([1.0, np.inf, 3.0], 'sigma', 1.0, 3)
    assert m == np.inf and count == 3
    src = np.full((1, 1), 65535, np.uint16)
    out, count = sr.stack_combine([src] * 3, [(1.0, 0.0, 0.0, g) for g in (1.0, 1e305, 1.0)], (1, 1), 'sigma', 1.0, 3)
    assert out.tolist() == [[65535]] and count.tolist() == [[3]]


def test_sums_follow_the_source_order():
    """(a + b) + c against (c + b) + a: a case where they differ, so that the order is part of the contract."""
    v = [1e16, 1.0, 1.0]
    assert _pixel(v, 'mean')[0] != _pixel(v[::-1], 'mean')[0]


def test_ssd_by_hand():
    ref = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint16)
    img = np.array([[9, 8, 7], [6, 5, 4], [3, 2, 1]], np.uint16)
    got = sr.shift_ssd(ref, img, 1)
    assert got[9] == 1 and got[:9].tolist() == [(5 - int(t)) ** 2 for t in img.ravel()]             # one pixel: the centre
    got = sr.shift_ssd(ref, img, 0)
    assert got.tolist() == [int(((ref.astype(int) - img.astype(int)) ** 2).sum()), 9]
    assert sr.shift_ssd(ref, img, 2).tolist() == [0] * 26                                           # w < 2 S + 1: empty
    assert sr.shift_ssd(ref, img, 0, (50.0, 50.0, 3.0)).tolist() == [0, 0]                          # the circle is off the image
    assert sr.shift_ssd(ref, img, 0, (1.0, 1.0, 1.0)).tolist() == [36 + 4 + 0 + 4 + 36, 5]                   # the plus-shaped five
    assert sr.shift_ssd(ref, img, 0, (-1, -1, -1)).tolist() == sr.shift_ssd(ref, img, 0).tolist()
    big = sr.shift_ssd(np.zeros((64, 64), np.uint16), np.full((64, 64), 65535, np.uint16), 0)
    assert int(big[0]) == 65535 ** 2 * 4096 and big.dtype == np.uint64


# ---- the parabola, and the host step of stack.py against its restatement ----
@pytest.mark.parametrize('vertex', [0.0, 0.3, -0.45, 0.5])
def test_parabola_refinement_on_known_quadratics(vertex):
    from solex_ser_recon_en_amd import stack
    e = [3.0 * (x - vertex) ** 2 + 11.0 for x in (-1.0, 0.0, 1.0)]
    for fn in (sr.parabola_offset, stack.parabola_offset):
        assert abs(float(fn(*e)) - vertex) < 1e-12
        assert fn(5.0, 5.0, 5.0) == 0.0 and fn(1.0, 5.0, 1.0) == 0.0                                # flat, and a maximum: no move


def test_refine_offset_matches_the_restatement_bit_for_bit():
    from solex_ser_recon_en_amd import stack
    rng = np.random.default_rng(5)
    for search in (0, 1, 3, 8):
        side = 2 * search + 1
        for trial in range(20):
            table = rng.integers(1 << 30, 1 << 58, side * side + 1).astype(np.uint64)
            table[-1] = 1234 if trial else 0
            if trial % 3 == 0 and search:                                    # a tie: the first in row-major order wins
                table[[side + 1, 2 * side + 2][:1 + (search > 1)]] = 7
            if trial % 4 == 1:                                               # a minimum on the border
                table[rng.integers(0, side)] = 3
            got = stack.refine_offset(table.view(np.int64), search)
            u, v, du, dv, least, pixels, rejected = sr.refine_offset(table, search)
            assert (got['u'], got['v'], got['ssd'], got['pixels'], got['rejected']) == (u, v, least, pixels, rejected)
            assert np.float64(got['du']).view(np.uint64) == np.float64(du).view(np.uint64)
            assert np.float64(got['dv']).view(np.uint64) == np.float64(dv).view(np.uint64)
            if trial % 4 == 1 and search:
                assert rejected and du == 0.0 and dv == 0.0
            if trial == 0:
                assert rejected
    with pytest.raises(ValueError):
        stack.refine_offset(np.zeros(9, np.int64), 1)


def test_transforms_compose_as_the_restatement_does():
    from solex_ser_recon_en_amd import stack
    circle, ref = (131.7, 120.2, 118.9), (124.3, 128.6, 120.4)
    s, tx, ty = stack.initial_transform(circle, ref)
    assert s == np.float64(118.9) / np.float64(120.4) and tx == np.float64(131.7) - s * np.float64(124.3)
    assert ty == np.float64(120.2) - s * np.float64(128.6)
    fit = {'u': -2, 'v': 3, 'du': 0.25, 'dv': -0.125}
    assert stack.refined_transform(s, tx, ty, fit) == (tx + s * np.float64(-1.75), ty + s * np.float64(2.875))
    with pytest.raises(ValueError, match='radius'):
        stack.initial_transform((1.0, 1.0, 0.0), ref)


def test_a_resampled_disk_registers_back_to_its_transform():
    """B(c, r) = A(tx0 + s0 c, ty0 + s0 r): B's circle follows from A's, handed over a pixel and more off; registered against A the
    record must map A's grid into B by the inverse, within the registration bound."""
    a, circle_a = fr.synthetic_disk(0.0)
    s0, tx0, ty0 = 1.008, -2.3, 1.7
    b = sr.stack_combine([a], [(s0, tx0, ty0, 0.9)], a.shape, 'mean')[0]
    circle_b = ((circle_a[0] - tx0) / s0, (circle_a[1] - ty0) / s0, circle_a[2] / s0)
    given = (circle_b[0] + 1.4, circle_b[1] - 0.9, circle_b[2])
    records = sr.register_disks([a, b], [circle_a, given])
    rec = records[1]
    assert not rec['rejected'] and records[0]['s'] == 1.0 and records[0]['gain'] == 1.0
    err = sr.registration_error(rec, circle_b, circle_a)
    print('registers back within %.6f px; offset %s; gain %.6f' % (err, rec['offset'], rec['gain']))
    assert err <= sr.TOLERANCE['registration']
    assert abs(rec['offset'][0] + 1.4) < 0.2 and abs(rec['offset'][1] - 0.9) < 0.2                  # the search took the error out
    assert abs(rec['gain'] - 1.0 / 0.9) < 0.002


# ---- the accuracy, re-measured ----
def test_accuracy_on_the_synthetic_series():
    measured = sr.series_measures(lambda images, circles, mode: sr.stack_series(images, circles, 0, mode, sr.SERIES_KAPPA))
    print('registration %.6f px; noise %.6f of a frame\'s; streak %.6f under sigma, %.6f under mean; offsets %s'
          % (measured['registration'], measured['noise'], measured['streak_sigma'], measured['streak_mean'], measured['offsets']))
    # a condition of the measurement: the search rejects none of the frames, every minimum strictly inside the window
    assert measured['rejected'] == []
    for u, v in measured['offsets']:
        assert abs(u) < 7.5 and abs(v) < 7.5
    for key in ('registration', 'noise', 'streak_mean'):
        assert measured[key] <= sr.TOLERANCE[key], (key, measured[key])
    assert abs(measured['streak_sigma']) <= sr.TOLERANCE['streak_sigma']
    assert measured['streak_mean'] > 20 * abs(measured['streak_sigma'])                             # the clipping is what removes it


def test_the_series_is_what_it_claims():
    images, true, given = sr.synthetic_series()
    assert len(images) == 5 and all(img.shape == (260, 250) and img.dtype == np.uint16 for img in images)
    for i, (dx, dy, scale, gain, err) in enumerate(sr.SERIES):
        assert abs(dx) <= 3 and abs(dy) <= 3 and abs(scale - 1) <= 0.01 + 1e-12 and 0.8 <= gain <= 1.2 and max(map(abs, err)) < 2
        assert i == 0 or (dx != round(dx) and dy != round(dy))
    lit = images[sr.STREAK_FRAME][sr.STREAK_ROWS[0], 100:150].astype(float).mean()
    assert lit > 1.4 * images[sr.STREAK_FRAME][sr.STREAK_ROWS[0] - 3, 100:150].astype(float).mean()


# ---- the C ABI without a device ----
def _arrays(n=2, dims=(20, 20, 20), xform=IDENTITY):
    ptrs = (ctypes.c_void_p * 32)(*([4096] * 32))
    d = (ctypes.c_int64 * 96)(*(list(dims) * 32))
    x = (ctypes.c_double * 128)(*(list(xform) * 32))
    return ptrs, d, x


def test_stack_calls_refuse_bad_arguments_before_any_device_work():
    """Every refusal comes before the first HIP call: made-up addresses are never touched."""
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    out, cnt = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)

    def combine(n=2, dims=(20, 20, 20), xform=IDENTITY, mode=2, kappa=2.5, iterations=2, out=out, oh=20, ow=20, out_pitch=20, count=cnt,
                count_pitch=20, srcs=True, have_dims=True, have_xform=True, null_src=None):
        ptrs, d, x = _arrays(n, dims, xform)
        if null_src is not None:
            ptrs[null_src] = None
        return lib.shg_stack_combine_u16(ptrs if srcs else None, d if have_dims else None, x if have_xform else None, n, mode, kappa,
                                         iterations, out, oh, ow, out_pitch, count, count_pitch, None)

    for over in (dict(oh=0), dict(ow=16385, out_pitch=16385, count_pitch=16385), dict(dims=(0, 20, 20)), dict(dims=(20, 16385, 16385))):
        assert combine(**over) == E_UNSUPPORTED, over
    nan, inf = float('nan'), float('inf')
    for over in (dict(n=0), dict(n=33), dict(srcs=False), dict(have_dims=False), dict(have_xform=False), dict(out=None), dict(null_src=1),
                 dict(out_pitch=19), dict(count_pitch=19), dict(dims=(20, 20, 19)), dict(mode=3), dict(mode=-1), dict(kappa=nan),
                 dict(kappa=0.5), dict(iterations=0), dict(iterations=4), dict(mode=0, kappa=0.5), dict(mode=1, iterations=4),
                 dict(xform=(0.0, 0.0, 0.0, 1.0)), dict(xform=(-1.0, 0.0, 0.0, 1.0)), dict(xform=(nan, 0.0, 0.0, 1.0)),
                 dict(xform=(inf, 0.0, 0.0, 1.0)), dict(xform=(1.0, nan, 0.0, 1.0)), dict(xform=(1.0, 0.0, inf, 1.0)),
                 dict(xform=(1.0, 0.0, 0.0, -0.5)), dict(xform=(1.0, 0.0, 0.0, nan)), dict(xform=(1.0, 0.0, 0.0, inf)),
                 dict(out=ctypes.c_void_p(4096)), dict(out=ctypes.c_void_p(4096 + 798)), dict(count=ctypes.c_void_p(4096 + 10)),
                 dict(count=out)):
        assert combine(**over) == E_ARG, over
    assert 'overlaps' in _lib.last_error()
    assert combine(count=None, count_pitch=0, out=None) == E_ARG                                    # (count may be NULL, out may not)

    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    ok = (ctypes.c_double * 3)(10.0, 10.0, 4.5)

    def ssd(ref=p, ref_pitch=20, img=q, img_pitch=20, h=20, w=20, s=8, c3=ok, table=out):
        return lib.shg_shift_ssd_u16(ref, ref_pitch, img, img_pitch, h, w, s, c3, table, None)

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385, ref_pitch=16385, img_pitch=16385)):
        assert ssd(**over) == E_UNSUPPORTED, over
    for over in (dict(ref=None), dict(img=None), dict(table=None), dict(ref_pitch=19), dict(img_pitch=19), dict(s=-1), dict(s=9),
                 dict(c3=(ctypes.c_double * 3)(nan, 10.0, 4.5)), dict(c3=(ctypes.c_double * 3)(10.0, 10.0, inf))):
        assert ssd(**over) == E_ARG, over


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from solex_ser_recon_en_amd import ops
    img = torch.zeros((8, 8), dtype=torch.uint16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.stack_combine_u16([img], [IDENTITY], (8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.shift_ssd_u16(img, img, 1)
    with pytest.raises(ValueError, match='mode'):
        ops.stack_combine_u16([img], [IDENTITY], (8, 8), mode='best')
    with pytest.raises(ValueError, match='transforms'):
        ops.stack_combine_u16([img, img], [IDENTITY], (8, 8))


# ---- stack_scans' and the command line's refusals ----
def test_stack_scans_refusals():
    from solex_ser_recon_en_amd import SHG_MAIN, stack
    two = ['no-such-a.ser', 'no-such-b.ser']
    for over in (dict(ratio_fixe=1.1), dict(slant_fix=0.5)):
        with pytest.raises(ValueError, match='circle'):
            stack.stack_scans(two, dict(SHG_MAIN.default_options(), **over))
    with pytest.raises(ValueError, match='de-vignette'):
        stack.stack_scans(two, dict(SHG_MAIN.default_options(), **{'de-vignette': True}))
    with pytest.raises(ValueError, match='at least two'):
        stack.stack_scans(two[:1])
    with pytest.raises(ValueError, match='at most 32'):
        stack.stack_scans(['no-such-%d.ser' % i for i in range(33)])
    with pytest.raises(ValueError, match='reference'):
        stack.stack_scans(two, reference=2)
    for over in (dict(mode='best'), dict(kappa=0.5), dict(kappa=float('nan')), dict(iterations=0), dict(iterations=4)):
        with pytest.raises(ValueError):
            stack.stack_scans(two, **over)


def test_scan_disk_refuses_a_frame_shard(monkeypatch):
    from solex_ser_recon_en_amd import dist, stack

    class Shard:
        FrameCount, frame_range, ih, iw = 300, (0, 150), 400, 48

        def device_stack(self):
            raise AssertionError('the shard must be refused before its frames are asked for')

    monkeypatch.setattr(dist, 'active', lambda: True)
    with pytest.raises(ValueError, match='stacking is single-process'):
        stack.scan_disk(Shard())


@pytest.mark.parametrize('world', [None, '2'])
@pytest.mark.parametrize('argv, message', [
    (['a.ser', 'b.ser', '-w', '3'], '-w is not a stack flag'),
    (['a.ser'], 'at least two'),
    (['scan%02d.ser' % i for i in range(33)], 'at most 32'),
    (['a.ser', 'b.ser', '--kappa', '0.5'], '--kappa'),
    (['a.ser', 'b.ser', '--kappa', 'nan'], '--kappa'),
    (['a.ser', 'b.ser', '--iterations', '4'], '--iterations'),
    (['a.ser', 'b.ser', '--search', '9'], '--search'),
    (['a.ser', 'b.ser', '--mode', 'best'], 'invalid choice'),
    (['a.ser', 'b.ser', '--reference', '2'], '--reference'),
    (['a.ser', 'b.ser'], 'no such file'),
])
def test_command_line_refusals(monkeypatch, capsys, world, argv, message):
    from solex_ser_recon_en_amd import stack
    if world is None:
        monkeypatch.delenv('WORLD_SIZE', raising=False)
    else:
        monkeypatch.setenv('WORLD_SIZE', world)
    with pytest.raises(SystemExit) as exit_info:
        stack.main(argv)
    assert exit_info.value.code == 2
    err = capsys.readouterr().err
    # under torchrun the refusal of torchrun comes first, except where argparse itself refuses the value
    assert (message if world is None or message == 'invalid choice' else 'without torchrun') in err
