"""Local alignment points, without a GPU: the lattice arithmetic, the restatement (tests/align_ref.py) against hand-worked cases, the
host steps of stack.py -- measure_field, fill_field, field_stats -- against their restatement bit for bit, the fill rule on an
isolated hole, a whole unmeasured border and nothing measured, the accuracy on the synthetic series -- re-measured here, printed,
and held to align_ref.TOLERANCE --, the argument refusals of the two entry points that need no device, and the refusals of the new
command-line flags."""
import ctypes

import numpy as np
import pytest

from tests import align_ref as ar
from tests import stack_ref as sr

E_ARG, E_UNSUPPORTED = -1, -3
IDENTITY = (1.0, 0.0, 0.0, 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the lattice ----
@pytest.mark.parametrize('shape, step, want', [((1, 1), 8, (1, 1)), ((1, 7), 8, (1, 2)), ((9, 8), 8, (2, 2)), ((10, 9), 8, (3, 2)),
                                               ((37, 263), 16, (4, 18)), ((64, 256), 16, (5, 17)), ((260, 250), 16, (18, 17)),
                                               ((2000, 2000), 16, (126, 126)), ((17, 16), 128, (2, 2))])
def test_lattice_arithmetic(shape, step, want):
    from solex_ser_recon_en_amd import ops, stack
    gh, gw, points = stack.align_lattice(shape, step)
    assert (gh, gw) == want == ops.lattice_shape(shape, step) == ar.lattice_shape(shape, step)
    assert points.dtype == np.int32 and points.shape == (gh * gw, 2) and np.array_equal(points, ar.align_lattice(shape, step)[2])
    assert points[0].tolist() == [0, 0] and points[1 if gw > 1 else 0].tolist() == [0, step if gw > 1 else 0]
    # the lattice covers the grid: the last node lies on or beyond the last pixel, the one before it inside
    assert (gh - 1) * step >= shape[0] - 1 and (gw - 1) * step >= shape[1] - 1
    assert (gh == 1 or (gh - 2) * step < shape[0] - 1) and (gw == 1 or (gw - 2) * step < shape[1] - 1)
    # every pixel's cell exists: j = r // step <= gh - 1
    assert (shape[0] - 1) // step <= gh - 1 and (shape[1] - 1) // step <= gw - 1


def test_lattice_refusals():
    from solex_ser_recon_en_amd import stack
    with pytest.raises(ValueError):
        stack.align_lattice((0, 5), 8)
    for over in (dict(step=7), dict(step=129), dict(size=32), dict(size=1), dict(size=67), dict(search=9), dict(search=-1),
                 dict(min_contrast=-0.1), dict(min_contrast=float('nan'))):
        args = dict(dict(step=16, size=33, search=4, min_contrast=0.0), **over)
        with pytest.raises(ValueError):
            stack.check_local(**args)


# ---- the restatement against hand-worked cases ----
def test_patch_ssd_by_hand():
    ref = np.arange(1, 26, dtype=np.uint16).reshape(5, 5)
    img = ref[::-1, ::-1].copy()
    # B = 1 around the centre, S = 1: the 3 x 3 patch, all of it at least one pixel from every edge
    got = ar.patch_ssd(ref, img, [(2, 2)], 1, 1)[0]
    assert got.dtype == np.uint64 and got[9:].tolist() == [9, int(ref[1:4, 1:4].sum()), int((ref[1:4, 1:4].astype(int) ** 2).sum())]
    whole = sr.shift_ssd(ref, img, 1)
    assert got[:10].tolist() == whole.tolist()                                   # the same set as the whole-image call's
    # a corner: of the 3 x 3 patch around (0, 0) one pixel, (1, 1), is a pixel from the edges
    got = ar.patch_ssd(ref, img, [(0, 0)], 1, 1)[0]
    assert got[9:].tolist() == [1, 7, 49] and got[4] == (7 - 19) ** 2 and got[0] == (7 - 25) ** 2
    # outside the image, and a circle that leaves nothing: rows of zeros; two equal points: two equal rows
    got = ar.patch_ssd(ref, img, [(-40, 2), (2, 2), (2, 2), (2, 900)], 1, 1)
    assert (got[0] == 0).all() and (got[3] == 0).all() and np.array_equal(got[1], got[2]) and got[1, 9] == 9
    assert (ar.patch_ssd(ref, img, [(2, 2)], 1, 0, (40.0, 40.0, 3.0)) == 0).all()
    got = ar.patch_ssd(ref, img, [(2, 2)], 2, 0, (2.0, 2.0, 1.0))[0]             # the plus-shaped five
    assert got.tolist() == [sum((int(ref[r, c]) - int(img[r, c])) ** 2 for r, c in ((1, 2), (2, 1), (2, 2), (2, 3), (3, 2))), 5, 65, 64 + 144 + 169 + 196 + 324]
    big = ar.patch_ssd(np.zeros((81, 81), np.uint16), np.full((81, 81), 65535, np.uint16), [(40, 40)], 32, 8)[0]
    assert (big[:289] == 65535 ** 2 * 4225).all() and big[289:].tolist() == [4225, 0, 0]


def test_displacement_by_hand():
    field = np.zeros((2, 3, 2))
    field[0, 1] = (8.0, -4.0)                                                    # one node, at (r, c) = (0, 8), on a 9 x 10 grid, step 8
    dx, dy = ar.displacement(field, (9, 10), 8)
    assert dx[0, 8] == 8.0 and dy[0, 8] == -4.0 and dx[0, 4] == 4.0 and dx[4, 8] == 4.0 and dx[4, 4] == 2.0 and dy[2, 9] == -2.625
    assert dx[8, 8] == 0.0 and dx[0, 0] == 0.0
    # the last lattice row and column clamp: a 1 x 1 lattice is one constant
    dx, dy = ar.displacement(np.array([[[0.5, -0.25]]]), (1, 1), 8)
    assert dx.tolist() == [[0.5]] and dy.tolist() == [[-0.25]]


def test_field_combine_restatement_by_hand():
    src = (np.arange(20, dtype=np.uint16) * 100).reshape(1, 20)
    shape = (1, 20)
    gh, gw = ar.lattice_shape(shape, 8)
    assert (gh, gw) == (1, 4)
    zero = np.zeros((gh, gw, 2))
    plain = sr.stack_combine([src], [IDENTITY], shape, 'mean')
    for field in (None, zero):
        out, count = ar.stack_combine_field([src], [IDENTITY], [field], 8, shape, 'mean')
        assert np.array_equal(out, plain[0]) and np.array_equal(count, plain[1])
    half = zero.copy()
    half[..., 0] = 0.5                                                           # every pixel reads half a pixel to the right
    out, count = ar.stack_combine_field([src], [IDENTITY], [half], 8, shape, 'mean')
    assert out[0, :19].tolist() == [100 * c + 50 for c in range(19)] and count[0].tolist() == [1] * 19 + [0]
    nan = zero.copy()
    nan[0, 1, 1] = np.nan                                                        # the node at column 8: its two cells lose their samples
    out, count = ar.stack_combine_field([src], [IDENTITY], [nan], 8, shape, 'mean')
    assert count[0].tolist() == [0] * 16 + [1] * 4 and (out[0, :16] == 0).all()
    out, count = ar.stack_combine_field([src, src], [IDENTITY] * 2, [nan, None], 8, shape, 'median')
    assert count[0].tolist() == [1] * 16 + [2] * 4 and np.array_equal(out, src)


# ---- the host steps against their restatement, and the fill rule ----
def random_tables(gh, gw, search, half, seed):
    rng = np.random.default_rng(seed)
    n_off = (2 * search + 1) ** 2
    full = (2 * half + 1) ** 2
    table = rng.integers(1 << 20, 1 << 44, (gh * gw, n_off + 3)).astype(np.int64)
    table[:, n_off] = rng.choice([0, full // 2, full // 2 + 1, full], gh * gw)  # empty, just under half (full is odd), just over, whole
    table[:, n_off + 1] = table[:, n_off] * rng.integers(100, 60000, gh * gw)
    table[:, n_off + 2] = (table[:, n_off + 1].astype(np.float64) ** 2 / np.maximum(table[:, n_off], 1) * rng.uniform(1.0, 1.02, gh * gw)).astype(np.int64)
    for p in range(0, gh * gw, 3):                                               # a clear minimum inside the window for a third
        table[p, rng.integers(1, 2 * search) * (2 * search + 1) + rng.integers(1, 2 * search)] = 5
    return table


@pytest.mark.parametrize('min_contrast', [0.0, 0.08])
def test_host_steps_match_the_restatement_bit_for_bit(min_contrast):
    from solex_ser_recon_en_amd import stack
    gh, gw, search, half = 7, 9, 3, 6
    table = random_tables(gh, gw, search, half, 11)
    got, got_m = stack.measure_field(table, gh, gw, half, search, min_contrast)
    want, want_m = ar.measure_field(table.view(np.uint64), gh, gw, half, search, min_contrast)
    assert np.array_equal(got_m, want_m) and np.array_equal(bits(got), bits(want)) and 0 < want_m.sum() < gh * gw
    assert not got_m.reshape(-1)[table[:, -3] * 2 < (2 * half + 1) ** 2].any()
    if min_contrast:
        assert want_m.sum() < ar.measure_field(table, gh, gw, half, search, 0.0)[1].sum()         # the knob leaves nodes out
    assert np.array_equal(bits(stack.fill_field(got, got_m)), bits(ar.fill_field(want, want_m)))
    stats, want_stats = stack.field_stats(got, got_m), ar.field_stats(want, want_m)
    assert stats == want_stats and stats['points'] == gh * gw and stats['used'] == int(want_m.sum()) and stats['max'] >= stats['rms'] > 0


def test_fill_rule():
    from solex_ser_recon_en_amd import stack
    rng = np.random.default_rng(3)
    field = rng.normal(0.0, 1.5, (6, 7, 2))
    for fill in (stack.fill_field, ar.fill_field):
        # an isolated hole: the mean of its eight neighbours, added in row-major order
        measured = np.ones((6, 7), bool)
        measured[2, 3] = False
        out = fill(field, measured)
        total = np.zeros(2)
        for dj, di in ar.NEIGHBOURS:
            total = total + field[2 + dj, 3 + di]
        assert np.array_equal(bits(out[2, 3]), bits(total / 8.0)) and np.array_equal(bits(out[measured]), bits(field[measured]))
        # a corner hole has three neighbours
        measured = np.ones((6, 7), bool)
        measured[0, 0] = False
        assert np.array_equal(bits(fill(field, measured)[0, 0]), bits(((field[0, 1] + field[1, 0]) + field[1, 1]) / 3.0))
        # a whole unmeasured border, two nodes deep on the left: the first pass fills the inner ring from the measured nodes alone,
        # the second the outer column from the first pass's state
        measured = np.zeros((6, 7), bool)
        measured[1:5, 2:6] = True
        out = fill(field, measured)
        assert np.array_equal(bits(out[measured]), bits(field[measured])) and np.isfinite(out).all()
        assert np.array_equal(bits(out[0, 1]), bits(field[1, 2]))                                  # one filled neighbour: its value
        assert np.array_equal(bits(out[0, 3]), bits(((field[1, 2] + field[1, 3]) + field[1, 4]) / 3.0))
        assert np.array_equal(bits(out[0, 0]), bits(((out[0, 1] + out[1, 1])) / 2.0))              # second pass: (0, 1) and (1, 1)
        assert np.array_equal(bits(out[1, 1]), bits(((field[1, 2] + field[2, 2])) / 2.0))
        # nothing measured: all zero, whatever the raw field held
        assert (fill(field, np.zeros((6, 7), bool)) == 0.0).all()
        # everything measured: the field itself
        assert np.array_equal(bits(fill(field, np.ones((6, 7), bool))), bits(field))
    hole = rng.random((9, 11)) < 0.7
    assert np.array_equal(bits(stack.fill_field(rng.normal(0, 1, (9, 11, 2)) * 0 + 1.25, hole)), bits(np.full((9, 11, 2), 1.25)))
    assert stack.field_stats(field, np.zeros((6, 7), bool)) == {'points': 42, 'used': 0, 'rms': 0.0, 'max': 0.0}


# ---- the accuracy, re-measured ----
def test_accuracy_on_the_synthetic_series():
    m = ar.series_measures(lambda images, circles, local: ar.stack_series(images, circles, 0, 'mean', local=local),
                           lambda images, records, circles: ar.local_fields(images, records, circles, want_measured=True))
    print('displacement: rms %.6f px, worst %.6f px over %s measured nodes; %d of %d whole patches rejected; noise against frame 0\'s '
          '(%.2f counts): %.6f with the fields, %.6f without; the fields\' own rms and max: %s'
          % (m['rms'], m['worst'], m['used'], m['rejected_inside'], 2 * m['inside'], m['frame'], m['noise_local'] / m['frame'],
             m['noise_global'] / m['frame'], [(round(s['rms'], 3), round(s['max'], 3)) for s in m['stats']]))
    assert m['rejected_inside'] == 0 and m['inside'] >= 80                       # a condition of the measurement
    assert m['rms'] <= ar.TOLERANCE['rms'] and m['worst'] <= ar.TOLERANCE['worst']
    assert m['noise_local'] / m['frame'] <= ar.TOLERANCE['noise']
    assert m['noise_local'] < m['noise_global']                                  # or the feature does nothing
    images, _, given = ar.synthetic_series()
    least, median = ar.patch_contrast(images[0], given[0])
    print('contrast of the reference\'s whole patches: %.4f at least, median %.4f' % (least, median))
    assert least > 0.02


def test_the_series_is_what_it_claims():
    images, true, given = ar.synthetic_series()
    assert len(images) == 3 and all(img.shape == (260, 250) and img.dtype == np.uint16 and not img.flags.writeable for img in images)
    assert true == [sr.series_circle(i) for i in range(3)] and given[1] == (true[1][0] + 1.3, true[1][1] - 0.8, true[1][2])
    t = ar.texture()
    assert abs(t.std() - 0.05) < 1e-12 and abs(t.mean()) < 0.01
    acf = float((t[:, 2:] * t[:, :-2]).mean() / (t * t).mean())                  # a Gaussian of sigma 2 twice: exp(-4 / 16) at a lag of 2
    assert 0.6 < acf < 0.9
    r, c = np.arange(260.0)[:, None], np.arange(250.0)[None, :]
    assert (ar.bend(0, r, c)[0] == 0).all()
    for i in (1, 2):
        dx, dy = ar.bend(i, r, c)
        assert dx.shape == (260, 250) and abs(np.abs(dx).max() - 1.5) < 0.01 and abs(np.abs(dy).max() - 1.5) < 0.01
        assert (dx[:, :1] == dx).all() and (dy[:1, :] == dy).all()               # dx along the rows, dy along the columns
    assert ar.PHASES[1] != ar.PHASES[2]


# ---- the C ABI without a device ----
def test_align_calls_refuse_bad_arguments_before_any_device_work():
    """Every refusal comes before the first HIP call: made-up addresses are never touched."""
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    p, q, pts, out = (ctypes.c_void_p(v) for v in (4096, 8192, 1 << 16, 1 << 20))
    ok = (ctypes.c_double * 3)(10.0, 10.0, 4.5)
    nan, inf = float('nan'), float('inf')

    def ssd(ref=p, ref_pitch=20, img=q, img_pitch=20, h=20, w=20, points=pts, n=5, b=4, s=2, c3=ok, table=out):
        return lib.shg_patch_ssd_u16(ref, ref_pitch, img, img_pitch, h, w, points, n, b, s, c3, table, None)

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385, ref_pitch=16385, img_pitch=16385)):
        assert ssd(**over) == E_UNSUPPORTED, over
    for over in (dict(ref=None), dict(img=None), dict(points=None), dict(table=None), dict(ref_pitch=19), dict(img_pitch=19), dict(n=0),
                 dict(n=-1), dict(n=(1 << 23) + 1), dict(b=0), dict(b=33), dict(s=-1), dict(s=9),
                 dict(c3=(ctypes.c_double * 3)(nan, 10.0, 4.5)), dict(c3=(ctypes.c_double * 3)(10.0, 10.0, inf)),
                 dict(table=ctypes.c_void_p(4096 + 2 * (19 * 20 + 19))), dict(table=ctypes.c_void_p(8192 - 8 * 5 * 28 + 8)),
                 dict(table=ctypes.c_void_p((1 << 16) + 4 * 9))):
        assert ssd(**over) == E_ARG, over
    assert 'overlaps' in _lib.last_error()

    cnt, field = ctypes.c_void_p(1 << 21), 1 << 22

    def combine(n=2, dims=(20, 20, 20), xform=IDENTITY, fields=(field, None), gh=4, gw=4, step=8, mode=2, kappa=2.5, iterations=2, out=out,
                oh=20, ow=20, out_pitch=20, count=cnt, count_pitch=20, have_fields=True, have_srcs=True, have_dims=True, have_xform=True):
        ptrs = (ctypes.c_void_p * 32)(*([4096] * 32))
        d = (ctypes.c_int64 * 96)(*(list(dims) * 32))
        x = (ctypes.c_double * 128)(*(list(xform) * 32))
        f = (ctypes.c_void_p * 32)(*(list(fields) + [None] * (32 - len(fields))))
        return lib.shg_stack_combine_field_u16(ptrs if have_srcs else None, d if have_dims else None, x if have_xform else None,
                                               f if have_fields else None, gh, gw, step, n, mode, kappa, iterations, out, oh, ow,
                                               out_pitch, count, count_pitch, None)

    for over in (dict(oh=0), dict(dims=(0, 20, 20))):
        assert combine(**over) == E_UNSUPPORTED, over
    for over in (dict(have_fields=False), dict(have_srcs=False), dict(have_dims=False), dict(have_xform=False), dict(step=7),
                 dict(step=129), dict(step=0), dict(gh=3), dict(gh=5), dict(gw=3), dict(gw=5), dict(step=16, gh=4, gw=4), dict(n=0), dict(n=33), dict(out=None), dict(out_pitch=19), dict(mode=3), dict(kappa=0.5),
                 dict(iterations=4), dict(xform=(1.0, nan, 0.0, 1.0)), dict(fields=(field + 8, None)),
                 dict(out=ctypes.c_void_p(field)), dict(out=ctypes.c_void_p(field + 4 * 4 * 16 - 2)), dict(count=ctypes.c_void_p(field + 16)),
                 dict(out=ctypes.c_void_p(field - 2 * (19 * 20 + 19))), dict(fields=(None, field), count=ctypes.c_void_p(field + 255))):
        assert combine(**over) == E_ARG, over
    assert 'overlaps' in _lib.last_error()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from solex_ser_recon_en_amd import ops
    img = torch.zeros((8, 8), dtype=torch.uint16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.patch_ssd_u16(img, img, [(4, 4)], 2, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.stack_combine_field_u16([img], [IDENTITY], [None], 8, (8, 8))
    with pytest.raises(ValueError, match='mode'):
        ops.stack_combine_field_u16([img], [IDENTITY], [None], 8, (8, 8), mode='best')
    with pytest.raises(ValueError, match='fields'):
        ops.stack_combine_field_u16([img, img], [IDENTITY] * 2, [None], 8, (8, 8))
    with pytest.raises(ValueError, match='step'):
        ops.stack_combine_field_u16([img], [IDENTITY], [None], 4, (8, 8))


# ---- stack_scans' and the command line's refusals ----
def test_stack_scans_refuses_a_bad_local():
    from solex_ser_recon_en_amd import stack
    two = ['no-such-a.ser', 'no-such-b.ser']
    for local in (dict(step=4), dict(size=34), dict(size=67), dict(search=9), dict(min_contrast=-1.0), dict(patch=33)):
        with pytest.raises(ValueError):
            stack.stack_scans(two, local=local)
    with pytest.raises(ValueError, match='step'):
        stack.stack_disks([], [], fields=[None])


@pytest.mark.parametrize('argv, message', [
    (['a.ser', 'b.ser', '--ap-size', '33'], '--ap-size needs --local'),
    (['a.ser', 'b.ser', '--ap-step', '16'], '--ap-step needs --local'),
    (['a.ser', 'b.ser', '--ap-search', '4'], '--ap-search needs --local'),
    (['a.ser', 'b.ser', '--ap-min-contrast', '0'], '--ap-min-contrast needs --local'),
    (['a.ser', 'b.ser', '--local', '--ap-size', '32'], '--ap-size'),
    (['a.ser', 'b.ser', '--local', '--ap-size', '1'], '--ap-size'),
    (['a.ser', 'b.ser', '--local', '--ap-size', '67'], '--ap-size'),
    (['a.ser', 'b.ser', '--local', '--ap-step', '7'], '--ap-step'),
    (['a.ser', 'b.ser', '--local', '--ap-step', '129'], '--ap-step'),
    (['a.ser', 'b.ser', '--local', '--ap-search', '0'], '--ap-search'),
    (['a.ser', 'b.ser', '--local', '--ap-search', '9'], '--ap-search'),
    (['a.ser', 'b.ser', '--local', '--ap-min-contrast', '-0.1'], '--ap-min-contrast'),
    (['a.ser', 'b.ser', '--local', '--ap-min-contrast', 'nan'], '--ap-min-contrast'),
    (['a.ser', 'b.ser', '--local', '--ap-size', '65', '--ap-step', '128', '--ap-search', '8', '--ap-min-contrast', '0.5'], 'no such file'),
    (['a.ser', 'b.ser', '--local'], 'no such file'),
])
def test_command_line_refusals(monkeypatch, capsys, argv, message):
    from solex_ser_recon_en_amd import stack
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(SystemExit) as exit_info:
        stack.main(argv)
    assert exit_info.value.code == 2
    assert message in capsys.readouterr().err
