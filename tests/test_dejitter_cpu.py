"""Dejittering without a GPU: the restatement (tests/dejitter_ref.py) held to the properties the method rests on -- the midpoints of a
sheared ellipse's column chords are linear with the planted slope, the weights sum to one, the fill rule --, the package's host steps
(dejitter.crossings, shifts_from_crossings, weights) held to the restatement's, the accuracy re-measured and held in
dejitter_ref.TOLERANCE, and the refusals of both C entry points that are reached before any device call."""
import ctypes

import numpy as np
import pytest

from solex_ser_recon_en_amd import dejitter
from tests import dejitter_ref as jr


@pytest.fixture(scope='module')
def scenes():
    jitter = jr.planted()
    return {'jitter': jitter, 'moved': jr.scene(jitter=jitter), 'still': jr.scene(), 'clean': jr.scene(noise=0.0)}


def package_measure(img, **args):
    """dejitter.measure with the restatement in the kernel's place."""
    t = jr.threshold(img, args.pop('level', 0.2)) if args.get('threshold') is None else args.pop('threshold')
    args.pop('threshold', None)
    window = args.pop('window', 5)
    top, bottom = dejitter.crossings(jr.column_limb(img, window, t), window, t)
    return dejitter.shifts_from_crossings(top, bottom, **args)


def test_midpoints_of_a_sheared_ellipse_are_linear(scenes):
    rec = jr.measure(scenes['clean'])
    m = rec['measured']
    assert m.sum() > 0.9 * rec['crossing'] and rec['rejected_by_max_shift'] == 0
    assert abs(rec['slope'] - jr.SHEAR) < 2e-4
    # without noise what is left is the limb's own profile: the blurred edge passes the level a little further out where the column
    # cuts the limb obliquely, by a small fraction of the blur's 1.2 rows: every column held to a tenth of that
    print('noise-free midpoints about the line: %.6f px rms, worst %.6f' % (rec['rms'], rec['max']))
    assert rec['max'] < 0.12
    # the planted shear is the line's slope also under jitter and noise
    assert abs(jr.measure(scenes['moved'])['slope'] - jr.SHEAR) < 2e-3


def test_package_host_steps_are_the_restatement(scenes):
    for name in ('moved', 'still', 'clean'):
        img = scenes[name]
        for args in ({}, {'window': 9, 'level': 0.3}, {'min_chord': 0.6, 'clip': 2.0, 'max_shift': 1.0}):
            want, got = jr.measure(img, **args), package_measure(img, **args)
            assert np.array_equal(got['measured'], want['measured']) and got['n_measured'] == want['n_measured']
            assert np.allclose(got['shift'], want['shift'], rtol=0, atol=1e-12)
            for key in ('slope', 'intercept', 'rms', 'max'):
                assert abs(got[key] - want[key]) < 1e-12, key
            assert np.array_equal(got['top'], want['top'], equal_nan=True) and np.array_equal(got['bottom'], want['bottom'], equal_nan=True)
    shift = np.concatenate([scenes['jitter'], [0.0, -0.0, 1.0, -3.25, 7.9, 0.5, -0.5, 202.0, -202.0]])
    for got, want in zip(dejitter.weights(shift), jr.weights(shift)):
        assert got.dtype == np.int32 and np.array_equal(got, want)


def test_weights():
    t = np.arange(0, 4097) / 4096.0
    for base in (0.0, -3.0, 7.0):
        offset, weight = dejitter.weights(base + t)
        assert (weight.sum(axis=1) == 16384).all() and weight.min() >= -4096 and weight.max() <= 20480
        assert np.array_equal(offset[:-1], np.full(4096, int(base))) and offset[-1] == int(base) + 1
    offset, weight = dejitter.weights([0.0, 5.0, -2.0])
    assert offset.tolist() == [0, 5, -2] and weight.tolist() == [[0, 16384, 0, 0]] * 3
    offset, weight = dejitter.weights([0.5])
    assert weight.tolist() == [[-1024, 9216, 9216, -1024]]
    for bad in ([np.nan], [np.inf], [20000.0]):
        with pytest.raises(ValueError):
            dejitter.weights(bad)
    # the identity leaves a plane as it came; an integer shift is a copy of rows, the ends repeated
    img = np.random.default_rng(5).integers(0, 65536, (9, 3)).astype(np.uint16)
    assert np.array_equal(jr.apply(img, [0.0, 0.0, 0.0]), img)
    out = jr.apply(img, [2.0, -1.0, 11.0])
    assert np.array_equal(out[:, 0], img[np.minimum(np.arange(9) + 2, 8), 0]) and np.array_equal(out[:, 1], img[np.maximum(np.arange(9) - 1, 0), 1])
    assert (out[:, 2] == img[8, 2]).all()


def crossings_of(mid, chord=100.0):
    mid = np.asarray(mid, dtype=np.float64)
    return mid - chord / 2.0, mid + chord / 2.0


def test_fill_rule():
    w = 40
    x = np.arange(w, dtype=np.float64)
    wobble = 0.3 * np.sin(1.7 * x)
    mid = 90.0 + 0.02 * x + wobble
    top, bottom = crossings_of(mid)
    for gone in ((0, 1, 2), (37, 38, 39), (10, 11, 12, 13), (0, 5, 6, 39)):
        t, b = top.copy(), bottom.copy()
        t[list(gone)] = b[list(gone)] = np.nan
        rec = dejitter.shifts_from_crossings(t, b)
        assert rec['n_measured'] == w - len(gone) and not rec['measured'][list(gone)].any()
        at = np.flatnonzero(rec['measured'])
        for c in gone:
            lo, hi = at[at < c], at[at > c]
            if lo.size == 0:
                want = rec['shift'][hi[0]]
            elif hi.size == 0:
                want = rec['shift'][lo[-1]]
            else:
                a, z = lo[-1], hi[0]
                want = rec['shift'][a] + (rec['shift'][z] - rec['shift'][a]) * (c - a) / (z - a)
            assert abs(rec['shift'][c] - want) < 1e-12, (gone, c)
        assert np.allclose(rec['shift'], jr.shifts(t, b)['shift'], rtol=0, atol=1e-12)
    # a short chord and a column beyond max_shift are unmeasured too, and neither pulls the line
    t, b = top.copy(), bottom.copy()
    t[20], b[20] = mid[20] - 10.0, mid[20] + 10.0
    t[30] += 40.0
    rec = dejitter.shifts_from_crossings(t, b)
    assert not rec['measured'][20] and not rec['measured'][30] and rec['n_measured'] == w - 2 and rec['rejected_by_max_shift'] == 1
    assert not rec['fitted'][30] and abs(rec['slope'] - 0.02) < 2e-3
    assert abs(rec['shift'][30] - (rec['shift'][29] + rec['shift'][31]) / 2.0) < 1e-12
    assert np.abs(rec['shift']).max() < 0.5


def test_a_bump_in_the_sky_and_a_hot_pixel_are_not_shifted(scenes):
    img = scenes['still'].copy()
    plain = jr.measure(img)
    t = plain['threshold']
    # (the disk ends near row 177: a crossing has to move by more than 16 rows to take the midpoint beyond max_shift = 8)
    img[190:195, 120] = 3 * t                       # five rows above T in the sky below the disk: the window's sum crosses there
    img[194, 140] = 65535                           # one hot pixel there: 65535 + 4 sky >= 5 T
    assert 65535 + 4 * 600 >= 5 * t
    for measure in (jr.measure, package_measure):
        rec = measure(img)
        for c in (120, 140):
            assert not rec['measured'][c]
            assert abs(rec['shift'][c] - (rec['shift'][c - 1] + rec['shift'][c + 1]) / 2.0) < 1e-12
        assert rec['rejected_by_max_shift'] == 2 and abs(rec['slope'] - plain['slope']) < 1e-3
        assert np.abs(rec['shift']).max() < 0.2


def test_too_few_columns():
    top, bottom = crossings_of(np.full(40, 50.0))
    top[15:], bottom[15:] = np.nan, np.nan
    for call in (dejitter.shifts_from_crossings, jr.shifts):
        with pytest.raises(ValueError):
            call(top, bottom)
    top, bottom = crossings_of(np.full(40, 50.0))
    top[15:] += 40.0                                # 25 columns with a short chord
    bottom[15:] -= 40.0
    with pytest.raises(ValueError):
        dejitter.shifts_from_crossings(top, bottom)
    top, bottom = crossings_of(50.0 + 20.0 * (np.arange(40) % 2))      # nothing within max_shift of the line
    with pytest.raises(ValueError):
        dejitter.shifts_from_crossings(top, bottom)
    with pytest.raises(ValueError):
        jr.measure(np.zeros((50, 50), np.uint16), 100)


def test_the_restatement_of_the_crossings_on_small_cases():
    col = np.array([0, 0, 9, 9, 9, 9, 0, 0, 0], np.uint16)[:, None]
    assert jr.column_limb(col, 1, 9).tolist() == [[2, 0, 9, 5, 9, 0]]                 # s == K T counts: the comparison is inclusive
    assert jr.column_limb(col, 1, 10).tolist() == [[-1] * 6]
    assert jr.column_limb(col, 3, 6).tolist() == [[1, 9, 18, 4, 18, 9]]
    assert jr.column_limb(col, 3, 0).tolist() == [[-1] * 6] and jr.column_limb(col, 9, 1).tolist() == [[-1] * 6]
    assert jr.column_limb(col[2:], 1, 5).tolist() == [[-1] * 6] and jr.column_limb(col[:6], 1, 5).tolist() == [[-1] * 6]
    top, bottom = jr.crossings(jr.column_limb(col, 3, 4), 3, 4)
    assert top[0] == (0.0 + (12 - 9) / 9.0) + 1.0 and bottom[0] == (4.0 + (18 - 12) / 9.0) + 1.0


def test_accuracy_is_within_the_tolerance(scenes):
    """The three measures of DESIGN.md section 24 on the 200 x 260 scene, through the package's host steps on the restatement of the
    kernels; the two conditions: no column rejected by max_shift, at least 60 % of the columns that cross the disk measured."""
    got = jr.accuracy(package_measure, lambda img, shift: jr.column_shift(img, *dejitter.weights(shift)))
    print('planted %.6f px rms; recovered to %.6f rms, worst %.6f; residual after apply %.6f; floor %.6f; measured %.3f; slope %.5f'
          % tuple(got[k] for k in ('planted_rms', 'shift_rms', 'shift_max', 'residual', 'floor', 'measured_fraction', 'slope')))
    assert 0.7 < got['planted_rms'] < 0.9
    assert got['rejected_by_max_shift'] == 0 and got['measured_fraction'] >= 0.6
    for key, bound in jr.TOLERANCE.items():
        assert got[key] <= bound, key
    assert got == jr.accuracy()


def test_c_entry_points_refuse_without_a_gpu():
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    img, table, out = (ctypes.c_void_p(a) for a in (4096, 65536, 131072))

    def limb(img=img, h=8, w=8, pitch=8, window=5, threshold=100, table=table):
        return lib.shg_column_limb_u16(img, h, w, pitch, window, threshold, table, None)

    offset = np.zeros(8, np.int32)
    weight = np.tile(np.array([0, 16384, 0, 0], np.int32), (8, 1))

    def shift(img=img, n=1, h=8, w=8, pitch=8, stride=64, offset=offset, weight=weight, out=out, out_pitch=8, out_stride=64):
        return lib.shg_column_shift_u16(img, n, h, w, pitch, stride, None if offset is None else offset.ctypes.data,
                                        None if weight is None else weight.ctypes.data, out, out_pitch, out_stride, None)

    def weights_with(c, k, v, fix=None):
        q = weight.copy()
        q[c, k] = v
        if fix is not None:
            q[c, fix] -= v - weight[c, k]
        return q

    for call, name in ((limb, 'shg_column_limb_u16'), (shift, 'shg_column_shift_u16')):
        for over in (dict(img=None), dict(pitch=7)):
            assert call(**over) == -1, (name, over)
            assert name in _lib.last_error()
        for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
            assert call(**over) == -3, (name, over)
            assert name in _lib.last_error()
    for over in (dict(table=None), dict(window=0), dict(window=4), dict(window=17), dict(window=-1), dict(threshold=-1), dict(threshold=65536),
                 dict(table=img), dict(table=ctypes.c_void_p(4096 + 2 * 63)), dict(table=ctypes.c_void_p(4096 - 8 * 24 + 4))):
        assert limb(**over) == -1, over
        assert 'shg_column_limb_u16' in _lib.last_error()
    assert 'overlaps' in _lib.last_error()
    far = offset.copy()
    far[3] = 16385
    near = offset.copy()
    near[7] = -16385
    for over in (dict(out=None), dict(offset=None), dict(weight=None), dict(out_pitch=7), dict(n=0), dict(n=65), dict(n=2, stride=63),
                 dict(n=2, out_stride=63), dict(stride=-1), dict(offset=far), dict(offset=near), dict(weight=weights_with(2, 1, 16385)),
                 dict(weight=weights_with(2, 1, 16383)), dict(weight=weights_with(5, 0, -4097, 1)), dict(weight=weights_with(7, 1, 20481, 2)),
                 dict(out=img), dict(out=ctypes.c_void_p(4096 + 2 * 63)), dict(out=ctypes.c_void_p(4096 - 2 * 63)),
                 dict(n=3, out=ctypes.c_void_p(4096 + 2 * (2 * 64 + 63)))):
        assert shift(**over) == -1, over
        assert 'shg_column_shift_u16' in _lib.last_error()
    assert 'overlaps' in _lib.last_error()


def test_command_line_refusals(capsys):
    for argv, message in ((['x.ser', '--level', '0.2', '--threshold', '3000'], 'exclude each other'), (['x.ser', '--level', '1.5'], '--level lies in'),
                          (['x.ser', '--threshold', '70000'], '--threshold is 0 to 65535'), (['x.ser', '--window', '4'], '--window must be odd'),
                          (['x.ser', '--min-chord', '0'], '--min-chord lies in'), (['x.ser', '--max-shift', '-1'], '--max-shift must be'),
                          (['no_such_file.ser', '--window', '7'], 'no such file')):
        with pytest.raises(SystemExit) as exit_:
            dejitter.main(argv)
        said = capsys.readouterr()
        assert exit_.value.code == 2 and said.out == '' and message in said.err, (argv, said.err)
    from solex_ser_recon_en_amd import deconvolve, sharpen
    for module in (deconvolve, sharpen):
        with pytest.raises(SystemExit) as exit_:
            module.main(['x.png', '--dejitter'])
        said = capsys.readouterr()
        assert exit_.value.code == 2 and '--dejitter goes with a scan' in said.err
