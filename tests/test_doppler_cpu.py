"""The Dopplergram without a GPU: the NumPy restatement (tests/linemaps_ref.py) on hand-built profiles, its recovery of an injected
velocity field (the tolerance the GPU tests hold dopplergram() to), the float32 FITS writer, and the CLI's argument errors."""
import hashlib

import numpy as np
import pytest

from tests import linemaps_ref as ref
from tests.linemaps_util import fit_at, one_row_scan, parabola


def shifts(frames, centre, half_width=5, **kw):
    """the restatement on a one_row_scan, the rows given only"""
    ih = max(frames.shape[1:])
    return ref.line_core_shift(frames, fit_at(centre, ih), half_width, **kw)[:len(centre)]


def test_rotation_and_samples():
    rng = np.random.default_rng(1)
    prof = rng.integers(0, 65535, size=(24, 3, 20), dtype=np.uint16)
    for rotate in (True, False):
        frames = one_row_scan(prof, rotate)
        for y in range(24):
            assert np.array_equal(ref.profiles(frames, y), prof[y].astype(np.int64))
    p8 = prof.astype(np.uint8)
    assert np.array_equal(ref.profiles(one_row_scan(p8), 2), p8[2].astype(np.int64) * 256)


def test_vertex_of_an_exact_parabola():
    # 4 j^2 - 162 j + K: vertex at 162 / 8 = 20.25, and three points of a parabola give its vertex exactly
    p = parabola(48, 4, -162, 2000)
    frames = one_row_scan(np.stack([p[None, :]] * 3))
    got = shifts(frames, [20.7, 20.0, 19.2], 5)
    assert got[:, 0].tolist() == [np.float32(20.25 - 20.7), np.float32(0.25), np.float32(20.25 - 19.2)]


def test_ties_take_the_first_minimum():
    p = np.full(40, 1000, dtype=np.uint16)
    p[17], p[18], p[19], p[20], p[21], p[22] = 900, 500, 700, 600, 500, 800
    got = shifts(one_row_scan(p[None, None, :]), [20.0], 5)[0, 0]
    a, b, e = 900, 500, 700
    assert got == np.float32((18.0 + (a - e) / (2.0 * (a + e - 2 * b))) - 20.0)


def test_minimum_on_the_window_edge_is_nan():
    p = parabola(40, 1, -2 * 14, 400)                          # vertex at 14: outside [20 - 5, 20 + 5], minimum at lo = 15
    assert np.isnan(shifts(one_row_scan(p[None, None, :]), [20.4], 5)[0, 0])
    q = parabola(40, 1, -2 * 26, 700)                          # minimum at hi = 25
    assert np.isnan(shifts(one_row_scan(q[None, None, :]), [20.4], 5)[0, 0])
    assert shifts(one_row_scan(q[None, None, :]), [22.4], 5)[0, 0] == np.float32(26.0 - 22.4)


def test_windows_clip_at_columns_1_and_iw_minus_2():
    assert ref.window(0.3, 0, 5, 40) == (1, 5)
    assert ref.window(37.9, 0, 5, 40) == (32, 38)
    assert ref.window(-0.5, 0, 5, 40) == (1, 5)                 # truncation toward zero, as astype(int)
    assert ref.window(-3.0, 0, 5, 40) is None                   # hi - lo = 1
    assert ref.window(43.0, 0, 5, 40) is None
    assert ref.window(20.0, 0, 1, 40) == (19, 21)
    # a deeper minimum at column 0 is outside the window [1, 5]: the vertex at 3 is found
    p = parabola(40, 10, -60, 200)
    p[0] = 0
    got = shifts(one_row_scan(p[None, None, :]), [0.5], 5)[0, 0]
    assert got == np.float32(3.0 - 0.5)
    p = parabola(40, 10, -2 * 10 * 38, 20000)                  # vertex at 38: outside [32, 38] on the right edge
    assert np.isnan(shifts(one_row_scan(p[None, None, :]), [37.5], 5)[0, 0])


def test_non_finite_fit_rows_are_nan():
    p = parabola(40, 4, -162, 2000)
    frames = one_row_scan(np.stack([p[None, :]] * 4))
    fit = fit_at([20.0] * 4, ih=frames.shape[2])
    fit[1, 0], fit[2, 0], fit[3, 3] = np.nan, np.inf, np.nan
    got = ref.line_core_shift(frames, fit, 5)[:4, 0]
    assert got[0] == np.float32(0.25) and np.isnan(got[1:]).all()


def test_flip_x_and_sharded_column_order():
    p = np.stack([parabola(40, 4, -2 * 4 * 20 + k, 3000) for k in range(5)])      # vertex moves with the frame
    frames = one_row_scan(p[None, :, :])
    plain = shifts(frames, [20.0], 5)[0]
    assert np.unique(plain).size == 5
    assert np.array_equal(shifts(frames, [20.0], 5, flip_x=True)[0], plain[::-1])
    shard = shifts(frames, [20.0], 5, n_cols=9, k_offset=3)[0]
    assert np.isnan(shard[:3]).all() and np.isnan(shard[8:]).all() and np.array_equal(shard[3:8], plain)
    shard = shifts(frames, [20.0], 5, flip_x=True, n_cols=9, k_offset=3)[0]
    assert np.array_equal(shard[1:6], plain[::-1]) and np.isnan(shard[[0, 6, 7, 8]]).all()


@pytest.mark.parametrize('noise', sorted(ref.TOLERANCE['doppler']))
def test_restatement_recovers_an_injected_field(noise):
    ih, n, iw = 400, 300, 48
    rms_tol, max_tol = ref.TOLERANCE['doppler'][noise]
    field = ref.injected_field(ih, n)
    frames, centre, on = ref.doppler_scan(field, iw, noise=noise, seed=3)
    got = ref.line_core_shift(frames, fit_at(centre), 5)
    err = (got.astype(np.float64) - field)[on]
    rms, mx = float(np.sqrt(np.mean(err * err))), float(np.abs(err).max())
    print('noise %g: RMS %.4f, max %.4f px over %d disk samples' % (noise, rms, mx, err.size))
    assert not np.isnan(err).any() and rms <= rms_tol and mx <= max_tol
    frames0, _, _ = ref.doppler_scan(np.zeros_like(field), iw, noise=noise, seed=3)
    assert abs(float(np.median(ref.line_core_shift(frames0, fit_at(centre), 5)[on]))) <= rms_tol


def test_finish_restatement_by_hand():
    raw = np.array([[0.0, 1.0, 2.0, np.nan], [4.0, 5.0, 6.0, 7.0]], dtype=np.float32)
    v, png = ref.doppler_finish(raw, 0.5, 0.0, 0.25, 3, 7, display_range=2.0)
    assert v.shape == (3, 7) and np.isnan(v[2]).all()                 # row 2 has no source row
    assert v[1, :6].tolist() == [4.25, 4.75, 5.25, 5.75, 6.25, 6.75] and np.isnan(v[1, 6])     # x = 3.25: tap 4 outside
    assert np.isnan(v[0, 4]) and v[0, 3] == np.float32(1.75)          # the NaN tap propagates
    assert png[1, 0] == np.uint16(np.rint(32768 + 4.25 * 32767 / 2.0).clip(1, 65535)) and png[2, 0] == 0
    masked, _ = ref.doppler_finish(raw, 0.5, 0.0, 0.25, 2, 6, circle=(1.0, 1.0, 1.0))
    assert np.isnan(masked[0, [0, 2, 3]]).all() and masked[0, 1] == v[0, 1] and masked[1, 2] == v[1, 2]
    cropped, _ = ref.doppler_finish(raw, 0.5, 0.0, 0.25, 2, 6, crop=(8, 1, 3, 4))
    assert cropped.shape == (2, 8) and np.isnan(cropped[:, [0, 1, 2, 7]]).all()
    assert np.array_equal(cropped[:, 3:7], v[:2, 1:5], equal_nan=True)


def test_fits_float32_round_trip_and_the_other_writers_unchanged(tmp_path):
    from solex_ser_recon_en_amd import fits_io
    hdr = {'BIN1': 1, 'BIN2': 1, 'EXPTIME': 0, 'NAXIS1': 5}
    a16 = np.arange(35, dtype=np.uint16).reshape(5, 7) * 1871
    a64 = np.linspace(-3, 5, 35).reshape(5, 7) / 7.0
    # the bytes the writer gave for these before it learnt float32
    assert hashlib.sha256(fits_io.fits_bytes(a16, hdr)).hexdigest() == '34f264f02e90fef7a07a7854338f8283c44890440edfd0b693ef331859ba6c93'
    assert hashlib.sha256(fits_io.fits_bytes(a64, hdr)).hexdigest() == '27455d90ac817afdbc415429a0ed90e32e79fe9823a0800ca11ea970e125f092'
    a32 = (a64 * 3).astype(np.float32)
    a32[1, 2] = np.nan
    data = fits_io.fits_bytes(a32, dict(hdr, BUNIT='km/s'))
    assert len(data) % 2880 == 0
    assert b'BITPIX  =                  -32' in data[:2880] and b"BUNIT   = 'km/s    '" in data[:2880]
    body = data[2880:2880 + a32.size * 4]
    assert body == a32.astype('>f4').tobytes()
    path = tmp_path / 'm.fits'
    fits_io.write_fits(str(path), a32, dict(hdr, BUNIT='pixel'))
    back, cards = fits_io.read_fits_f32(str(path))
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), a32.view(np.uint32))
    assert cards['BUNIT'] == "'pixel   '" and cards['NAXIS1'] == '7' and cards['NAXIS2'] == '5'
    fits_io.write_fits(str(path), a32, dict(hdr, BUNIT='km/s', NOTE="it's a/b"))
    assert fits_io.read_fits_f32(str(path))[1]['BUNIT'] == "'km/s    '"
    assert fits_io.read_fits_f32(str(path))[1]['NOTE'] == "'it''s a/b'"


# ---- the CLI's argument errors (no GPU: they are refused before the scan is read) ----
@pytest.fixture
def doppler():
    from solex_ser_recon_en_amd import doppler
    return doppler


@pytest.mark.parametrize('argv, message', [
    (['scan.ser', '--half-width', '0'], '--half-width'),
    (['scan.ser', '--half-width', '33'], '--half-width'),
    (['scan.ser', '--dispersion', '0.05'], '--dispersion and --wavelength'),
    (['scan.ser', '--wavelength', '6562.8'], '--dispersion and --wavelength'),
    (['scan.ser', '--atlas', 'alps.npz'], '--atlas and --anchor'),
    (['scan.ser', '--dispersion', '0.05', '--wavelength', '6562.8', '--atlas', 'a.npz', '--anchor', '6562.8'], 'exclude'),
    (['scan.ser', '--dispersion', '-1', '--wavelength', '6562.8'], 'positive'),
    (['scan.ser', '--range', '0'], '--range'),
    (['scan.ser', '-w', '3'], '-w'),
    (['--half-width', '4'], 'exactly one'),
    (['a.ser', 'b.ser'], 'exactly one'),
    (['missing_scan.ser'], 'no such file'),
])
def test_cli_argument_errors(doppler, capsys, argv, message):
    with pytest.raises(SystemExit) as e:
        doppler.main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_cli_refuses_torchrun(doppler, capsys, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        doppler.main(['scan.ser'])
    assert e.value.code == 2 and 'single-process' in capsys.readouterr().err


def test_library_argument_errors(doppler):
    with pytest.raises(ValueError, match='half_width'):
        doppler.dopplergram('scan.ser', half_width=40)
    with pytest.raises(ValueError, match='both'):
        doppler.dopplergram('scan.ser', dispersion=0.05)
    assert doppler.velocity_factor(0.05, 6562.808) == (0.05 / 6562.808) * ref.C_KM_S
