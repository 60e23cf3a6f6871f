"""The line-profile maps without a GPU: the NumPy restatement (tests/linemaps_ref.py) on hand-built profiles, one plane and one
NaN rule at a time, its accuracy on a scan with injected fields (the tolerance the GPU tests hold line_profile_maps() to), the
display planes, and the CLI's argument errors."""
import numpy as np
import pytest

from tests import linemaps_ref as ref
from tests.linemaps_util import fit_at, one_row_scan, parabola

IW = 40


def planes(prof, centre, half_width=5, shift=0, rows=1):
    """the five planes (dict of float32 [rows, n]) of a one_row_scan of profiles prof [rows, n, iw] with the line at centre[y]"""
    prof = np.asarray(prof, dtype=np.uint16)
    frames = one_row_scan(prof)
    out = ref.line_profile(frames, fit_at(centre, frames.shape[2]), half_width, shift)[:, :rows]
    return dict(zip(ref.PLANES, out))


def single(p, centre=20.0, half_width=5, shift=0):
    return {k: v[0, 0] for k, v in planes(np.asarray(p)[None, None, :], [centre], half_width, shift).items()}


def test_core_of_an_exact_parabola():
    # 4 j^2 - 162 j + 2000: vertex 20.25, value 2000 - 162^2 / 16 = 359.75, and the three-point parabola is the profile itself
    got = single(parabola(IW, 4, -162, 2000))
    assert got['core'] == np.float32(359.75) and got['shift'] == np.float32(0.25)


def test_width_of_a_triangle():
    # a V of slope 200 with its tip at 20, flat at 2000 beyond +-10: core 0, half level 1000, crossings at 15 and 25 exactly
    j = np.arange(IW)
    p = np.minimum(200 * np.abs(j - 20), 2000)
    got = single(p, half_width=15)
    assert got['core'] == 0.0 and got['width'] == np.float32(10.0)
    p[15] = 1100          # the left crossing interpolates between j = 15 (1100) and 16 (800): 15 + 100 / 300
    assert single(p, half_width=15)['width'] == np.float32(25.0 - (15.0 + 100.0 / 300.0))


def test_cog_of_a_symmetric_profile_is_its_centre():
    j = np.arange(IW)
    p = (3000 - 1500 * np.exp(-0.5 * ((j - 21) / 2.5) ** 2)).round()
    got = single(p, centre=21.3, half_width=8)
    assert got['cog'] == np.float32(21.0 - 21.3)
    assert planes(np.stack([p[None, :]] * 3), [21.3, 21.0, 21.9], 8, rows=3)['cog'][:, 0].tolist() == \
        [np.float32(21.0 - 21.3), np.float32(0.0), np.float32(21.0 - 21.9)]


def test_ew_of_a_known_profile():
    # continuum 1000 at both ends of [15, 25], a box of depth 600 over five samples: sum(1 - p / 1000) = 5 * 0.6
    p = np.full(IW, 1000)
    p[18:23] = 400
    got = single(p)
    assert got['ew'] == np.float32(3.0)
    p[15] = 1400          # continuum (1400 + 1000) / 2 = 1200: (11 * 2400 - 2 * (1400 + 5 * 1000 + 5 * 400)) / 2400
    assert single(p)['ew'] == np.float32((11 * 2400 - 2 * 8400) / 2400.0)


def test_unbracketed_minimum_leaves_cog_and_ew():
    p = parabola(IW, 1, -2 * 14, 400)          # minimum on lo = 15
    got = single(p, 20.4)
    assert np.isnan([got['shift'], got['core'], got['width']]).all()
    assert np.isfinite([got['cog'], got['ew']]).all()


def test_no_half_level_crossing_is_nan():
    # window [15, 25], continuum (1000 + 9000) / 2 = 5000, core 500, half 2750: nothing left of j* = 20 reaches it
    p = np.full(IW, 1200)
    p[15], p[20], p[25] = 1000, 500, 9000
    got = single(p)
    assert got['core'] == np.float32(500.0) and np.isnan(got['width'])
    q = p[::-1].copy()                          # mirrored about 19.5: window [14, 24] around 19, nothing right of j* = 19
    got = single(q, 19.0)
    assert got['core'] == np.float32(500.0) and np.isnan(got['width'])
    q[16] = 2750                                # >= half on the left does not help the right
    assert np.isnan(single(q, 19.0)['width'])
    p[17] = 2750                                # both crossings: p(17) = half exactly, so xl = 17
    assert single(p)['width'] == np.float32((25.0 - (9000 - 2750) / (9000 - 1200)) - 17.0)


def test_minimum_not_below_half_is_nan():
    # continuum (2001 + 2001) / 2 just above p(j*) = 2000, core 2000 - 7000^2 / (8 * 7000) = 1125: half = 1563 <= p(j*)
    p = np.full(IW, 5000)
    p[15], p[25] = 2001, 2001
    p[19:22] = [9000, 2000, 2000]
    got = single(p)
    assert got['core'] == np.float32(1125.0) and np.isnan(got['width']) and np.isfinite(got['shift'])


def test_s0_not_positive_and_c2_zero():
    p = np.full(IW, 100)
    p[15], p[25] = 0, 0                        # C2 = 0: S0 = -2 sum p < 0 -> cog NaN, ew NaN (and the minimum is on lo)
    p[19:22] = [60, 50, 60]
    got = single(p)
    assert np.isnan([got['cog'], got['ew'], got['shift']]).all()
    q = np.full(IW, 100)                       # an emission line: S0 < 0, C2 > 0 -> cog NaN, ew negative
    q[17:24] = [150, 200, 250, 300, 250, 200, 150]
    got = single(q)
    assert np.isnan(got['cog']) and got['ew'] == np.float32((11 * 200 - 2 * (4 * 100 + 1500)) / 200.0)
    got = single(np.full(IW, 100))             # a flat profile: S0 = 11 * 200 - 2 * 1100 = 0 exactly
    assert np.isnan(got['cog']) and got['ew'] == 0.0


def test_non_finite_fit_rows():
    p = parabola(IW, 4, -162, 2000)
    prof = np.stack([p[None, :]] * 4)
    frames = one_row_scan(prof)
    fit = fit_at([20.0] * 4, ih=frames.shape[2])
    fit[1, 0], fit[2, 0], fit[3, 3] = np.nan, np.inf, np.nan
    got = ref.line_profile(frames, fit, 5)[:, :4, 0]
    assert np.isfinite(got[:, 0]).all() and np.isnan(got[:, 1:3]).all()
    # fit[y, 3] NaN: the positions (shift, cog) are NaN, the rest is measured
    assert np.isnan(got[[0, 3], 3]).all() and np.isfinite(got[[1, 2, 4], 3]).all()


@pytest.mark.parametrize('shift, window', [(-17, (1, 8)), (-3, (12, 22)), (4, (19, 29)), (16, (31, 38)), (-16, (1, 9)),
                                           (22, None), (-23, None)])
def test_windows_with_a_shift_clip_at_the_edges(shift, window):
    assert ref.window(20.0, shift, 5, IW) == window
    # a line at 20 + shift measured around 20 + shift: the positions relative to fit[y, 3] + S are the unshifted line's
    p0 = parabola(IW, 4, -2 * 4 * 20, 4000).astype(np.int64) + 7 * np.arange(IW)
    p = np.roll(p0, shift)
    got = single(p, 20.0, 5, shift)
    if window is None:
        assert all(np.isnan(v) for v in got.values())
        return
    want = single(p0, 20.0, 5, 0)
    assert got['shift'] == pytest.approx(float(want['shift']), abs=1e-6) and got['core'] == want['core']
    assert np.isfinite(got['cog']) and got['ew'] > 0
    if window[1] - window[0] == 10:            # not clipped: the whole window moves with the line
        assert got['ew'] == want['ew'] and got['width'] == pytest.approx(float(want['width']), abs=1e-6)
        assert got['cog'] == pytest.approx(float(want['cog']), abs=1e-6)


def test_shift_plane_at_zero_is_the_dopplergram():
    from solex_ser_recon_en_amd import synth
    frames = synth.synth_frames_numpy(9, 120, 30, 16, seed=3, tilt=0.01, curv=2e-5)
    centre = synth.curve_of_row(np.arange(120, dtype=np.float64), 120, 30) + np.random.default_rng(1).uniform(-3, 3, 120)
    fit = fit_at(centre)
    for hw in (1, 5, 12):
        got = ref.line_profile(frames, fit, hw)[0]
        want = ref.line_core_shift(frames, fit, hw)
        assert np.array_equal(got.view(np.uint32)[~np.isnan(got)], want.view(np.uint32)[~np.isnan(want)])
        assert np.array_equal(np.isnan(got), np.isnan(want))


@pytest.mark.parametrize('noise', sorted(ref.TOLERANCE['profile']))
def test_restatement_recovers_injected_fields(noise):
    ih, n, iw = 400, 300, 48
    shift, sigma, depth = ref.injected_fields(ih, n)
    frames, centre, on, core = ref.profile_scan(shift, sigma, depth, iw, noise=noise, seed=3)
    for d in ref.FIT_OFFSETS:
        fit = fit_at(centre + d)
        got = ref.profile_errors(ref.line_profile(frames, fit, 10), fit, shift, sigma, depth, centre, core, on)
        print('noise %g, fit %+g px: %s' % (noise, d, got))
        for name, (rms_tol, max_tol) in ref.TOLERANCE['profile'][noise].items():
            rms, mx, nans = got[name]
            assert nans == 0 and rms <= rms_tol and mx <= max_tol, name


def test_display_planes():
    v = np.array([np.nan, -3.0, 0.0, 0.4, 1e9, 70000.0], dtype=np.float32)
    assert ref.display(v, 'core', 5, 2.0).tolist() == [0, 1, 1, 0 + 1, 65535, 65535]
    assert ref.display(v, 'width', 5, 2.0).tolist() == [0, 1, 1, int(np.rint(1 + np.float64(np.float32(0.4)) * 65534 / 11)), 65535, 65535]
    assert ref.display(v, 'cog', 5, 2.0).tolist() == [0, 1, 32768, int(np.rint(32768 + np.float64(np.float32(0.4)) * 32767 / 2)), 65535, 65535]
    raw = np.stack([np.arange(12, dtype=np.float32).reshape(3, 4) + q for q in range(5)])
    maps, png = ref.line_profile_finish(raw, 1.0, 0.0, 0.0, 3, 4, half_width=5, display_range=2.0)
    assert np.array_equal(maps, raw) and png[1].tolist() == np.clip(raw[1], 1, None).astype(np.uint16).tolist()


# ---- the CLI's argument errors (no GPU: they are refused before the scan is read) ----
@pytest.fixture
def lineprofile():
    from solex_ser_recon_en_amd import lineprofile
    return lineprofile


@pytest.mark.parametrize('argv, message', [
    (['scan.ser', '--half-width', '0'], '--half-width'),
    (['scan.ser', '--half-width', '33'], '--half-width'),
    (['scan.ser', '--line', '5875.6'], '--line needs --atlas'),
    (['scan.ser', '--line', '5875.6', '--shift', '3', '--atlas', 'a.npz', '--anchor', '6562.8'], 'exclude'),
    (['scan.ser', '--dispersion', '0.05'], '--dispersion and --wavelength'),
    (['scan.ser', '--atlas', 'alps.npz'], '--atlas and --anchor'),
    (['scan.ser', '--dispersion', '0.05', '--wavelength', '6562.8', '--atlas', 'a.npz', '--anchor', '6562.8'], 'exclude'),
    (['scan.ser', '--line', '-1', '--atlas', 'a.npz', '--anchor', '6562.8'], 'positive'),
    (['scan.ser', '--range', '0'], '--range'),
    (['scan.ser', '-w', '3'], '-w'),
    (['--half-width', '4'], 'exactly one'),
    (['a.ser', 'b.ser'], 'exactly one'),
    (['missing_scan.ser'], 'no such file'),
])
def test_cli_argument_errors(lineprofile, capsys, argv, message):
    with pytest.raises(SystemExit) as e:
        lineprofile.main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_cli_refuses_torchrun(lineprofile, capsys, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        lineprofile.main(['scan.ser'])
    assert e.value.code == 2 and 'single-process' in capsys.readouterr().err


def test_library_argument_errors(lineprofile):
    with pytest.raises(ValueError, match='half_width'):
        lineprofile.line_profile_maps('scan.ser', half_width=40)
    with pytest.raises(ValueError, match='both'):
        lineprofile.line_profile_maps('scan.ser', dispersion=0.05)
    with pytest.raises(ValueError, match='positive'):
        lineprofile.line_profile_maps('scan.ser', display_range=0.0)
