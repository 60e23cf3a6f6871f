"""The spectral analyser's host half without a GPU: the NumPy restatement against g17, the line-list parser, the shift arithmetic
of spectralAnalyserUI.py:245-258, the two ValueError deviations, the C ABI's argument checks and the CLI's argument errors."""
import ctypes
import os

import numpy as np
import pytest

from tests import spectral_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ATLAS = os.path.join(GOLDEN, 'alps.npz')


@pytest.fixture(scope='module')
def atlas_npz():
    return dict(np.load(ATLAS))


def test_atlas_axis_is_first_plus_k_d(atlas_npz):
    """What lets the kernel rebuild the atlas axis from k: NumPy's arange is first + k * d exactly, d = (first + step) - first."""
    from solex_ser_recon_en_amd import spectral
    at = spectral.load_atlas(ATLAS)
    a = ref.atlas_axis(atlas_npz['first'], atlas_npz['last'], atlas_npz['step'])
    assert at.n == a.shape[0] == atlas_npz['y'].shape[0] == 700000
    assert at.d == 0.010000000000218279
    assert np.array_equal(a, at.first + np.arange(at.n) * at.d)
    assert at.a_last == a[-1]
    assert spectral.load_atlas(ATLAS) is at                      # cached by path


@pytest.mark.parametrize('case', ['ha200', 'ha600', 'na600', 'ha_edge', 'ha_right'])
def test_restatement_reproduces_g17(golden, atlas_npz, case):
    g = golden('g17_spectral')
    s2, ax, lam = g[case + '_spectrum2'], float(g[case + '_anchor_x']), float(g[case + '_anchor_wavelength'])
    w = s2.shape[0]
    scales = ref.scale_guesses(w)
    assert np.array_equal(scales, g[case + '_scales'])
    # every guess for the small cases, every fifth and the chosen one for the large (the whole loop takes seconds in NumPy)
    idx = np.arange(3 * w) if w <= 300 else np.union1d(np.arange(0, 3 * w, 5), [int(g[case + '_index'])])
    corr, _ = ref.correlations(s2, ax, lam, atlas_npz['first'], atlas_npz['last'], atlas_npz['step'], atlas_npz['y'], scales[idx])
    assert np.array_equal(corr, g[case + '_corr'][idx])
    assert int(np.argmax(g[case + '_corr'])) == int(g[case + '_index'])


def test_parity_is_with_the_reference_not_the_truth(golden):
    """W = 200 around H-alpha: a true 0.05 A/px comes out as 0.0636 (the window is too narrow for the loop to lock on)."""
    g = golden('g17_spectral')
    assert float(g['ha200_true_dispersion']) == 0.05
    assert round(float(g['ha200_scales'][int(g['ha200_index'])]), 4) == 0.0636
    for case in ('ha600', 'na600', 'ha_edge'):
        step = 0.1 / (3 * g[case + '_spectrum2'].shape[0] - 1)
        assert abs(g[case + '_scales'][int(g[case + '_index'])] - float(g[case + '_true_dispersion'])) <= step


def test_load_lines(tmp_path):
    from solex_ser_recon_en_amd import spectral
    p = tmp_path / 'lines.txt'
    p.write_text('6562.808 H(α)\n5875.618 He(D3)\n\n3968.492 Ca(H)', encoding='utf-8')
    lam, names, labels = spectral.load_lines(str(p))
    assert lam == [6562.808, 5875.618, 3968.492]
    assert names == ['H(α)', 'He(D3)', 'Ca(H)']
    assert labels == ['H(α)(6562.808)', 'He(D3)(5875.618)', 'Ca(H)(3968.492)']


def _fit(columns):
    fit = np.zeros((len(columns), 4))
    fit[:, 3] = columns
    return fit


def test_shift_arithmetic():
    from solex_ser_recon_en_amd import spectral
    fit = _fit([95.5, 100.0, 104.25])
    # int() truncates toward zero, as the reference's does
    assert spectral.shift_for_wavelength(6563.0, 6562.808, 0.05, fit, 200) == (3, False)
    assert spectral.shift_for_wavelength(6562.6, 6562.808, 0.05, fit, 200) == (-4, False)
    # the <= edge: a position equal to iw still counts as within
    assert spectral.shift_for_wavelength(6562.808 + 100 * 0.05 + 1e-9, 6562.808, 0.05, fit, 200) == (100, True)
    assert spectral.shift_for_wavelength(6562.808 + 95.75 * 0.05, 6562.808, 0.05, _fit([104.25]), 200) == (95, False)
    assert spectral.shift_for_wavelength(6562.808 + 96 * 0.05 + 1e-9, 6562.808, 0.05, _fit([104.0]), 200) == (96, False)
    # partial: some rows leave the frame
    assert spectral.shift_for_wavelength(6562.808 - 96 * 0.05 - 1e-9, 6562.808, 0.05, fit, 200) == (-96, True)
    # outside on every row
    with pytest.raises(ValueError, match='not in the image'):
        spectral.shift_for_wavelength(6562.808 + 120 * 0.05, 6562.808, 0.05, fit, 200)
    with pytest.raises(ValueError, match='positive'):
        spectral.shift_for_wavelength(6563.0, 6562.808, 0.0, fit, 200)
    # the same decisions as the restatement
    for lam in np.linspace(6555.0, 6571.0, 41):
        shift, within = ref.shift_for_wavelength(lam, 6562.808, 0.0512, fit, 200)
        if within.any():
            assert spectral.shift_for_wavelength(lam, 6562.808, 0.0512, fit, 200) == (shift, not within.all())


def test_window_follows_the_reference_slice():
    from solex_ser_recon_en_amd import spectral
    for w in (12, 200):
        for ax in (-30.0, -7.5, -0.4, 0.0, 3.7, 99.9, w - 5.2, w - 0.5, w + 3.0, w + 30.0):
            u = np.arange(w)
            lo, hi = spectral.window(ax, w)
            assert np.array_equal(u[lo:hi], u[ref.window(ax, w)]), (w, ax)


def test_log_spectrum_matches_the_restatement():
    from solex_ser_recon_en_amd import spectral
    s2 = np.random.default_rng(3).integers(1, 65535, 300).astype(np.uint16)
    got = spectral.log_spectrum(s2, 140.6)
    assert got.dtype == np.float32
    assert np.array_equal(got, ref.log_spectrum(s2, 140.6))


def test_zero_pixel_raises(atlas_npz):
    """Deviation 1: the reference's log gives -inf, every correlation NaN and a silent 0.02."""
    from solex_ser_recon_en_amd import spectral
    s2 = np.full(50, 1000, dtype=np.uint16)
    s2[17] = 0
    with np.errstate(divide='ignore', invalid='ignore'):
        corr, scales = ref.correlations(s2, 25.0, 6562.808, atlas_npz['first'], atlas_npz['last'], atlas_npz['step'], atlas_npz['y'])
    assert np.isnan(corr).all() and scales[np.argmax(corr)] == 0.02
    with pytest.raises(ValueError, match='pixel 17'):
        spectral.correlate(s2, 25.0, 6562.808, spectral.load_atlas(ATLAS), scales)


def test_anchor_outside_the_atlas_raises(atlas_npz):
    """Deviation 2: the reference fails on min() of an empty array."""
    from solex_ser_recon_en_amd import spectral
    s2 = np.full(50, 1000, dtype=np.uint16)
    a = ref.atlas_axis(atlas_npz['first'], atlas_npz['last'], atlas_npz['step'])
    with pytest.raises(ValueError):
        ref.interp_row(a, atlas_npz['y'] / 255, 2000.0, 25.0, 0.05, 50)
    for lam in (2000.0, 10000.5):
        with pytest.raises(ValueError, match='outside the atlas'):
            spectral.auto_dispersion(s2, 25.0, lam, spectral.load_atlas(ATLAS))


def test_c_abi_argument_checks():
    """Rejected before any HIP call: runs without a GPU."""
    from solex_ser_recon_en_amd import _lib
    lib, one = _lib.lib, ctypes.c_void_p(16)
    args = lambda w, lo=0, hi=0, n_rows=0: (one, 700000, 3000.0, 0.01, 6562.8, 100.0, one, w, lo, hi, one, 3 * w, one, one, None, n_rows, None, None)
    assert lib.shg_atlas_correlate(*args(8193)) == -3
    assert 'above the supported' in _lib.last_error()
    assert lib.shg_atlas_correlate(*args(1)) == -1
    assert lib.shg_atlas_correlate(*args(200, 95, 201)) == -1
    assert lib.shg_atlas_correlate(*args(200, n_rows=2)) == -1
    a = list(args(200))
    a[0] = None
    assert lib.shg_atlas_correlate(*a) == -1 and 'null pointer' in _lib.last_error()


@pytest.mark.parametrize('argv, message', [
    (['scan.ser', '--anchor', '6562.808', '--goto', '6560'], 'required'),                            # no --atlas
    (['scan.ser', '--atlas', ATLAS, '--anchor', '6562.808'], 'required'),                           # no --goto
    (['scan.ser', '--atlas', ATLAS, '--anchor', 'H(α)', '--goto', '6560'], 'neither a wavelength'),
    (['scan.ser', '--atlas', ATLAS, '--anchor', '6562.808', '--goto', '6560', '--dispersion', '-0.05'], 'positive'),
    (['scan.ser', '--atlas', ATLAS, '--anchor', '6562.808', '--goto', '6560', '--process', '-w', '3'], 'other than -w'),
    (['nope.ser', '--atlas', ATLAS, '--anchor', '6562.808', '--goto', '6560'], 'no such file'),
])
def test_cli_argument_errors(argv, message, capsys, tmp_path, monkeypatch):
    from solex_ser_recon_en_amd import spectral
    monkeypatch.chdir(tmp_path)
    if argv[0] == 'scan.ser':
        (tmp_path / 'scan.ser').write_bytes(b'')
    with pytest.raises(SystemExit) as e:
        spectral.main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_cli_names_lines_from_lines_files(tmp_path, capsys, monkeypatch):
    from solex_ser_recon_en_amd import spectral
    lines = tmp_path / 'anchors.txt'
    lines.write_text('6562.808 H(α)\n', encoding='utf-8')
    assert spectral._wavelength('H(α)', [spectral.load_lines(str(lines))]) == 6562.808
    assert spectral._wavelength('H(α)(6562.808)', [spectral.load_lines(str(lines))]) == 6562.808
    assert spectral._wavelength('5875.618', []) == 5875.618


def test_cli_refuses_torchrun(tmp_path, capsys, monkeypatch):
    from solex_ser_recon_en_amd import spectral
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit):
        spectral.main([str(tmp_path / 'scan.ser'), '--atlas', ATLAS, '--anchor', '6562.808', '--goto', '6560'])
    assert 'single-process' in capsys.readouterr().err
