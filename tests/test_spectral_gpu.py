"""The spectral analyser on the GPU (shg_atlas_correlate): interpolated rows bit-exact to np.interp, correlations against the
NumPy restatement (tests/spectral_ref.py) and g17, the size limits, and the CLI end to end on a synthetic scan whose spectral
axis is the atlas at a known dispersion, --process included."""
import json
import os
import shutil

import numpy as np
import pytest

from tests import spectral_ref as ref
from tests.spectral_util import ATLAS, H_ALPHA, IW, TRUE_DISPERSION, atlas_npz, atlas_scan, core_wavelength  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

CASES = ['ha200', 'ha600', 'na600', 'ha_edge', 'ha_right']


@pytest.fixture(scope='module')
def spectral():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import spectral
    return spectral


def atlas_spectrum(atlas_npz, w, anchor_wavelength, dispersion, anchor_x, seed=0):
    p = np.arange(w, dtype=np.float64)
    prof = np.interp(anchor_wavelength + (p - anchor_x) * dispersion, atlas_npz['a'], atlas_npz['yv'])
    noise = np.random.default_rng(seed).normal(0.0, 0.004, w)
    return np.clip(np.rint(50000.0 * (prof * (1.0 + 0.1 * (p / w - 0.5)) + noise)), 1, 65535).astype(np.uint16)


def check_rows(spectral, atlas_npz, s2, ax, lam, scales, idx):
    with np.errstate(invalid='ignore', divide='ignore'):
        return _check_rows(spectral, atlas_npz, s2, ax, lam, scales, idx)


def _check_rows(spectral, atlas_npz, s2, ax, lam, scales, idx):
    corr, rows = spectral.correlate(s2, ax, lam, spectral.load_atlas(ATLAS), scales, row_guesses=idx)
    lspec = ref.log_spectrum(s2, ax)
    for r, i in enumerate(idx):
        want = ref.interp_row(atlas_npz['a'], atlas_npz['yv'], lam, ax, scales[i], s2.shape[0])
        assert np.array_equal(rows[r].view(np.uint64), want.view(np.uint64)), 'guess %d: row differs from np.interp' % i
        c = np.corrcoef(want, lspec)[0, 1]
        assert (np.isnan(c) and np.isnan(corr[i])) or abs(corr[i] - c) <= 1e-12
    return corr


@pytest.mark.parametrize('case', CASES)
def test_matches_g17(spectral, atlas_npz, golden, case):
    g = golden('g17_spectral')
    s2, ax, lam = g[case + '_spectrum2'], float(g[case + '_anchor_x']), float(g[case + '_anchor_wavelength'])
    want = g[case + '_corr']
    idx = sorted(set(np.linspace(0, want.shape[0] - 1, 9).astype(int).tolist() + [int(g[case + '_index'])]))
    corr = check_rows(spectral, atlas_npz, s2, ax, lam, g[case + '_scales'], idx)
    err = np.abs(corr - want)
    print('%s: max |corr - reference| = %.2e over %d guesses' % (case, err.max(), corr.shape[0]))
    assert err.max() <= 1e-12
    top2 = np.sort(want)[-2:]
    if top2[1] - top2[0] > 1e-9:
        assert int(np.argmax(corr)) == int(g[case + '_index'])
    disp, corr2, scales = spectral.auto_dispersion(s2, ax, lam, spectral.load_atlas(ATLAS))
    assert np.array_equal(scales, g[case + '_scales']) and np.array_equal(corr2, corr)
    assert disp == scales[int(g[case + '_index'])]


@pytest.mark.parametrize('w, dispersion, ax', [(2, 0.05, 0.5), (37, 0.05, 20.2), (1000, 0.03, 511.7), (2000, 0.02, 1999.4),
                                               (8192, 0.012, 4100.3)])
def test_rows_bit_exact_up_to_8192(spectral, atlas_npz, w, dispersion, ax):
    s2 = atlas_spectrum(atlas_npz, w, H_ALPHA, dispersion, ax, seed=w)
    scales = ref.scale_guesses(w)
    idx = sorted(set(np.linspace(0, scales.shape[0] - 1, 7).astype(int).tolist()))
    corr = check_rows(spectral, atlas_npz, s2, ax, H_ALPHA, scales, idx)
    if w > 2:                 # (two pixels, one of them the filled window: often a zero variance, NaN as in NumPy)
        assert np.isfinite(corr).all() and (np.abs(corr) <= 1).all()


def test_unsupported_width(spectral):
    s2 = np.full(8193, 1000, dtype=np.uint16)
    with pytest.raises(RuntimeError, match='above the supported'):
        spectral.correlate(s2, 4000.0, H_ALPHA, spectral.load_atlas(ATLAS), np.array([0.05]))


def test_empty_run_raises(spectral):
    """An anchor at the atlas's last point with the line at pixel 0: every other point lies left of the frame."""
    at = spectral.load_atlas(ATLAS)
    s2 = np.full(100, 1000, dtype=np.uint16)
    with pytest.raises(ValueError, match='no atlas point'):
        spectral.correlate(s2, -50.0, at.a_last, at, np.array([0.05, 0.06]))


# ---- end to end: a scan whose spectral axis is the atlas (spectral_util.atlas_scan) -------------------------------------
def run_cli(spectral, capsys, argv):
    capsys.readouterr()
    assert spectral.main(argv) == 0
    out = capsys.readouterr().out
    return json.loads(next(line for line in out.splitlines() if line.startswith('{')))


def test_cli_recovers_the_dispersion(spectral, atlas_npz, atlas_scan, capsys):
    # The line fit's column on the middle row sits ~1.7 px off the core (the atlas's H-alpha core is asymmetric and the fit
    # works on a blurred trace): the anchor is the wavelength the scan really has at that column, as a user would name it.
    res = spectral.analyse(atlas_scan)
    anchor = core_wavelength(atlas_npz) + (res['anchor_x'] - IW / 2.0) * TRUE_DISPERSION
    targets = [6559.58, 6563.5, 6567.0]
    argv = [atlas_scan, '--atlas', ATLAS, '--anchor', repr(anchor)] + [a for t in targets for a in ('--goto', str(t))]
    got = run_cli(spectral, capsys, argv)
    step = 0.1 / (3 * IW - 1)
    print('recovered %.6f (truth %.4f, guess step %.2e), anchor_x %.3f' % (got['dispersion'], TRUE_DISPERSION, step, got['anchor_x']))
    assert abs(got['dispersion'] - TRUE_DISPERSION) <= step
    assert got['anchor_x'] == res['anchor_x'] and got['dispersion_rounded'] == round(got['dispersion'], 6)
    want_disp, corr, _ = ref.auto_dispersion(res['spectrum2'], res['anchor_x'], anchor, dict(np.load(ATLAS)))
    top2 = np.sort(corr)[-2:]
    if top2[1] - top2[0] > 1e-9:
        assert got['dispersion'] == want_disp
    for t, item in zip(targets, got['targets']):
        shift, within = ref.shift_for_wavelength(t, anchor, got['dispersion'], res['fit'], IW)
        assert item == {'wavelength': t, 'shift': shift, 'partial': bool(not within.all())}
    # --dispersion skips the fit
    fixed = run_cli(spectral, capsys, argv + ['--dispersion', '0.05'])
    assert fixed['dispersion'] == 0.05 and fixed['targets'][0]['shift'] == int((6559.58 - anchor) / 0.05)


def test_cli_process_matches_shg_main(spectral, atlas_npz, atlas_scan, capsys, tmp_path):
    from solex_ser_recon_en_amd import SHG_MAIN, outputs
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir()
    b.mkdir()
    shutil.copy(atlas_scan, a / 'scan.ser')
    shutil.copy(atlas_scan, b / 'scan.ser')
    got = run_cli(spectral, capsys, [str(a / 'scan.ser'), '--atlas', ATLAS, '--anchor', repr(core_wavelength(atlas_npz)), '--goto', '6559.58',
                                     '--goto', '6564.0', '--process', '-c'])
    outputs.flush()
    shifts = ','.join(str(t['shift']) for t in got['targets'])
    assert SHG_MAIN.main(['-c', '-w', shifts, str(b / 'scan.ser')]) == 0
    outputs.flush()
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert any('shift=%d' % got['targets'][0]['shift'] in n for n in names)
    for n in names:
        if n.endswith('_log.txt'):          # its first line is the start time
            continue
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
