"""The Dopplergram on the GPU: shg_line_core_shift and shg_doppler_finish bit for bit against the NumPy restatement
(tests/linemaps_ref.py), dopplergram() recovering an injected velocity field within what the restatement achieves
(linemaps_ref.TOLERANCE['doppler']), and the CLI end to end: FITS, PNG, geometry, the products' shape, --atlas."""
import numpy as np
import pytest

from tests import linemaps_ref as ref
from tests.linemaps_util import CASES, IH, IW, N, finish_cases, fit_for, run_json, same_bits, scan_reader, upload, write_scan
from tests.spectral_util import ATLAS, atlas_npz, atlas_scan, core_wavelength  # noqa: F401  -- the g17-style atlas scan and its fixtures

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import doppler, ops, synth
    return doppler, ops, synth


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_line_core_shift_bit_exact(mods, case):
    _, ops, synth = mods
    name, n, width, height, bits, hw, flip, sharded, pitched = case
    frames = synth.synth_frames_numpy(n, width, height, bits, seed=11, tilt=0.01, curv=2e-5)
    ih, iw = max(width, height), min(width, height)
    fit = fit_for(synth, ih, iw, seed=len(name))
    stack = upload(ops, frames, bits, pitched)
    n_cols, k_offset = (n + 9, 4) if sharded else (n, 0)
    got = ops.line_core_shift(stack, fit, hw, flip_x=flip, n_cols=n_cols, k_offset=k_offset)
    want = ref.line_core_shift(frames, fit, hw, flip_x=flip, n_cols=n_cols, k_offset=k_offset)
    got = got.cpu().numpy()
    print('%s: %d of %d NaN' % (name, np.isnan(want).sum(), want.size))
    held = want[:, k_offset:k_offset + n]
    assert 0 < np.isnan(held).sum() < held.size       # both kinds of sample are there
    same_bits(got, want)


def test_line_core_shift_c2_size(mods):
    _, ops, synth = mods
    stack = synth.synth_frames_torch(2000, 2000, 200, 16, seed=2, padded=True)
    frames = ops.stack_to_host(stack)
    fit = fit_for(synth, 2000, 200, seed=5, jitter=1.0, edges=False, nans=False)
    got = ops.line_core_shift(stack, fit, 5).cpu().numpy()
    same_bits(got, ref.line_core_shift(frames, fit, 5))
    assert np.isfinite(got).mean() > 0.9


def test_unsupported_arguments(mods):
    _, ops, _ = mods
    stack = torch.zeros((2, 40, 300), dtype=torch.uint16, device='cuda')
    fit = np.zeros((300, 4))
    for hw in (0, 33):
        with pytest.raises(RuntimeError, match='half-width'):
            ops.line_core_shift(stack, fit, hw)
    with pytest.raises(ValueError):
        ops.line_core_shift(stack, np.zeros((40, 4)), 5)


@pytest.mark.parametrize('phi, ratio, shift', [(0.0, 1.0, 0.0), (0.12, 1.07, 0.0), (-0.3, 0.91, 0.0), (0.05, 1.2, 37.5), (0.0, 1.0, -90.25)])
def test_doppler_finish_bit_exact(mods, phi, ratio, shift):
    _, ops, _ = mods
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    rng = np.random.default_rng(3)
    h, w = 400, 500
    raw = rng.normal(0.0, 0.8, (h, w)).astype(np.float32)
    raw[rng.random((h, w)) < 0.05] = np.nan
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(phi, ratio, h, w)
    h00, h01, h02 = mat3[0, 0], mat3[0, 1], mat3[0, 2] + shift       # a shifted transform: taps outside on one side
    rt = torch.empty((h, w + 12), dtype=torch.float32, device='cuda')[:, :w]
    rt.copy_(torch.from_numpy(raw))
    for name, circle, opts in finish_cases():
        crop, _ = crop_plan(out_h, out_w, circle if circle is not None else (-1, -1, -1), opts)
        got, png = ops.doppler_finish(rt, h00, h01, h02, out_h, out_w, circle, crop, 1.7)
        want, want_png = ref.doppler_finish(raw, h00, h01, h02, out_h, out_w, circle, crop, 1.7)
        same_bits(got.cpu().numpy(), want)
        assert np.array_equal(png.cpu().numpy(), want_png), name
        got2, none = ops.doppler_finish(rt, h00, h01, h02, out_h, out_w, circle, crop)
        assert none is None
        same_bits(got2.cpu().numpy(), want)


# ---- dopplergram() on a scan with a known velocity field ----
@pytest.mark.parametrize('noise', sorted(ref.TOLERANCE['doppler']))
def test_dopplergram_recovers_an_injected_field(mods, noise):
    doppler, _, _ = mods
    rms_tol, max_tol = ref.TOLERANCE['doppler'][noise]
    field = ref.injected_field(IH, N)
    frames, centre, on = ref.doppler_scan(field, IW, noise=noise, seed=3)
    res = doppler.dopplergram(scan_reader(frames))
    same_bits(res['raw'], ref.line_core_shift(frames, res['fit'], 5))
    # the shift is relative to the scan's own fitted line: compare where the line core is
    pos = res['raw'].astype(np.float64) + res['fit'][:, 3:4]
    err = (pos - (centre[:, None] + field))[on]
    rms, mx = float(np.sqrt(np.mean(err * err))), float(np.abs(err).max())
    print('noise %g: RMS %.4f, max %.4f px over %d disk samples; circle %s' % (noise, rms, mx, err.size, res['circle']))
    assert not np.isnan(err).any() and rms <= rms_tol and mx <= max_tol
    assert res['units'] == 'pixel' and res['circle'] != (-1, -1, -1)
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(res['phi'], res['ratio'], IH, N)
    want, want_png = ref.doppler_finish(res['raw'], mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, res['circle'], None, 2.0)
    same_bits(res['map'], want)
    assert np.array_equal(res['png'], want_png)
    kms = doppler.dopplergram(scan_reader(frames), dispersion=0.05, wavelength=6562.8)
    assert kms['units'] == 'km/s'
    same_bits(kms['map'], (want.astype(np.float64) * ((0.05 / 6562.8) * ref.C_KM_S)).astype(np.float32))


@pytest.mark.parametrize('noise', sorted(ref.TOLERANCE['doppler']))
def test_dopplergram_of_a_still_scan(mods, noise):
    doppler, _, _ = mods
    frames, _, _ = ref.doppler_scan(np.zeros((IH, N)), IW, noise=noise, seed=3)
    res = doppler.dopplergram(scan_reader(frames))
    stats = doppler.disk_stats(res)
    print('noise %g: %s' % (noise, stats))
    assert stats['valid_fraction'] > 0.95 and abs(stats['median']) <= ref.TOLERANCE['doppler'][noise][0]


# ---- the command line ----
@pytest.fixture(scope='module')
def scan_file(tmp_path_factory):
    return write_scan(tmp_path_factory, 'doppler', ref.doppler_scan(ref.injected_field(IH, N), IW, noise=0.004, seed=4)[0])


def test_cli_end_to_end(mods, scan_file, capsys):
    doppler, _, _ = mods
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.device import DeviceImage
    from solex_ser_recon_en_amd.ellipse_to_circle import ellipse_to_circle
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    from solex_ser_recon_en_amd.solex_util import compute_mean_return_fit, extract_disks
    from solex_ser_recon_en_amd.fits_io import make_header
    from solex_ser_recon_en_amd.video_reader import video_reader
    got = run_json(doppler.main, capsys, [scan_file, '--range', '1.5', '--half-width', '6'])
    res = doppler.dopplergram(scan_file, half_width=6, display_range=1.5)
    m, cards = read_fits_f32(got['fits'])
    same_bits(m, res['map'])
    assert cards['BUNIT'] == "'pixel   '" and cards['HALFWID'] == '6' and got['units'] == 'pixel'
    png = read_png_gray(got['png'])
    with np.errstate(invalid='ignore'):
        q = np.clip(np.rint(32768.0 + m.astype(np.float64) * (32767.0 / 1.5)), 1, 65535)
    assert np.array_equal(png, np.where(np.isnan(m), 0, q).astype(np.uint16))
    assert got['shape'] == list(m.shape) and 0.95 < got['valid_fraction'] <= 1.0
    assert got['p1'] < got['median'] < got['p99']
    # the geometry is ellipse_to_circle's on the ellipse-fit shift's disk
    opts = dict(SHG_MAIN.default_options(), _nolog=True)
    rdr = video_reader(scan_file)
    _, fit, _, _ = compute_mean_return_fit(rdr, opts, make_header(rdr), rdr.iw, rdr.ih, '')
    disk = extract_disks(rdr, fit, [opts['ellipse_fit_shift']])[0]
    _, circle, ratio, phi, _ = ellipse_to_circle(DeviceImage(disk), opts, '', need_image=False)
    assert got['ratio'] == ratio and got['phi'] == phi and got['circle'] == [float(c) for c in circle]


@pytest.mark.parametrize('flags', [['-s'], ['-r', '300'], ['-m', '-r', '260'], ['-x']])
def test_cli_map_has_the_products_shape(mods, scan_file, capsys, tmp_path, flags):
    doppler, _, _ = mods
    import shutil
    from solex_ser_recon_en_amd import SHG_MAIN, outputs
    from solex_ser_recon_en_amd.png_io import read_png_gray
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir()
    b.mkdir()
    shutil.copy(scan_file, a / 'scan.ser')
    shutil.copy(scan_file, b / 'scan.ser')
    got = run_json(doppler.main, capsys, [str(a / 'scan.ser')] + flags)
    assert SHG_MAIN.main(['-c'] + flags + [str(b / 'scan.ser')]) == 0
    outputs.flush()
    clahe = read_png_gray(str(b / 'scan_shift=0_clahe.png'))
    assert got['shape'] == list(clahe.shape) == list(read_png_gray(got['png']).shape)
    if '-x' in flags:
        assert got['circle'] == [-1, -1, -1] and got['valid_fraction'] > 0.5


def test_cli_atlas_gives_the_analysers_dispersion(mods, atlas_npz, atlas_scan, capsys):
    doppler, _, _ = mods
    from solex_ser_recon_en_amd import spectral
    path, anchor = atlas_scan, core_wavelength(atlas_npz)
    got = run_json(doppler.main, capsys, [path, '--atlas', ATLAS, '--anchor', repr(anchor)])
    a = spectral.analyse(path)
    want = spectral.auto_dispersion(a['spectrum2'], a['anchor_x'], anchor, spectral.load_atlas(ATLAS))[0]
    assert got['dispersion'] == want and got['wavelength'] == anchor and got['units'] == 'km/s'
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    m, cards = read_fits_f32(got['fits'])
    assert cards['BUNIT'] == "'km/s    '"
    res = doppler.dopplergram(path, dispersion=want, wavelength=anchor)
    same_bits(m, res['map'])
