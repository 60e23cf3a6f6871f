"""The line-profile maps on the GPU: shg_line_profile and shg_line_profile_finish bit for bit against the NumPy restatement
(tests/linemaps_ref.py) and against the Dopplergram's kernels where they overlap, line_profile_maps() recovering injected line
shift, width and depth within what the restatement achieves (linemaps_ref.TOLERANCE['profile']), and the CLI end to end."""
import os

import numpy as np
import pytest

from tests import linemaps_ref as ref
from tests.linemaps_util import IH, IW, N, SHIFT_CASES, finish_cases, fit_for, run_json, same_bits, scan_reader, upload, write_scan
from tests.spectral_util import ATLAS, atlas_npz, atlas_scan, core_wavelength  # noqa: F401  -- the g17-style atlas scan and its fixtures

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import lineprofile, ops, synth
    return lineprofile, ops, synth


@pytest.mark.parametrize('case', SHIFT_CASES, ids=['%s_s%d' % (c[0], c[-1]) for c in SHIFT_CASES])
def test_line_profile_bit_exact(mods, case):
    _, ops, synth = mods
    name, n, width, height, bits, hw, flip, sharded, pitched, shift = case
    frames = synth.synth_frames_numpy(n, width, height, bits, seed=11, tilt=0.01, curv=2e-5)
    ih, iw = max(width, height), min(width, height)
    fit = fit_for(synth, ih, iw, seed=len(name))
    stack = upload(ops, frames, bits, pitched)
    n_cols, k_offset = (n + 9, 4) if sharded else (n, 0)
    got = ops.line_profile(stack, fit, hw, shift, flip_x=flip, n_cols=n_cols, k_offset=k_offset).cpu().numpy()
    want = ref.line_profile(frames, fit, hw, shift, flip_x=flip, n_cols=n_cols, k_offset=k_offset)
    for q, plane in enumerate(ref.PLANES):
        held = want[q][:, k_offset:k_offset + n]
        print('%s S=%d %s: %d of %d NaN' % (name, shift, plane, np.isnan(held).sum(), held.size))
        assert np.isfinite(held).any()
        same_bits(got[q], want[q])
    assert np.isnan(want[2][:, k_offset:k_offset + n]).any()      # rows without a width are there
    if shift == 0:
        same_bits(got[0], ops.line_core_shift(stack, fit, hw, flip_x=flip, n_cols=n_cols, k_offset=k_offset).cpu().numpy())


def test_line_profile_c2_size(mods):
    _, ops, synth = mods
    stack = synth.synth_frames_torch(2000, 2000, 200, 16, seed=2, padded=True)
    frames = ops.stack_to_host(stack)
    fit = fit_for(synth, 2000, 200, seed=5, jitter=1.0, edges=False, nans=False)
    got = ops.line_profile(stack, fit, 12).cpu().numpy()
    want = ref.line_profile(frames, fit, 12)
    for q in range(len(ref.PLANES)):
        same_bits(got[q], want[q])
    assert np.isfinite(got[2]).mean() > 0.9
    same_bits(got[0], ops.line_core_shift(stack, fit, 12).cpu().numpy())


def test_unsupported_arguments(mods):
    _, ops, _ = mods
    stack = torch.zeros((2, 40, 300), dtype=torch.uint16, device='cuda')
    fit = np.zeros((300, 4))
    for hw in (0, 33):
        with pytest.raises(RuntimeError, match='half-width'):
            ops.line_profile(stack, fit, hw)
    for s in (42, -42):                       # 3 - iw - H < S < iw - 3 + H, iw = 40, H = 5
        with pytest.raises(RuntimeError, match='shift'):
            ops.line_profile(stack, fit, 5, s)
    ops.line_profile(stack, fit, 5, 41)
    with pytest.raises(ValueError):
        ops.line_profile(stack, np.zeros((40, 4)), 5)


@pytest.mark.parametrize('phi, ratio, shift', [(0.0, 1.0, 0.0), (0.12, 1.07, 0.0), (-0.3, 0.91, 0.0), (0.05, 1.2, 37.5)])
def test_finish_matches_doppler_finish_and_the_restatement(mods, phi, ratio, shift):
    _, ops, _ = mods
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    rng = np.random.default_rng(3)
    h, w = 300, 400
    raw = np.stack([rng.normal(0.0, 0.8, (h, w)), rng.uniform(-100, 70000, (h, w)), rng.uniform(-1, 13, (h, w)),
                    rng.normal(0.0, 3.0, (h, w)), rng.uniform(-2, 12, (h, w))]).astype(np.float32)
    raw[rng.random(raw.shape) < 0.05] = np.nan
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(phi, ratio, h, w)
    h00, h01, h02 = mat3[0, 0], mat3[0, 1], mat3[0, 2] + shift
    rt = torch.empty((5, h, w + 12), dtype=torch.float32, device='cuda')[:, :, :w]
    rt.copy_(torch.from_numpy(raw))
    for name, circle, opts in finish_cases():
        crop, _ = crop_plan(out_h, out_w, circle if circle is not None else (-1, -1, -1), opts)
        maps, png = ops.line_profile_finish(rt, h00, h01, h02, out_h, out_w, circle, crop, 6, 1.7)
        want, want_png = ref.line_profile_finish(raw, h00, h01, h02, out_h, out_w, circle, crop, 6, 1.7)
        maps, png = maps.cpu().numpy(), png.cpu().numpy()
        for q in range(5):
            one, _ = ops.doppler_finish(rt[q], h00, h01, h02, out_h, out_w, circle, crop)
            same_bits(maps[q], one.cpu().numpy())
            same_bits(maps[q], want[q])
        assert np.array_equal(png, want_png), name
        maps2, none = ops.line_profile_finish(rt, h00, h01, h02, out_h, out_w, circle, crop)
        assert none is None
        same_bits(maps2.cpu().numpy(), want)


# ---- line_profile_maps() on a scan with known fields ----
@pytest.mark.parametrize('noise', sorted(ref.TOLERANCE['profile']))
def test_maps_recover_injected_fields(mods, noise):
    lineprofile, _, _ = mods
    shift, sigma, depth = ref.injected_fields(IH, N)
    frames, centre, on, core = ref.profile_scan(shift, sigma, depth, IW, noise=noise, seed=3)
    res = lineprofile.line_profile_maps(scan_reader(frames))
    raw = np.stack([res['raw'][p] for p in ref.PLANES])
    want = ref.line_profile(frames, res['fit'], 10)
    for q in range(5):
        same_bits(raw[q], want[q])
    # against the truth: the scan's own fitted line, not the exact centre, is the reference position
    got = ref.profile_errors(raw, res['fit'], shift, sigma, depth, centre, core, on)
    print('noise %g: %s; circle %s' % (noise, got, res['circle']))
    for name, (rms_tol, max_tol) in ref.TOLERANCE['profile'][noise].items():
        rms, mx, nans = got[name]
        assert nans == 0 and rms <= rms_tol and mx <= max_tol, name
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(res['phi'], res['ratio'], IH, N)
    maps, png = ref.line_profile_finish(raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, res['circle'], None, 10, 2.0)
    for q, p in enumerate(ref.PLANES):
        same_bits(res['maps'][p], maps[q])
        assert np.array_equal(res['png'][p], png[q]), p
    assert res['units'] == {'shift': 'pixel', 'core': 'adu', 'width': 'pixel', 'cog': 'pixel', 'ew': 'pixel'}
    kms = lineprofile.line_profile_maps(scan_reader(frames), dispersion=0.05, wavelength=6562.8)
    assert kms['units']['cog'] == 'km/s' and kms['units']['width'] == 'pixel'
    same_bits(kms['maps']['cog'], (maps[3].astype(np.float64) * ((0.05 / 6562.8) * 299792.458)).astype(np.float32))
    same_bits(kms['maps']['width'], maps[2])


def test_maps_of_a_shifted_line_keep_the_geometry(mods):
    lineprofile, _, _ = mods
    shift, sigma, depth = ref.injected_fields(IH, N)
    frames, _, _, _ = ref.profile_scan(shift, sigma, depth, IW, noise=0.004, seed=3)
    base = lineprofile.line_profile_maps(scan_reader(frames), half_width=4)
    moved = lineprofile.line_profile_maps(scan_reader(frames), half_width=4, shift=-15)
    assert moved['circle'] == base['circle'] and moved['ratio'] == base['ratio'] and moved['shift'] == -15
    assert moved['maps']['ew'].shape == base['maps']['ew'].shape
    same_bits(np.stack([moved['raw'][p] for p in ref.PLANES]), ref.line_profile(frames, moved['fit'], 4, -15))
    # 15 px into the continuum there is no line: the equivalent width is far below the line's
    on = np.isfinite(base['maps']['ew']) & np.isfinite(moved['maps']['ew'])
    assert np.median(moved['maps']['ew'][on]) < 0.2 * np.median(base['maps']['ew'][on])


# ---- the command line ----
@pytest.fixture(scope='module')
def scan_file(tmp_path_factory):
    return write_scan(tmp_path_factory, 'lineprofile', ref.profile_scan(*ref.injected_fields(IH, N), IW, noise=0.004, seed=4)[0])


def test_cli_end_to_end(mods, scan_file, capsys):
    lineprofile, _, _ = mods
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    got = run_json(lineprofile.main, capsys, [scan_file, '--half-width', '8', '--shift', '2', '--range', '1.5'])
    res = lineprofile.line_profile_maps(scan_file, half_width=8, shift=2, display_range=1.5)
    assert sorted(got['fits']) == sorted(lineprofile.WRITTEN) and got['shift'] == 2
    base = os.path.splitext(scan_file)[0]
    for name in lineprofile.WRITTEN:
        assert got['fits'][name] == base + '_shift=2_line_%s.fits' % name and got['png'][name] == base + '_shift=2_line_%s.png' % name
        m, cards = read_fits_f32(got['fits'][name])
        same_bits(m, res['maps'][name])
        assert cards['HALFWID'] == '8' and cards['SHIFT'] == '2' and cards['BUNIT'].strip("' ") == res['units'][name]
        assert np.array_equal(read_png_gray(got['png'][name]), res['png'][name])
        assert got['shape'] == list(m.shape) and got['valid_fraction'][name] > 0.9
    assert not os.path.exists(base + '_shift=2_line_shift.fits')
    assert 0 < got['median']['width'] < 17 and got['median']['core'] > 0


@pytest.mark.parametrize('flags', [['-s'], ['-r', '300']])
def test_cli_maps_have_the_products_shape(mods, scan_file, capsys, tmp_path, flags):
    lineprofile, _, _ = mods
    import shutil
    from solex_ser_recon_en_amd import SHG_MAIN, outputs
    from solex_ser_recon_en_amd.png_io import read_png_gray
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir()
    b.mkdir()
    shutil.copy(scan_file, a / 'scan.ser')
    shutil.copy(scan_file, b / 'scan.ser')
    got = run_json(lineprofile.main, capsys, [str(a / 'scan.ser')] + flags)
    assert SHG_MAIN.main(['-c'] + flags + [str(b / 'scan.ser')]) == 0
    outputs.flush()
    clahe = read_png_gray(str(b / 'scan_shift=0_clahe.png'))
    for name in lineprofile.WRITTEN:
        assert got['shape'] == list(clahe.shape) == list(read_png_gray(got['png'][name]).shape)


def test_cli_line_takes_the_analysers_shift(mods, atlas_npz, atlas_scan, capsys):
    lineprofile, _, _ = mods
    from solex_ser_recon_en_amd import spectral
    from solex_ser_recon_en_amd.video_reader import video_reader
    path, anchor = atlas_scan, core_wavelength(atlas_npz)
    a = spectral.analyse(path)
    disp = spectral.auto_dispersion(a['spectrum2'], a['anchor_x'], anchor, spectral.load_atlas(ATLAS))[0]
    line = anchor + 9.0 * disp
    want, _ = spectral.shift_for_wavelength(line, anchor, disp, a['fit'], int(video_reader(path).iw))
    got = run_json(lineprofile.main, capsys, [path, '--atlas', ATLAS, '--anchor', repr(anchor), '--line', repr(line), '--half-width', '3'])
    assert got['shift'] == want != 0 and got['dispersion'] == disp and got['wavelength'] == line
    assert got['units']['cog'] == 'km/s' and got['fits']['ew'].endswith('_shift=%d_line_ew.fits' % want)
