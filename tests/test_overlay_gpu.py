"""The written Dopplergram and line-profile maps overlay the written products (DESIGN sections 11 and 12), at file level, under
every flag that moves, mirrors, turns, crops or masks the image: a scan whose frames 70..99 at slit rows 120..199 are brighter
and carry the line 2 px to the red is run through SHG_MAIN and both command lines; that patch must sit on the same pixels of
`_shift=0_uncontrasted.png`, `_doppler.fits` and `_shift=0_line_cog.fits` (up to a one-pixel border), the maps' NaN must be the
products' circle (crop_plan's circle_out) and crop in the written orientation, and the maps' geometry the products'."""
import shutil

import numpy as np
import pytest

from tests.linemaps_util import IH, N, SHIFT, marked_scan, run_json, same_region, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def scan_file(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return write_scan(tmp_path_factory, 'overlay', marked_scan())


FLAGS = [('m', ['-m'], 0), ('s', ['-s'], 0), ('r_wide', ['-r', '500'], 0), ('r_narrow', ['-r', '200'], 0), ('x', ['-x'], 0),
         ('rot90', [], 90), ('rot180', [], 180), ('rot270', [], 270), ('m_s_rot90', ['-m', '-s'], 90)]


@pytest.mark.parametrize('flags, rotate', [f[1:] for f in FLAGS], ids=[f[0] for f in FLAGS])
def test_maps_overlay_the_products(scan_file, tmp_path, capsys, monkeypatch, flags, rotate):
    from solex_ser_recon_en_amd import CLI_handler, SHG_MAIN, doppler, lineprofile, outputs
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    defaults = SHG_MAIN.default_options
    monkeypatch.setattr(SHG_MAIN, 'default_options', lambda: dict(defaults(), img_rotate=rotate))
    dirs = {}
    for name in ('products', 'doppler', 'profile'):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
        shutil.copy(scan_file, dirs[name] / 'scan.ser')
    assert SHG_MAIN.main(['-t'] + flags + [str(dirs['products'] / 'scan.ser')]) == 0
    outputs.flush()
    dop = run_json(doppler.main, capsys, [str(dirs['doppler'] / 'scan.ser')] + flags)
    prof = run_json(lineprofile.main, capsys, [str(dirs['profile'] / 'scan.ser')] + flags)
    unc = read_png_gray(str(dirs['products'] / 'scan_shift=0_uncontrasted.png')).astype(np.float64)
    dmap, _ = read_fits_f32(dop['fits'])
    cog, _ = read_fits_f32(prof['fits']['cog'])
    assert dmap.shape == cog.shape == unc.shape == read_png_gray(str(dirs['products'] / 'scan_shift=0_clahe.png')).shape
    # the marker: above 0.6 of the brightest pixel in the product (the rest of the disk's line core stays below 0.5 of it), shifted
    # by more than half the injected shift in the maps
    with np.errstate(invalid='ignore'):
        same_region(unc > 0.6 * unc.max(), dmap > SHIFT / 2, 'doppler vs uncontrasted')
        same_region(unc > 0.6 * unc.max(), cog > SHIFT / 2, 'line cog vs uncontrasted')
    # the maps' NaN: the products' circle and crop, turned as written
    opts = SHG_MAIN.default_options()
    CLI_handler.handle_CLI(opts, flags + [scan_file])
    assert dop['circle'] == prof['circle'] and dop['ratio'] == prof['ratio'] and dop['phi'] == prof['phi'] and dop['crop'] == prof['crop']
    _, _, _, out_h, out_w, _, _ = _warp_geometry(dop['phi'], dop['ratio'], IH, N)
    crop, circle_out = crop_plan(out_h, out_w, tuple(dop['circle']), opts)
    assert (None if crop is None else list(crop)) == dop['crop']
    nw, lo, dx0, n = crop if crop is not None else (out_w, 0, 0, out_w)
    off = np.zeros((out_h, nw), dtype=bool)
    off[:, :dx0] = off[:, dx0 + n:] = True
    if tuple(circle_out) != (-1, -1, -1):
        cx, cy, rad = circle_out
        r = np.arange(out_h, dtype=np.float64)[:, None]
        c = np.arange(nw, dtype=np.float64)[None, :]
        off |= (c - cx) * (c - cx) + (r - cy) * (r - cy) > rad * rad
    off = np.rot90(off, rotate // 90)
    for what, m in (('doppler', dmap), ('line cog', cog)):
        assert not np.isfinite(m[off]).any(), '%s: values outside the products\' circle or crop' % what
        inside_nan = int(np.isnan(m[~off]).sum())
        print('%s %s rot %d: %d of %d disk pixels NaN' % (what, flags, rotate, inside_nan, int((~off).sum())))
        if tuple(circle_out) != (-1, -1, -1):         # (without a circle the dark ends of the slit and the sky stay NaN)
            assert inside_nan <= 0.002 * (~off).sum(), '%s: the NaN pattern is not the products\' circle' % what
    # the geometry is the products': ellipse_to_circle on the ellipse-fit shift's disk, mirrored with -m
    if '-x' in flags:
        assert dop['circle'] == [-1, -1, -1]
        return
    from solex_ser_recon_en_amd.device import DeviceImage
    from solex_ser_recon_en_amd.ellipse_to_circle import ellipse_to_circle
    from solex_ser_recon_en_amd.fits_io import make_header
    from solex_ser_recon_en_amd.solex_util import compute_mean_return_fit, extract_disks
    from solex_ser_recon_en_amd.video_reader import video_reader
    opts['_nolog'] = True
    rdr = video_reader(scan_file)
    _, fit, _, _ = compute_mean_return_fit(rdr, opts, make_header(rdr), rdr.iw, rdr.ih, '')
    disk = extract_disks(rdr, fit, [opts['ellipse_fit_shift']], flip_x=bool(opts['flip_x']))[0]
    _, circle, ratio, phi, _ = ellipse_to_circle(DeviceImage(disk), opts, '', need_image=False)
    assert dop['ratio'] == ratio and dop['phi'] == phi and dop['circle'] == [float(v) for v in circle]
