"""The Dopplergram: where the line core sits at every point of the disk, i.e. a line-of-sight velocity map, in the geometry of
the scan's products (it overlays `_clahe.png` pixel for pixel).  Not a reference feature: the arithmetic is the one
include/shg_hip.h states for shg_line_core_shift and shg_doppler_finish (tests/doppler_ref.py restates it in NumPy).

    python -m solex_ser_recon_en_amd.doppler FILE [--half-width H] [--range R]
        [--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags: -x -s -r W -m ...]

writes <base>_doppler.fits (float32, NaN off the disk, BUNIT 'pixel' or 'km/s') and <base>_doppler.png (16-bit grey: 32768 =
no shift, +-R pixels = 1 / 65535, 0 = no data), both rotated by img_rotate as the other products, and prints one JSON line.
The CLI is single-process: under torchrun (WORLD_SIZE > 1) it refuses to run.

Per slit row y and frame k the line core is the vertex of the parabola through the minimum of the profile within H pixels of
the fitted line (fit[y, 0]) and its two neighbours; the shift is that position minus fit[y, 3], the line centre of the mean
image.  A positive shift is a longer wavelength (the spectral analyser's convention); with a dispersion D (A / px) and the
line's wavelength L (A) it is d * D / L * 299792.458 km/s.
"""
import argparse
import contextlib
import io
import json
import math
import os
import sys

import numpy as np

from . import ops

C_KM_S = 299792.458
MAX_HALF_WIDTH = 32


def _geometry(rdr, fit, opts):
    """(circle, ratio, phi) exactly as Solex_recon.solex_process obtains them: the limb fit of the ellipse-fit shift's disk (flipped
    with flip_x, as solex_read extracts it), or ratio_fixe / slant_fix with no circle."""
    if opts['ratio_fixe'] is None and opts['slant_fix'] is None:
        from .device import DeviceImage
        from .ellipse_to_circle import ellipse_to_circle
        from .solex_util import extract_disks
        disks, mm = extract_disks(rdr, fit, [opts['ellipse_fit_shift']], flip_x=bool(opts['flip_x']), want_minmax=True)
        disk = DeviceImage(disks[0], minmax=None if mm is None else mm[0])
        with contextlib.redirect_stdout(io.StringIO()):           # ellipse_to_circle reports the borders on stdout
            _, circle, ratio, phi, _ = ellipse_to_circle(disk, opts, '', need_image=False)
        return tuple(float(v) for v in circle), float(ratio), float(phi)
    ratio = opts['ratio_fixe'] if opts['ratio_fixe'] is not None else 1.0
    phi = math.radians(opts['slant_fix']) if opts['slant_fix'] is not None else 0.0
    return (-1, -1, -1), float(ratio), float(phi)


def finish_circle(circle, crop, circle_out):
    """The circle the finish masks with, in the corrected image's columns: the products' circle (crop_plan's circle_out) taken back
    through the crop.  crop_plan centres the crop on int(cx) and moves the circle to the crop's middle column nw // 2, dropping the
    fraction of cx; masking with `circle` itself would put the map's disk that fraction of a pixel off the products' disk."""
    if crop is None or tuple(circle) == (-1, -1, -1):
        return circle
    nw, lo, dx0, n = crop
    return (float(circle_out[0] - dx0 + lo), circle[1], circle[2])


def velocity_factor(dispersion, wavelength):
    """km/s per pixel of shift: (dispersion / wavelength) * c."""
    return (float(dispersion) / float(wavelength)) * C_KM_S


def _line_maps(file_or_reader, options, half_width, display_range, dispersion, wavelength, sharded, measure, finish, check_frame=None):
    """The driver dopplergram() and lineprofile.line_profile_maps() share: argument checks, reader (`sharded`: the refusal of a
    frame-sharded scan), line fit, raw = measure(stack, fit, flip_x) and (maps, png) = finish(raw, h00, h01, h02, out_h, out_w, circle,
    crop) in the products' geometry.  check_frame(iw) may refuse the frame before the fit.  -> (raw, maps, png as NumPy arrays, the
    fields of the result dict both share, km/s per pixel or None)."""
    from . import SHG_MAIN, dist
    from .ellipse_to_circle import _warp_geometry
    from .fits_io import make_header
    from .Solex_recon import crop_plan
    from .solex_util import compute_mean_return_fit
    from .video_reader import video_reader
    if not 1 <= half_width <= MAX_HALF_WIDTH:
        raise ValueError('half_width must lie in [1, %d], got %d' % (MAX_HALF_WIDTH, half_width))
    if not (math.isfinite(display_range) and display_range > 0):
        raise ValueError('display_range must be positive')
    if (dispersion is None) != (wavelength is None):
        raise ValueError('km/s needs both the dispersion and the wavelength')
    if dispersion is not None and not (dispersion > 0 and wavelength > 0):
        raise ValueError('dispersion and wavelength must be positive')
    opts = SHG_MAIN.default_options() if options is None else dict(options)
    opts.update(save_fit=False, flag_display=False, _nolog=True, basefich0='')
    rdr = file_or_reader if hasattr(file_or_reader, 'device_stack') else video_reader(file_or_reader)
    if dist.is_sharded(rdr):
        raise ValueError(sharded)
    ih, iw, n = int(rdr.ih), int(rdr.iw), int(rdr.FrameCount)
    if check_frame is not None:
        check_frame(iw)
    _, fit, _, _ = compute_mean_return_fit(rdr, opts, make_header(rdr), iw, ih, '')
    raw = measure(rdr.device_stack(), fit, bool(opts['flip_x']))
    circle, ratio, phi = _geometry(rdr, fit, opts)
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(phi, ratio, ih, n)
    crop, circle_out = crop_plan(out_h, out_w, circle, opts)
    maps, png = finish(raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, finish_circle(circle, crop, circle_out), crop)
    common = {'circle': circle, 'circle_out': circle_out, 'ratio': ratio, 'phi': phi, 'crop': crop, 'fit': fit, 'half_width': half_width,
              'display_range': float(display_range), 'dispersion': dispersion, 'wavelength': wavelength}
    factor = None if dispersion is None else velocity_factor(dispersion, wavelength)
    return raw.contiguous().cpu().numpy(), maps.cpu().numpy(), png.cpu().numpy(), common, factor


def _km_s(m, factor):
    """A pixel-shift map in km/s."""
    return (m.astype(np.float64) * factor).astype(np.float32)


def dopplergram(file_or_reader, options=None, half_width=5, display_range=2.0, dispersion=None, wavelength=None):
    """The Dopplergram of one scan -> dict(raw = float32 [ih, N] shift in pixels per slit row and frame; map = float32, the raw map
    resampled to the corrected image, NaN off the disk and in the crop's padding, in `units`; png = uint16 display plane of the
    pixel map (0 = NaN, 32768 +- 32767 at +-display_range pixels); circle (-1, -1, -1 without a limb fit), ratio, phi, crop (the
    crop_plan, or None), fit [ih, 4], units ('pixel', or 'km/s' when dispersion and wavelength are both given)).
    options: SHG_MAIN's (flip_x, ratio_fixe, slant_fix, crop_width_square, fixed_width, ellipse_fit_shift are used)."""
    half_width = int(half_width)
    raw, dmap, png, res, factor = _line_maps(
        file_or_reader, options, half_width, display_range, dispersion, wavelength,
        'the Dopplergram of a frame-sharded scan is not supported',
        lambda stack, fit, flip: ops.line_core_shift(stack, fit, half_width, flip_x=flip),
        lambda raw, *geometry: ops.doppler_finish(raw, *geometry, display_range))
    res.update(raw=raw, map=dmap if factor is None else _km_s(dmap, factor), png=png, units='pixel' if factor is None else 'km/s')
    return res


def disk_stats(res):
    """valid fraction, median and 1st / 99th percentile of the map on the disk (the whole map without a circle)."""
    m = res['map']
    cx, cy, rad = res['circle_out']
    if (cx, cy, rad) == (-1, -1, -1):
        on = np.ones(m.shape, dtype=bool)
    else:
        r = np.arange(m.shape[0], dtype=np.float64)[:, None]
        c = np.arange(m.shape[1], dtype=np.float64)[None, :]
        on = (c - cx) * (c - cx) + (r - cy) * (r - cy) <= rad * rad
    v = m[on]
    v = v[np.isfinite(v)]
    out = {'valid_fraction': float(v.size / max(int(on.sum()), 1))}
    if v.size:
        p1, med, p99 = np.percentile(v.astype(np.float64), [1, 50, 99])
        out.update(median=float(med), p1=float(p1), p99=float(p99))
    else:
        out.update(median=None, p1=None, p99=None)
    return out


# ---- command line ---------------------------------------------------------------------------------
def _parser(prog, usage, description, half_width, helps, extra=None):
    """The parser of the flags both CLIs take; helps = the help of --half-width, --range, --dispersion, --wavelength; extra(p) adds
    a CLI's own flags after --half-width."""
    p = argparse.ArgumentParser(prog=prog, usage=usage, description=description)
    p.add_argument('--half-width', type=int, default=half_width, help=helps[0])
    if extra is not None:
        extra(p)
    p.add_argument('--range', type=float, default=2.0, help=helps[1])
    p.add_argument('--dispersion', type=float, help=helps[2])
    p.add_argument('--wavelength', type=float, help=helps[3])
    p.add_argument('--atlas', help='atlas in alps.npz layout: the dispersion from the spectral analyser\'s fit')
    p.add_argument('--anchor', type=float, help='A, the line the scan is centred on (with --atlas)')
    return p


def _cli(p, argv, single, w_flag, extra_checks=None, positive=()):
    """The command line both CLIs share: parse, validate (`single`, `w_flag`: the refusals under torchrun and of -w; extra_checks(args)
    after --range, `positive`: more flags that must be positive), the SHG_MAIN flags, the one file and the atlas -> (args, opts, path,
    atlas or None).  Errors exit through p.error."""
    from . import CLI_handler, SHG_MAIN, spectral
    args, rest = p.parse_known_args(sys.argv[1:] if argv is None else list(argv))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        p.error(single)
    if not 1 <= args.half_width <= MAX_HALF_WIDTH:
        p.error('--half-width must lie in [1, %d]' % MAX_HALF_WIDTH)
    if not (math.isfinite(args.range) and args.range > 0):
        p.error('--range must be positive')
    if extra_checks is not None:
        extra_checks(args)
    if (args.dispersion is None) != (args.wavelength is None):
        p.error('--dispersion and --wavelength go together')
    if (args.atlas is None) != (args.anchor is None):
        p.error('--atlas and --anchor go together')
    if args.atlas is not None and args.dispersion is not None:
        p.error('--atlas / --anchor and --dispersion / --wavelength exclude each other')
    for name in ('dispersion', 'wavelength', 'anchor') + tuple(positive):
        v = getattr(args, name)
        if v is not None and not (math.isfinite(v) and v > 0):
            p.error('--%s must be positive' % name)
    if any(a.startswith('-') and 'w' in a for a in rest):
        p.error(w_flag)
    opts = SHG_MAIN.default_options()
    try:
        with contextlib.redirect_stdout(sys.stderr):            # the SHG_MAIN parser reports on stdout: keep it for the JSON line
            files = CLI_handler.handle_CLI(opts, rest)
    except ValueError as e:
        p.error(str(e))
    unknown = [a for a in rest if not a.startswith('-') and a not in files and not a.isdigit()]
    if len(files) != 1 or unknown:
        p.error('exactly one SER or AVI file is needed (got %s)' % (files + unknown))
    path = files[0]
    if not os.path.isfile(path):
        p.error('no such file: %s' % path)
    try:
        atlas = spectral.load_atlas(args.atlas) if args.atlas is not None else None
    except (OSError, KeyError, ValueError) as e:
        p.error('--atlas: %s' % e)
    return args, opts, path, atlas


def _cli_dispersion(rdr, opts, args, atlas):
    """(dispersion, wavelength, the spectral analysis or None): the flags', or with --atlas / --anchor the analyser's fit at the anchor."""
    from . import spectral
    if atlas is None:
        return args.dispersion, args.wavelength, None
    a = spectral.analyse(rdr, opts)
    return spectral.auto_dispersion(a['spectrum2'], a['anchor_x'], args.anchor, atlas)[0], args.anchor, a


def _write_pair(stem, opts, rdr, m, png, units, half_width, dispersion, wavelength, **keys):
    """<stem>.fits (float32 map, header BUNIT, HALFWID, keys, DISPERS / WAVELEN with a dispersion) and <stem>.png (16-bit display
    plane), both rotated by img_rotate -> (fits path, png path, shape written)."""
    from .fits_io import make_header, write_fits
    from .png_io import write_png
    from .solex_util import output_path
    hdr = make_header(rdr)
    hdr['BUNIT'] = units
    hdr['HALFWID'] = half_width
    for k, v in keys.items():
        hdr[k] = v
    if dispersion is not None:
        hdr['DISPERS'] = float(dispersion)
        hdr['WAVELEN'] = float(wavelength)
    k = opts['img_rotate'] // 90
    fits_path, png_path = output_path(stem + '.fits', opts), output_path(stem + '.png', opts)
    m = np.ascontiguousarray(np.rot90(m, k))
    write_fits(fits_path, m, hdr)
    write_png(png_path, np.ascontiguousarray(np.rot90(png, k)), 0)
    return fits_path, png_path, list(m.shape)


def main(argv=None):
    from .video_reader import video_reader
    p = _parser('python -m solex_ser_recon_en_amd.doppler',
                '%(prog)s FILE [--half-width H] [--range R] [--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags]',
                'Line-of-sight velocity map (Dopplergram) of a scan, in the geometry of its products.', 5,
                ('pixels either side of the fitted line searched for the core (1..32)',
                 'PNG display range: +-R pixels of shift map to 1 .. 65535', 'A / pixel (with --wavelength: the map in km/s)',
                 'A, the line the scan is centred on'))
    args, opts, path, atlas = _cli(p, argv, 'the Dopplergram is single-process: run it without torchrun',
                                   '-w is not a Dopplergram flag: the line core is searched around the fitted line')
    try:
        rdr = video_reader(path)
        dispersion, wavelength, _ = _cli_dispersion(rdr, opts, args, atlas)
        res = dopplergram(rdr, opts, args.half_width, args.range, dispersion, wavelength)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    fits_path, png_path, shape = _write_pair(os.path.splitext(path)[0] + '_doppler', opts, rdr, res['map'], res['png'], res['units'],
                                             res['half_width'], dispersion, wavelength)
    out = {'fits': fits_path, 'png': png_path, 'shape': shape, 'units': res['units'], 'half_width': res['half_width'],
           'display_range': res['display_range'], 'dispersion': dispersion, 'wavelength': wavelength}
    out.update(disk_stats(res))
    out.update(circle=list(res['circle']), ratio=res['ratio'], phi=res['phi'], crop=None if res['crop'] is None else list(res['crop']))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
