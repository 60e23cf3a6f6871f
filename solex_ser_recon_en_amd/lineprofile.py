"""Line-profile maps: the line's core intensity, width (FWHM), centre of gravity and equivalent width at every point of the disk,
for the fitted line or any line at an integer pixel shift, in the geometry of the scan's products (the maps overlay
`<base>_shift=<S>_clahe.png` pixel for pixel).  Not a reference feature: the arithmetic is the one include/shg_hip.h states for
shg_line_profile and shg_line_profile_finish (tests/lineprofile_ref.py restates it in NumPy).

    python -m solex_ser_recon_en_amd.lineprofile FILE [--half-width H] [--shift S | --line L] [--range R]
        [--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags: -x -s -r W -m ...]

writes <base>_shift=<S>_line_{core,width,cog,ew}.fits (float32, NaN off the disk) and the matching 16-bit .png files, rotated by
img_rotate as the other products, and prints one JSON line.  --line L (with --atlas / --anchor) measures the line at wavelength
L: S from spectral.shift_for_wavelength, and L is the wavelength of the km/s.  The core's position is the Dopplergram's product
(python -m solex_ser_recon_en_amd.doppler) and is not written here.  The CLI is single-process: under torchrun it refuses to run.

Per slit row and frame, in the window of H pixels either side of the line: core = the intensity at the vertex of the parabola
through the profile's minimum and its neighbours (sample scale); width = the distance between the crossings of the level halfway
from the core to the continuum (the mean of the window's end samples), linearly interpolated; cog = the centre of gravity of
continuum - p, minus the mean image's line centre (+ = longer wavelength, km/s as the Dopplergram's); ew = the equivalent width
within the window, sum(1 - p / continuum) pixels.
"""
import argparse
import contextlib
import json
import math
import os
import sys

import numpy as np

from . import ops
from .doppler import MAX_HALF_WIDTH, _geometry, disk_stats, velocity_factor

PLANES = ops.LINE_PROFILE_PLANES
WRITTEN = ('core', 'width', 'cog', 'ew')        # the CLI's products (the shift plane is the Dopplergram's)


def line_profile_maps(file_or_reader, options=None, half_width=10, shift=0, display_range=2.0, dispersion=None, wavelength=None):
    """The line-profile maps of one scan -> dict(raw = {plane: float32 [ih, N] per slit row and frame}; maps = {plane: float32, the
    raw plane resampled to the corrected image, NaN off the disk and in the crop's padding, in units[plane]}; png = {plane: uint16
    display plane of the raw-unit map}; circle (-1, -1, -1 without a limb fit), circle_out, ratio, phi, crop (the crop_plan, or None),
    fit [ih, 4], units = {plane: 'pixel' | 'km/s' | 'adu'}, half_width, shift, display_range, dispersion, wavelength).
    Planes: shift and cog (pixels, or km/s given dispersion and wavelength), core (sample scale), width and ew (pixels).
    The geometry is the ellipse-fit shift's, whatever `shift` is.  options: SHG_MAIN's (as dopplergram())."""
    from . import SHG_MAIN, dist
    from .ellipse_to_circle import _warp_geometry
    from .fits_io import make_header
    from .Solex_recon import crop_plan
    from .solex_util import compute_mean_return_fit
    from .video_reader import video_reader
    half_width, shift = int(half_width), int(shift)
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
        raise ValueError('the line-profile maps of a frame-sharded scan are not supported')
    ih, iw, n = int(rdr.ih), int(rdr.iw), int(rdr.FrameCount)
    if not 3 - iw - half_width < shift < iw - 3 + half_width:
        raise ValueError('shift %d puts every window outside the frame (%d columns)' % (shift, iw))
    _, fit, _, _ = compute_mean_return_fit(rdr, opts, make_header(rdr), iw, ih, '')
    raw = ops.line_profile(rdr.device_stack(), fit, half_width, shift, flip_x=bool(opts['flip_x']))
    circle, ratio, phi = _geometry(rdr, fit, opts)
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(phi, ratio, ih, n)
    crop, circle_out = crop_plan(out_h, out_w, circle, opts)
    maps, png = ops.line_profile_finish(raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, circle, crop, half_width, display_range)
    maps, png, raw = maps.cpu().numpy(), png.cpu().numpy(), raw.contiguous().cpu().numpy()
    units = {'shift': 'pixel', 'core': 'adu', 'width': 'pixel', 'cog': 'pixel', 'ew': 'pixel'}
    out = {name: maps[q] for q, name in enumerate(PLANES)}
    if dispersion is not None:
        f = velocity_factor(dispersion, wavelength)
        for name in ('shift', 'cog'):
            out[name] = (out[name].astype(np.float64) * f).astype(np.float32)
            units[name] = 'km/s'
    return {'raw': {name: raw[q] for q, name in enumerate(PLANES)}, 'maps': out, 'png': {name: png[q] for q, name in enumerate(PLANES)},
            'circle': circle, 'circle_out': circle_out, 'ratio': ratio, 'phi': phi, 'crop': crop, 'fit': fit, 'units': units,
            'half_width': half_width, 'shift': shift, 'display_range': float(display_range), 'dispersion': dispersion,
            'wavelength': wavelength}


# ---- command line ---------------------------------------------------------------------------------
def _parser():
    p = argparse.ArgumentParser(prog='python -m solex_ser_recon_en_amd.lineprofile',
                                usage='%(prog)s FILE [--half-width H] [--shift S | --line L] [--range R] '
                                      '[--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags]',
                                description='Line core intensity, width, centre of gravity and equivalent width maps of a scan.')
    p.add_argument('--half-width', type=int, default=10, help='pixels either side of the line measured (1..32)')
    p.add_argument('--shift', type=int, help='pixel shift of the line to measure (the -w shift; default 0: the fitted line)')
    p.add_argument('--line', type=float, help='A, the line to measure (with --atlas / --anchor: its shift from the analyser)')
    p.add_argument('--range', type=float, default=2.0, help='PNG display range of the cog map: +-R pixels to 1 .. 65535')
    p.add_argument('--dispersion', type=float, help='A / pixel (with --wavelength: the cog map in km/s)')
    p.add_argument('--wavelength', type=float, help='A, the line measured')
    p.add_argument('--atlas', help='atlas in alps.npz layout: the dispersion from the spectral analyser\'s fit')
    p.add_argument('--anchor', type=float, help='A, the line the scan is centred on (with --atlas)')
    return p


def main(argv=None):
    from . import CLI_handler, SHG_MAIN, spectral
    from .fits_io import make_header, write_fits
    from .png_io import write_png
    from .solex_util import output_path
    from .video_reader import video_reader
    p = _parser()
    args, rest = p.parse_known_args(sys.argv[1:] if argv is None else list(argv))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        p.error('the line-profile maps are single-process: run them without torchrun')
    if not 1 <= args.half_width <= MAX_HALF_WIDTH:
        p.error('--half-width must lie in [1, %d]' % MAX_HALF_WIDTH)
    if not (math.isfinite(args.range) and args.range > 0):
        p.error('--range must be positive')
    if args.shift is not None and args.line is not None:
        p.error('--shift and --line exclude each other')
    if args.line is not None and args.atlas is None:
        p.error('--line needs --atlas and --anchor')
    if (args.dispersion is None) != (args.wavelength is None):
        p.error('--dispersion and --wavelength go together')
    if (args.atlas is None) != (args.anchor is None):
        p.error('--atlas and --anchor go together')
    if args.atlas is not None and args.dispersion is not None:
        p.error('--atlas / --anchor and --dispersion / --wavelength exclude each other')
    for name in ('dispersion', 'wavelength', 'anchor', 'line'):
        v = getattr(args, name)
        if v is not None and not (math.isfinite(v) and v > 0):
            p.error('--%s must be positive' % name)
    if any(a.startswith('-') and 'w' in a for a in rest):
        p.error('-w is not a line-profile flag: give the line with --shift or --line')
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
    try:
        rdr = video_reader(path)
        dispersion, wavelength = args.dispersion, args.wavelength
        shift = args.shift or 0
        if atlas is not None:
            a = spectral.analyse(rdr, opts)
            dispersion = spectral.auto_dispersion(a['spectrum2'], a['anchor_x'], args.anchor, atlas)[0]
            wavelength = args.anchor
            if args.line is not None:
                shift, _ = spectral.shift_for_wavelength(args.line, args.anchor, dispersion, a['fit'], int(rdr.iw))
                wavelength = args.line
        res = line_profile_maps(rdr, opts, args.half_width, shift, args.range, dispersion, wavelength)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    base = os.path.splitext(path)[0]
    k = opts['img_rotate'] // 90
    out = {'shape': None, 'shift': res['shift'], 'half_width': res['half_width'], 'display_range': res['display_range'],
           'dispersion': dispersion, 'wavelength': wavelength, 'fits': {}, 'png': {}, 'units': {}, 'median': {}, 'valid_fraction': {}}
    for name in WRITTEN:
        hdr = make_header(rdr)
        hdr['BUNIT'] = res['units'][name]
        hdr['HALFWID'] = res['half_width']
        hdr['SHIFT'] = res['shift']
        if dispersion is not None:
            hdr['DISPERS'] = float(dispersion)
            hdr['WAVELEN'] = float(wavelength)
        stem = '%s_shift=%d_line_%s' % (base, res['shift'], name)
        fits_path, png_path = output_path(stem + '.fits', opts), output_path(stem + '.png', opts)
        m = np.ascontiguousarray(np.rot90(res['maps'][name], k))
        write_fits(fits_path, m, hdr)
        write_png(png_path, np.ascontiguousarray(np.rot90(res['png'][name], k)), 0)
        stats = disk_stats({'map': res['maps'][name], 'circle_out': res['circle_out']})
        out['fits'][name], out['png'][name], out['units'][name] = fits_path, png_path, res['units'][name]
        out['median'][name], out['valid_fraction'][name] = stats['median'], stats['valid_fraction']
        out['shape'] = list(m.shape)
    out.update(circle=list(res['circle']), ratio=res['ratio'], phi=res['phi'], crop=None if res['crop'] is None else list(res['crop']))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
