"""The Dopplergram: where the line core sits at every point of the disk, i.e. a line-of-sight velocity map, in the geometry of
the scan's products (it overlays `_clahe.png` pixel for pixel).  Not a reference feature: the arithmetic is the one
include/shg_hip.h states for shg_line_core_shift and shg_doppler_finish (tests/linemaps_ref.py restates it in NumPy).

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
import os
import sys

from . import ops
from .linemaps import _cli, _cli_dispersion, _km_s, _line_maps, _parser, _print_json, _write_pair, disk_stats
from .linemaps import finish_circle, velocity_factor  # noqa: F401  (this module's API too)


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


# ---- command line ---------------------------------------------------------------------------------
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
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
