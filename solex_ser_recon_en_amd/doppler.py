"""The Dopplergram: where the line core sits at every point of the disk, i.e. a line-of-sight velocity map, in the geometry of
the scan's products (it overlays `_clahe.png` pixel for pixel).  Not a reference feature: the arithmetic is the one
include/shg_hip.h states for shg_line_core_shift and shg_doppler_finish (tests/linemaps_ref.py restates it in NumPy).

    python -m solex_ser_recon_en_amd.doppler FILE [--half-width H] [--range R]
        [--dispersion D --wavelength L | --atlas A --anchor L] [--detrend plane [--clip K] [--clip-iterations I]]
        [SHG_MAIN flags: -x -s -r W -m ...]

writes <base>_doppler.fits (float32, NaN off the disk, BUNIT 'pixel' or 'km/s') and <base>_doppler.png (16-bit grey: 32768 =
no shift, +-R pixels = 1 / 65535, 0 = no data), both rotated by img_rotate as the other products, and prints one JSON line.
The CLI is single-process: under torchrun (WORLD_SIZE > 1) it refuses to run.

Per slit row y and frame k the line core is the vertex of the parabola through the minimum of the profile within H pixels of
the fitted line (fit[y, 0]) and its two neighbours; the shift is that position minus fit[y, 3], the line centre of the mean
image.  A positive shift is a longer wavelength (the spectral analyser's convention); with a dispersion D (A / px) and the
line's wavelength L (A) it is d * D / L * 299792.458 km/s.

The shift is measured against the scan's own fitted line, so a field that does not average out over the scan -- solar rotation,
a plane across the disk of about +-2 km/s at the limb -- stays in the map and moves its zero.  --detrend plane fits that plane
(a + b * column + g * row, sigma-clipped least squares over the disk: linemaps.detrend_plane) on the GPU and also writes the map
without it, <base>_doppler_detrended.fits / .png; the coefficients are in pixels of shift per pixel of the map BEFORE img_rotate
turns it, as `circle` is.
"""
import math
import os
import sys

from . import ops
from .linemaps import _cli, _cli_dispersion, _km_s, _line_maps, _parser, _print_json, _write_pair, detrend_plane, disk_stats
from .linemaps import MAX_CLIP_ITERATIONS
from .linemaps import finish_circle, velocity_factor  # noqa: F401  (this module's API too)


def dopplergram(file_or_reader, options=None, half_width=5, display_range=2.0, dispersion=None, wavelength=None, detrend=None,
                clip=3.0, clip_iterations=3):
    """The Dopplergram of one scan -> dict(raw = float32 [ih, N] shift in pixels per slit row and frame; map = float32, the raw map
    resampled to the corrected image, NaN off the disk and in the crop's padding, in `units`; png = uint16 display plane of the
    pixel map (0 = NaN, 32768 +- 32767 at +-display_range pixels); circle (-1, -1, -1 without a limb fit), ratio, phi, crop (the
    crop_plan, or None), fit [ih, 4], units ('pixel', or 'km/s' when dispersion and wavelength are both given)).
    options: SHG_MAIN's (flip_x, ratio_fixe, slant_fix, crop_width_square, fixed_width, ellipse_fit_shift are used).
    detrend='plane' (None: the dict above, nothing more): also detrended = the map minus its sigma-clipped plane (detrend_plane on
    the finished pixel map, inside the circle the finish masked with, before the maps leave the GPU; clip, clip_iterations: its
    clip and iterations) in `units`, detrended_png = its display plane, and plane = detrend_plane's info in pixels (columns and
    rows of `map`), with a dispersion also b_kms, g_kms, sigma_kms and limb_amplitude_kms."""
    half_width = int(half_width)
    if detrend not in (None, 'plane'):
        raise ValueError('detrend must be None or \'plane\', got %r' % (detrend,))
    flat = {}

    def finish(raw, h00, h01, h02, out_h, out_w, circle, crop):
        m, png = ops.doppler_finish(raw, h00, h01, h02, out_h, out_w, circle, crop, display_range)
        if detrend is not None:
            # the finish's circle lies in the corrected image's columns: the map's own start at the crop
            if crop is not None and circle is not None and tuple(circle) != (-1, -1, -1):
                circle = (circle[0] - crop[1] + crop[2], circle[1], circle[2])
            flat['out'], flat['png'], flat['info'] = detrend_plane(m, circle, clip, clip_iterations, display_range)
        return m, png

    raw, dmap, png, res, factor = _line_maps(
        file_or_reader, options, half_width, display_range, dispersion, wavelength,
        'the Dopplergram of a frame-sharded scan is not supported',
        lambda stack, fit, flip: ops.line_core_shift(stack, fit, half_width, flip_x=flip), finish)
    res.update(raw=raw, map=dmap if factor is None else _km_s(dmap, factor), png=png, units='pixel' if factor is None else 'km/s')
    if detrend is not None:
        flat_map, info = flat['out'].cpu().numpy(), dict(flat['info'])
        if factor is not None:
            info.update(b_kms=info['b'] * factor, g_kms=info['g'] * factor, sigma_kms=info['sigma'] * factor)
            if 'limb_amplitude' in info:
                info['limb_amplitude_kms'] = info['limb_amplitude'] * factor
        res.update(detrended=flat_map if factor is None else _km_s(flat_map, factor), detrended_png=flat['png'].cpu().numpy(),
                   plane=info)
    return res


# ---- command line ---------------------------------------------------------------------------------
def _detrend_flags(p):
    p.add_argument('--detrend', choices=['plane'],
                   help='also write <base>_doppler_detrended.fits / .png: the map minus its sigma-clipped least-squares plane (solar '
                        'rotation); the coefficients a, b, g of a + b * column + g * row (FITS DTA, DTB, DTG, the JSON line\'s plane) refer '
                        'to the map before img_rotate turns it, as circle does')
    p.add_argument('--clip', type=float, help='with --detrend: pixels beyond K sigma of the previous fit are left out (default 3)')
    p.add_argument('--clip-iterations', type=int, help='with --detrend: clipped passes after the first fit, 0..16 (default 3)')


def main(argv=None):
    from .video_reader import video_reader
    p = _parser('python -m solex_ser_recon_en_amd.doppler',
                '%(prog)s FILE [--half-width H] [--range R] [--dispersion D --wavelength L | --atlas A --anchor L] '
                '[--detrend plane [--clip K] [--clip-iterations I]] [SHG_MAIN flags]',
                'Line-of-sight velocity map (Dopplergram) of a scan, in the geometry of its products.', 5,
                ('pixels either side of the fitted line searched for the core (1..32)',
                 'PNG display range: +-R pixels of shift map to 1 .. 65535', 'A / pixel (with --wavelength: the map in km/s)',
                 'A, the line the scan is centred on'), extra=_detrend_flags)

    def checks(args):
        if args.detrend is None and (args.clip is not None or args.clip_iterations is not None):
            p.error('--clip and --clip-iterations need --detrend')
        if args.clip is not None and not (math.isfinite(args.clip) and args.clip > 0):
            p.error('--clip must be positive')
        if args.clip_iterations is not None and not 0 <= args.clip_iterations <= MAX_CLIP_ITERATIONS:
            p.error('--clip-iterations must lie in [0, %d]' % MAX_CLIP_ITERATIONS)

    args, opts, path, atlas = _cli(p, argv, 'the Dopplergram is single-process: run it without torchrun',
                                   '-w is not a Dopplergram flag: the line core is searched around the fitted line', checks)
    try:
        rdr = video_reader(path)
        dispersion, wavelength, _ = _cli_dispersion(rdr, opts, args, atlas)
        res = dopplergram(rdr, opts, args.half_width, args.range, dispersion, wavelength, args.detrend,
                          3.0 if args.clip is None else args.clip, 3 if args.clip_iterations is None else args.clip_iterations)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    stem = os.path.splitext(path)[0] + '_doppler'
    fits_path, png_path, shape = _write_pair(stem, opts, rdr, res['map'], res['png'], res['units'], res['half_width'], dispersion,
                                             wavelength)
    out = {'fits': fits_path, 'png': png_path, 'shape': shape, 'units': res['units'], 'half_width': res['half_width'],
           'display_range': res['display_range'], 'dispersion': dispersion, 'wavelength': wavelength}
    out.update(disk_stats(res))
    if args.detrend is not None:
        plane = res['plane']
        out['detrended_fits'], out['detrended_png'], _ = _write_pair(
            stem + '_detrended', opts, rdr, res['detrended'], res['detrended_png'], res['units'], res['half_width'], dispersion,
            wavelength, DETREND='plane', DTA=plane['a'], DTB=plane['b'], DTG=plane['g'], DTSIGMA=plane['sigma'], DTNUSED=plane['n_used'])
        out['plane'] = plane
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
