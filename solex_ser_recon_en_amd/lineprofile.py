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
import json
import os
import sys

from . import ops
from .doppler import _cli, _cli_dispersion, _km_s, _line_maps, _parser, _write_pair, disk_stats

PLANES = ops.LINE_PROFILE_PLANES
WRITTEN = ('core', 'width', 'cog', 'ew')        # the CLI's products (the shift plane is the Dopplergram's)


def line_profile_maps(file_or_reader, options=None, half_width=10, shift=0, display_range=2.0, dispersion=None, wavelength=None):
    """The line-profile maps of one scan -> dict(raw = {plane: float32 [ih, N] per slit row and frame}; maps = {plane: float32, the
    raw plane resampled to the corrected image, NaN off the disk and in the crop's padding, in units[plane]}; png = {plane: uint16
    display plane of the raw-unit map}; circle (-1, -1, -1 without a limb fit), circle_out, ratio, phi, crop (the crop_plan, or None),
    fit [ih, 4], units = {plane: 'pixel' | 'km/s' | 'adu'}, half_width, shift, display_range, dispersion, wavelength).
    Planes: shift and cog (pixels, or km/s given dispersion and wavelength), core (sample scale), width and ew (pixels).
    The geometry is the ellipse-fit shift's, whatever `shift` is.  options: SHG_MAIN's (as dopplergram())."""
    half_width, shift = int(half_width), int(shift)

    def check_frame(iw):
        if not 3 - iw - half_width < shift < iw - 3 + half_width:
            raise ValueError('shift %d puts every window outside the frame (%d columns)' % (shift, iw))

    raw, maps, png, res, factor = _line_maps(
        file_or_reader, options, half_width, display_range, dispersion, wavelength,
        'the line-profile maps of a frame-sharded scan are not supported',
        lambda stack, fit, flip: ops.line_profile(stack, fit, half_width, shift, flip_x=flip),
        lambda raw, *geometry: ops.line_profile_finish(raw, *geometry, half_width, display_range), check_frame)
    units = {'shift': 'pixel', 'core': 'adu', 'width': 'pixel', 'cog': 'pixel', 'ew': 'pixel'}
    out = {name: maps[q] for q, name in enumerate(PLANES)}
    if factor is not None:
        for name in ('shift', 'cog'):
            out[name] = _km_s(out[name], factor)
            units[name] = 'km/s'
    res.update(raw={name: raw[q] for q, name in enumerate(PLANES)}, maps=out, png={name: png[q] for q, name in enumerate(PLANES)},
               units=units, shift=shift)
    return res


# ---- command line ---------------------------------------------------------------------------------
def _own_flags(p):
    p.add_argument('--shift', type=int, help='pixel shift of the line to measure (the -w shift; default 0: the fitted line)')
    p.add_argument('--line', type=float, help='A, the line to measure (with --atlas / --anchor: its shift from the analyser)')


def main(argv=None):
    from . import spectral
    from .video_reader import video_reader
    p = _parser('python -m solex_ser_recon_en_amd.lineprofile',
                '%(prog)s FILE [--half-width H] [--shift S | --line L] [--range R] '
                '[--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags]',
                'Line core intensity, width, centre of gravity and equivalent width maps of a scan.', 10,
                ('pixels either side of the line measured (1..32)', 'PNG display range of the cog map: +-R pixels to 1 .. 65535',
                 'A / pixel (with --wavelength: the cog map in km/s)', 'A, the line measured'), _own_flags)

    def own_checks(args):
        if args.shift is not None and args.line is not None:
            p.error('--shift and --line exclude each other')
        if args.line is not None and args.atlas is None:
            p.error('--line needs --atlas and --anchor')

    args, opts, path, atlas = _cli(p, argv, 'the line-profile maps are single-process: run them without torchrun',
                                   '-w is not a line-profile flag: give the line with --shift or --line', own_checks, ('line',))
    try:
        rdr = video_reader(path)
        dispersion, wavelength, a = _cli_dispersion(rdr, opts, args, atlas)
        shift = args.shift or 0
        if args.line is not None:
            shift, _ = spectral.shift_for_wavelength(args.line, args.anchor, dispersion, a['fit'], int(rdr.iw))
            wavelength = args.line
        res = line_profile_maps(rdr, opts, args.half_width, shift, args.range, dispersion, wavelength)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    base = os.path.splitext(path)[0]
    out = {'shape': None, 'shift': res['shift'], 'half_width': res['half_width'], 'display_range': res['display_range'],
           'dispersion': dispersion, 'wavelength': wavelength, 'fits': {}, 'png': {}, 'units': {}, 'median': {}, 'valid_fraction': {}}
    for name in WRITTEN:
        fits_path, png_path, out['shape'] = _write_pair('%s_shift=%d_line_%s' % (base, res['shift'], name), opts, rdr, res['maps'][name],
                                                        res['png'][name], res['units'][name], res['half_width'], dispersion,
                                                        wavelength, SHIFT=res['shift'])
        stats = disk_stats({'map': res['maps'][name], 'circle_out': res['circle_out']})
        out['fits'][name], out['png'][name], out['units'][name] = fits_path, png_path, res['units'][name]
        out['median'][name], out['valid_fraction'][name] = stats['median'], stats['valid_fraction']
    out.update(circle=list(res['circle']), ratio=res['ratio'], phi=res['phi'], crop=None if res['crop'] is None else list(res['crop']))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
