"""Line-profile maps: the line's core intensity, width (FWHM), centre of gravity and equivalent width at every point of the disk,
for the fitted line or any line at an integer pixel shift, in the geometry of the scan's products (the maps overlay
`<base>_shift=<S>_clahe.png` pixel for pixel).  Not a reference feature: the arithmetic is the one include/shg_hip.h states for
shg_line_profile and shg_line_profile_finish (tests/linemaps_ref.py restates it in NumPy).

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
import sys

from . import ops
from .linemaps import _by_plane, _cli, _cli_dispersion, _line_maps, _parser, _print_json, _write_planes

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
    raw, maps, png, res, factor = _line_maps(
        file_or_reader, options, half_width, display_range, dispersion, wavelength,
        'the line-profile maps of a frame-sharded scan are not supported',
        lambda stack, fit, flip: ops.line_profile(stack, fit, half_width, shift, flip_x=flip),
        lambda raw, *geometry: ops.line_profile_finish(raw, *geometry, half_width, display_range), shift)
    return _by_plane(res, PLANES, {'shift': 'pixel', 'core': 'adu', 'width': 'pixel', 'cog': 'pixel', 'ew': 'pixel'}, ('shift', 'cog'),
                     raw, maps, png, factor, shift=shift)


# ---- command line ---------------------------------------------------------------------------------
def main(argv=None):
    from .video_reader import video_reader
    p = _parser('python -m solex_ser_recon_en_amd.lineprofile',
                '%(prog)s FILE [--half-width H] [--shift S | --line L] [--range R] '
                '[--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags]',
                'Line core intensity, width, centre of gravity and equivalent width maps of a scan.', 10,
                ('pixels either side of the line measured (1..32)', 'PNG display range of the cog map: +-R pixels to 1 .. 65535',
                 'A / pixel (with --wavelength: the cog map in km/s)', 'A, the line measured'), shift=True)
    args, opts, path, atlas = _cli(p, argv, 'the line-profile maps are single-process: run them without torchrun',
                                   '-w is not a line-profile flag: give the line with --shift or --line')
    try:
        rdr = video_reader(path)
        dispersion, wavelength, shift = _cli_dispersion(rdr, opts, args, atlas)
        res = line_profile_maps(rdr, opts, args.half_width, shift, args.range, dispersion, wavelength)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    out = _write_planes(path, opts, rdr, res, dispersion, wavelength, [(name, 'line_' + name, name, {}) for name in WRITTEN])
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
