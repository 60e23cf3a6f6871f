"""Line-bisector maps: the line shift at several depths of the line, at every point of the disk, for the fitted line or any line at
an integer pixel shift, in the geometry of the scan's products (the maps overlay `<base>_shift=<S>_clahe.png` pixel for pixel).  Not
a reference feature: the arithmetic is the one include/shg_hip.h states for shg_line_bisector and shg_line_bisector_finish
(tests/linemaps_ref.py restates it in NumPy).

    python -m solex_ser_recon_en_amd.bisector FILE [--half-width H] [--shift S | --line L] [--levels 0.2,0.4,0.6,0.8] [--widths]
        [--range R] [--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags: -x -s -r W -m ...]

writes <base>_shift=<S>_bisector_<P>.fits (float32, NaN off the disk) and the matching 16-bit .png for every level f, P = 100 f
(as %g), rotated by img_rotate as the other products; with --widths also <base>_shift=<S>_bisector_<P>_chord.{fits,png}.  It prints
one JSON line.  --line L (with --atlas / --anchor) measures the line at wavelength L, as the line-profile CLI does.  The CLI is
single-process: under torchrun it refuses to run.

Per slit row and frame, in the window of H pixels either side of the line: the level at fraction f is (1 - f) core + f continuum
(core: the intensity at the vertex of the parabola through the profile's minimum and its neighbours; continuum: the mean of the
window's end samples), so f = 0.5 is the line-profile maps' half level.  Its crossings either side of the core are linearly
interpolated as the width's; the bisector is their midpoint minus the mean image's line centre (+ = longer wavelength, km/s as
the Dopplergram's), the chord their distance (pixels; at f = 0.5 the line-profile maps' width).  Different depths of a line form at
different heights, so the bisectors at several levels give the line-of-sight velocity against height and the line's asymmetry.
"""
import math
import sys

from . import ops
from .linemaps import _by_plane, _cli, _cli_dispersion, _line_maps, _parser, _print_json, _write_planes

DEFAULT_LEVELS = (0.2, 0.4, 0.6, 0.8)
MAX_LEVELS = 8


def check_levels(levels):
    """levels as a tuple of floats: 1 to 8 finite fractions, strictly increasing, inside (0, 1); else ValueError."""
    try:
        lv = tuple(float(v) for v in levels)
    except (TypeError, ValueError):
        raise ValueError('levels must be a sequence of numbers, got %r' % (levels,))
    if not 1 <= len(lv) <= MAX_LEVELS:
        raise ValueError('between 1 and %d levels are needed, got %d' % (MAX_LEVELS, len(lv)))
    if not all(math.isfinite(v) and 0.0 < v < 1.0 for v in lv):
        raise ValueError('levels must lie strictly between 0 (the core) and 1 (the continuum), got %s' % (lv,))
    if any(b <= a for a, b in zip(lv, lv[1:])):
        raise ValueError('levels must be strictly increasing, got %s' % (lv,))
    return lv


def level_tag(f):
    """The file-name tag of a level: 100 f as %g (0.2 -> '20', 0.35 -> '35', 0.125 -> '12.5')."""
    return '%g' % (100.0 * f)


def line_bisector_maps(file_or_reader, options=None, half_width=10, shift=0, levels=DEFAULT_LEVELS, display_range=2.0,
                       dispersion=None, wavelength=None):
    """The line-bisector maps of one scan -> dict(raw = {(kind, f): float32 [ih, N] per slit row and frame}; maps = {(kind, f):
    float32, the raw plane resampled to the corrected image, NaN off the disk and in the crop's padding, in units[(kind, f)]};
    png = {(kind, f): uint16 display plane of the raw-unit map}, kind 'bisector' or 'chord' and f each of `levels`; levels, circle
    (-1, -1, -1 without a limb fit), circle_out, ratio, phi, crop (the crop_plan, or None), fit [ih, 4], units = {(kind, f): 'pixel' |
    'km/s'}, half_width, shift, display_range, dispersion, wavelength).  The bisectors are in pixels from the line centre (km/s given
    dispersion and wavelength), the chords in pixels; the bisector display plane is 32768 +- 32767 at +-display_range pixels, the
    chord's 1 + v * 65534 / (2H + 1).  The geometry is the ellipse-fit shift's, whatever `shift` is.  options: SHG_MAIN's (as
    dopplergram())."""
    levels = check_levels(levels)
    half_width, shift = int(half_width), int(shift)
    raw, maps, png, res, factor = _line_maps(
        file_or_reader, options, half_width, display_range, dispersion, wavelength,
        'the line-bisector maps of a frame-sharded scan are not supported',
        lambda stack, fit, flip: ops.line_bisector(stack, fit, half_width, levels, shift, flip_x=flip),
        lambda raw, *geometry: ops.line_bisector_finish(raw, *geometry, half_width, display_range), shift)
    keys = [('bisector', f) for f in levels] + [('chord', f) for f in levels]
    return _by_plane(res, keys, {key: 'pixel' for key in keys}, [('bisector', f) for f in levels], raw, maps, png, factor, shift=shift,
                     levels=levels)


# ---- command line ---------------------------------------------------------------------------------
def _own_flags(p):
    p.add_argument('--levels', default=','.join('%g' % f for f in DEFAULT_LEVELS),
                   help='comma-separated fractions from the core (0) to the continuum (1), 1 to 8, strictly increasing')
    p.add_argument('--widths', action='store_true', help='also write the chord (width) map of every level')


def main(argv=None):
    from .video_reader import video_reader
    p = _parser('python -m solex_ser_recon_en_amd.bisector',
                '%(prog)s FILE [--half-width H] [--shift S | --line L] [--levels 0.2,0.4,0.6,0.8] [--widths] [--range R] '
                '[--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags]',
                'Line-bisector maps of a scan: the line shift at several depths of the line.', 10,
                ('pixels either side of the line measured (1..32)', 'PNG display range of the bisector maps: +-R pixels to 1 .. 65535',
                 'A / pixel (with --wavelength: the bisector maps in km/s)', 'A, the line measured'), True, _own_flags)

    def own_checks(args):
        try:
            args.levels = check_levels([v for v in args.levels.split(',')] if args.levels.strip() else [])
        except ValueError as e:
            p.error('--levels: %s' % e)

    args, opts, path, atlas = _cli(p, argv, 'the line-bisector maps are single-process: run them without torchrun',
                                   '-w is not a line-bisector flag: give the line with --shift or --line', own_checks)
    try:
        rdr = video_reader(path)
        dispersion, wavelength, shift = _cli_dispersion(rdr, opts, args, atlas)
        res = line_bisector_maps(rdr, opts, args.half_width, shift, args.levels, args.range, dispersion, wavelength)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    kinds = ('bisector', 'chord') if args.widths else ('bisector',)
    names = [('bisector_%s' % level_tag(f) + ('_chord' if kind == 'chord' else ''), (kind, f)) for f in res['levels'] for kind in kinds]
    out = _write_planes(path, opts, rdr, res, dispersion, wavelength, [(name, name, key, {'LEVEL': float(key[1])}) for name, key in names],
                        levels=list(res['levels']))
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
