"""Emission-line maps: the Doppler shift, peak, width, centre of gravity and flux of a line seen in EMISSION, in a ring around the
limb (prominences in H-alpha, He D3 off the limb) or, with --on-disk, on the disk as well (flares), in the geometry of the scan's
products (the maps overlay `<base>_shift=<S>_protus.png` pixel for pixel).  Not a reference feature: the arithmetic is the one
include/shg_hip.h states for shg_line_emission and shg_line_emission_finish (tests/emission_ref.py restates it in NumPy).

    python -m solex_ser_recon_en_amd.prominence FILE [--half-width H] [--shift S | --line L] [--min-excess E] [--inner P]
        [--outer F] [--on-disk] [--range R] [--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags: -x -s -r W -m ...]

writes <base>_shift=<S>_emission_{shift,peak,width,cog,flux}.fits (float32, NaN outside the ring and where no emission is found)
and the matching 16-bit .png files, rotated by img_rotate as the other products, and prints one JSON line.  The CLI is
single-process: under torchrun it refuses to run.

Per slit row and frame, in the window of H pixels either side of the line: the background is the mean of the window's end samples;
the pixel is measured only when the window's first maximum lies inside the window and the parabola through it and its neighbours
peaks at least --min-excess (sample units, default 0) above the background.  Scattered disk light off the limb still carries the
absorption line, whose maximum sits on the window's edge, so empty sky is rejected by the bracket rule already; --min-excess rejects
noise bumps (six times the noise's sigma is a good start).  shift = the parabola's vertex minus the mean image's line centre (+ =
longer wavelength, km/s given a dispersion); peak = its height above the background; width = the distance between the crossings of
the level halfway from the background to the peak; cog = the centre of gravity of p - background; flux = sum(p - background).

The ring: the products' circle (cx, cy, rad) with r_in = rad + inner and r_out = rad * outer.  inner defaults to the options'
delta_radius, so the ring's inner edge is `_protus.png`'s black disc; --outer defaults to 1.4 and may be inf.  With ratio_fixe or
slant_fix there is no limb fit, hence no circle and no ring: nothing is masked, and the JSON line says so.
"""
import math
import sys

import numpy as np

from . import ops
from .linemaps import _by_plane, _cli, _cli_dispersion, _line_maps, _parser, _print_json, _write_planes

PLANES = ops.LINE_EMISSION_PLANES
DEFAULT_OUTER = 1.4


def ring_of(circle, inner, outer, on_disk=False):
    """The finish's ring (cx, cy, r_in, r_out) of a circle (cx, cy, rad): r_in = rad + inner (-1: no inner mask, with on_disk),
    r_out = rad * outer; None without a circle."""
    if circle is None or tuple(circle) == (-1, -1, -1):
        return None
    cx, cy, rad = (float(v) for v in circle)
    r_in, r_out = -1.0 if on_disk else max(rad + float(inner), 0.0), rad * float(outer)
    if r_out < r_in:
        raise ValueError('the ring is empty: inner edge %g px beyond the outer edge %g px' % (r_in, r_out))
    return (cx, cy, r_in, r_out)


def ring_mask(shape, ring):
    """bool [h, w]: the pixels the ring keeps (all of them without a ring), by shg_line_emission_finish's float64 steps."""
    if ring is None:
        return np.ones(shape, dtype=bool)
    cx, cy, r_in, r_out = ring
    r = np.arange(shape[0], dtype=np.float64)[:, None]
    c = np.arange(shape[1], dtype=np.float64)[None, :]
    dx, dy = c - cx, r - cy
    d2 = dx * dx + dy * dy
    keep = ~(d2 > r_out * r_out)
    if r_in >= 0:
        keep &= ~(d2 <= r_in * r_in)
    return keep


def ring_stats(m, ring):
    """valid fraction, median and 1st / 99th percentile of a map over the ring (linemaps.disk_stats counts the disk)."""
    on = ring_mask(m.shape, ring)
    v = m[on]
    v = v[np.isfinite(v)]
    out = {'valid_fraction': float(v.size / max(int(on.sum()), 1)), 'median': None, 'p1': None, 'p99': None}
    if v.size:
        p1, med, p99 = np.percentile(v.astype(np.float64), [1, 50, 99])
        out.update(median=float(med), p1=float(p1), p99=float(p99))
    return out


def emission_maps(file_or_reader, options=None, half_width=10, shift=0, min_excess=0.0, inner=None, outer=DEFAULT_OUTER, on_disk=False,
                  display_range=2.0, dispersion=None, wavelength=None):
    """The emission-line maps of one scan -> dict(raw = {plane: float32 [ih, N] per slit row and frame}; maps = {plane: float32, the
    raw plane resampled to the corrected image, NaN outside the ring, where no emission passes the gate and in the crop's padding,
    in units[plane]}; png = {plane: uint16 display plane of the raw-unit map}; ring = (cx, cy, r_in, r_out) in the finish's columns
    and ring_out = the same in the written map's columns (both None without a limb fit); circle, circle_out, ratio, phi, crop, fit,
    units, half_width, shift, min_excess, display_range, dispersion, wavelength).  Planes: shift and cog (pixels, or km/s given
    dispersion and wavelength), peak and flux (sample scale), width (pixels).  inner: pixels added to the limb's radius for the
    ring's inner edge (None: the options' delta_radius); outer: the outer edge as a factor of the radius (>= 1, inf allowed);
    on_disk: no inner mask.  options: SHG_MAIN's (as dopplergram())."""
    from . import SHG_MAIN
    half_width, shift, min_excess, outer = int(half_width), int(shift), float(min_excess), float(outer)
    if not (math.isfinite(min_excess) and min_excess >= 0):
        raise ValueError('min_excess must be finite and >= 0')
    if not outer >= 1:
        raise ValueError('outer must be a factor >= 1 (inf allowed)')
    if inner is None:
        inner = (SHG_MAIN.default_options() if options is None else options)['delta_radius']
    inner = float(inner)
    if not math.isfinite(inner):
        raise ValueError('inner must be finite')
    ring = None

    def finish(raw, h00, h01, h02, out_h, out_w, circle, crop):
        nonlocal ring
        ring = ring_of(circle, inner, outer, on_disk)
        return ops.line_emission_finish(raw, h00, h01, h02, out_h, out_w, ring, crop, half_width, display_range)

    raw, maps, png, res, factor = _line_maps(
        file_or_reader, options, half_width, display_range, dispersion, wavelength,
        'the emission-line maps of a frame-sharded scan are not supported',
        lambda stack, fit, flip: ops.line_emission(stack, fit, half_width, shift, min_excess, flip_x=flip), finish, shift)
    return _by_plane(res, PLANES, {'shift': 'pixel', 'peak': 'adu', 'width': 'pixel', 'cog': 'pixel', 'flux': 'adu'}, ('shift', 'cog'),
                     raw, maps, png, factor, shift=shift, min_excess=min_excess, ring=ring,
                     ring_out=ring_of(res['circle_out'], inner, outer, on_disk))


# ---- command line ---------------------------------------------------------------------------------
def _own_flags(p):
    p.add_argument('--min-excess', type=float, default=0.0,
                   help='sample units the peak must rise above the background (default 0: the bracketed maximum alone decides)')
    p.add_argument('--inner', type=float, help='pixels added to the limb radius for the ring\'s inner edge (default: delta_radius, '
                                               'the black disc of _protus.png)')
    p.add_argument('--outer', type=float, default=DEFAULT_OUTER, help='the ring\'s outer edge as a factor of the limb radius '
                                                                      '(>= 1, default %g; inf: no outer edge)' % DEFAULT_OUTER)
    p.add_argument('--on-disk', action='store_true', help='no inner mask: emission on the disk too (flares)')


def main(argv=None):
    from .video_reader import video_reader
    p = _parser('python -m solex_ser_recon_en_amd.prominence',
                '%(prog)s FILE [--half-width H] [--shift S | --line L] [--min-excess E] [--inner P] [--outer F] [--on-disk] [--range R] '
                '[--dispersion D --wavelength L | --atlas A --anchor L] [SHG_MAIN flags]',
                'Emission-line maps of a scan: Doppler shift, peak, width, centre of gravity and flux of prominences off the limb.', 10,
                ('pixels either side of the line measured (1..32)', 'PNG display range of the shift and cog maps: +-R pixels to 1 .. 65535',
                 'A / pixel (with --wavelength: the shift and cog maps in km/s)', 'A, the line measured'), True, _own_flags)

    def own_checks(args):
        if not (math.isfinite(args.min_excess) and args.min_excess >= 0):
            p.error('--min-excess must be finite and >= 0')
        if args.inner is not None and not math.isfinite(args.inner):
            p.error('--inner must be finite')
        if not args.outer >= 1:
            p.error('--outer must be a factor >= 1 (inf allowed)')

    args, opts, path, atlas = _cli(p, argv, 'the emission-line maps are single-process: run them without torchrun',
                                   '-w is not an emission-map flag: give the line with --shift or --line', own_checks)
    try:
        rdr = video_reader(path)
        dispersion, wavelength, shift = _cli_dispersion(rdr, opts, args, atlas)
        res = emission_maps(rdr, opts, args.half_width, shift, args.min_excess, args.inner, args.outer, args.on_disk, args.range,
                            dispersion, wavelength)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    ring = res['ring_out']
    keys = {'MINEXC': res['min_excess'], 'RINGIN': -1.0 if ring is None else ring[2],
            'RINGOUT': -1.0 if ring is None or math.isinf(ring[3]) else ring[3]}
    out = _write_planes(path, opts, rdr, res, dispersion, wavelength, [(name, 'emission_' + name, name, keys) for name in PLANES],
                        min_excess=res['min_excess'], ring=None if ring is None else [v if math.isfinite(v) else None for v in ring],
                        masked=ring is not None,
                        note=None if ring is not None else 'no limb fit (ratio_fixe / slant_fix): no circle, hence no ring; nothing is masked')
    for name in PLANES:                                            # _write_planes counts the disk: count the ring
        stats = ring_stats(res['maps'][name], ring)
        out['median'][name], out['valid_fraction'][name] = stats['median'], stats['valid_fraction']
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
