"""Limb protection for the filters that follow a stack: deconvolve and sharpen ring at the limb because the
limb is a step, not because of what they do to the disk.  protect() hands a filter two images without the step -- the disk out to
rad - margin continued outwards by a point reflection along every ray, and the sky from rad + margin continued inwards the same
way (ops.limb_split_u16) --, runs the unchanged filter on each, and puts the results back around the band of the limb itself, which
stays as observed (ops.limb_merge_u16).  Both steps are HIP kernels whose arithmetic include/shg_hip.h states exactly.

Out of scope: sharpening the limb itself, an ellipse instead of a circle."""
import math

DEFAULT_BLEND = 4.0
DEFAULT_REACH = 32.0
KEYS = ('circle', 'margin', 'blend', 'reach', 'sky')


def settings(limb, default_margin, circle=None):
    """The `limb` dict of deconvolve_disk / sharpen_disk (keys: margin, blend, reach, sky, circle) with the defaults filled in ->
    (circle, margin, blend, reach, sky).  circle: the caller's own (a scan's limb fit), used when the dict names none.  ValueError for
    an unknown key, no circle, or a value out of range."""
    if not isinstance(limb, dict):
        raise ValueError('limb is a dict with the keys %s, got %r' % (', '.join(KEYS), limb))
    unknown = sorted(set(limb) - set(KEYS))
    if unknown:
        raise ValueError('limb has no key %s (it has %s)' % (', '.join(map(repr, unknown)), ', '.join(KEYS)))
    if limb.get('circle') is not None:
        circle = limb['circle']
    if circle is None or tuple(float(v) for v in circle) == (-1.0, -1.0, -1.0):
        raise ValueError('limb protection needs the disk\'s circle (cx, cy, rad)')
    margin = default_margin if limb.get('margin') is None else limb['margin']
    blend = DEFAULT_BLEND if limb.get('blend') is None else limb['blend']
    reach = DEFAULT_REACH if limb.get('reach') is None else limb['reach']
    return _checked(circle, margin, blend, reach) + (bool(limb.get('sky', True)),)


def _checked(circle, margin, blend, reach):
    """(circle, margin, blend, reach) as floats, reach clipped to rad - margin; ValueError outside the ranges the kernels take."""
    try:
        circle = tuple(float(v) for v in circle)
        margin, blend, reach = float(margin), float(blend), float(reach)
    except (TypeError, ValueError):
        raise ValueError('circle is (cx, cy, rad) and margin, blend and reach are numbers')
    if len(circle) != 3 or not all(math.isfinite(v) for v in circle) or not 0.0 < circle[2] < 16384.0:
        raise ValueError('circle (cx, cy, rad) must be finite with a radius in (0, 16384), got %r' % (circle,))
    if not (math.isfinite(margin) and margin >= 0.0):
        raise ValueError('margin is finite and >= 0, got %r' % margin)
    edge = circle[2] - margin
    if not edge >= 1.0:
        raise ValueError('rad - margin is at least 1, got a radius of %r and a margin of %r' % (circle[2], margin))
    if not (math.isfinite(blend) and blend > 0.0):
        raise ValueError('blend is finite and > 0, got %r' % blend)
    if not (math.isfinite(reach) and reach >= 1.0):
        raise ValueError('reach is finite and >= 1, got %r' % reach)
    return circle, margin, blend, min(reach, edge)


def protect(image, circle, process, margin, blend=DEFAULT_BLEND, reach=DEFAULT_REACH, sky=True):
    """process(plane) -> a uint16 device image of the plane's shape, run on the uint16 device image's disk plane and, with sky, on
    its sky plane, and merged back: inside rad - margin the processed disk plane, beyond rad + margin the processed sky plane (sky
    False: the image as it was), each blended in over `blend` pixels, and the band in between as it was -> (the uint16 device image,
    the record {'circle', 'margin', 'blend', 'reach' (clipped to rad - margin), 'sky'})."""
    from . import ops
    from .device import to_device_u16
    circle, margin, blend, reach = _checked(circle, margin, blend, reach)
    t = to_device_u16(image)
    inner, outer = ops.limb_split_u16(t, circle, margin, reach, want_outer=bool(sky))
    disk_plane = process(inner)
    sky_plane = process(outer) if sky else None
    out = ops.limb_merge_u16(t, disk_plane, sky_plane, circle, margin, blend)
    return out, {'circle': list(circle), 'margin': margin, 'blend': blend, 'reach': reach, 'sky': bool(sky)}


# ---- what the two command lines share ----
def add_arguments(p, default_margin):
    """--limb-protect [MARGIN], --limb-blend, --limb-reach, --limb-disk-only on the parser of deconvolve or sharpen."""
    p.add_argument('--limb-protect', type=float, nargs='?', const=True, default=None, metavar='MARGIN',
                   help='filter the disk and the sky apart and leave the band within MARGIN pixels of the limb as it is: no ringing at '
                        'the limb (default MARGIN: %s; after INPUT, or as --limb-protect=MARGIN)' % default_margin)
    p.add_argument('--limb-blend', type=float, default=None, metavar='B',
                   help='with --limb-protect: the filtered planes fade in over B pixels (default %g)' % DEFAULT_BLEND)
    p.add_argument('--limb-reach', type=float, default=None, metavar='Q',
                   help='with --limb-protect: the planes continue across the limb for Q pixels, then stay level (default %g)' % DEFAULT_REACH)
    p.add_argument('--limb-disk-only', action='store_true', help='with --limb-protect: leave the sky as it is')


def from_arguments(p, args, circle, default_margin):
    """The `limb` dict the flags stand for, or None without --limb-protect; p.error for a --limb-* flag without it and for values
    out of range.  circle: --circle's, or None (a scan brings its own)."""
    if args.limb_protect is None:
        if args.limb_blend is not None or args.limb_reach is not None or args.limb_disk_only:
            p.error('--limb-blend, --limb-reach and --limb-disk-only go with --limb-protect')
        return None
    limb = {'margin': None if args.limb_protect is True else args.limb_protect, 'blend': args.limb_blend, 'reach': args.limb_reach,
            'sky': not args.limb_disk_only}
    if circle is not None:
        limb['circle'] = tuple(circle)
    try:
        # (a scan's circle is not known yet: the ranges that do not need it are checked on a radius that holds any margin)
        probe = limb.get('circle', (0.0, 0.0, 16383.0))
        settings(dict(limb, circle=probe), default_margin)
    except ValueError as e:
        p.error('--limb-protect: %s' % e)
    return limb
