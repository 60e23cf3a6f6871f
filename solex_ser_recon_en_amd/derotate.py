"""Derotate a disk: the Sun turns about 13.7 degrees a day as seen from Earth, faster at the equator than at the poles, so over a
series of scans the centre of the disk drifts by pixels against the limb.  The motion is known in closed form: every on-disk pixel
is carried to the sphere, turned back about the solar pole by the angle its latitude rotates in the time difference and carried
back to the image, and -- limb darkening belongs to the view, not to the surface -- rescaled by the radial profile of its new radius
over that of its old one.  The resampling is one HIP kernel (ops.derotate_u16); the orientation matrix, the
rotation law and the time of a scan are host steps in float64, restated by tests/derotate_ref.py.

    python -m solex_ser_recon_en_amd.derotate INPUT --north P --b0 B [--mirror] (--dt-minutes M | --to ISO-UTC [--time ISO-UTC])
                                                     [--no-clv] [--rotation A,B,C] [--circle cx,cy,rad] [--shift S] [--contrast]
                                                     [SHG_MAIN flags]
"""
import argparse
import datetime
import math
import os
import struct
import sys

import numpy as np

from . import disk

LAWS = {'snodgrass': (14.71, -2.39, -1.78)}       # A, B, C in degrees a day, sidereal: A + B sin^2(latitude) + C sin^4(latitude)
EARTH_DEG_PER_DAY = 0.9856                        # the Earth's mean orbital motion: sidereal less this is the rate as seen
MAX_RATE = 0.5                                    # ops.DEROTATE_MAX_RATE: |k0| + |k1| + |k2| in radians
SERIES_KEYS = ('north', 'b0', 'mirror', 'times', 'interval', 'law', 'clv')


def orientation(north_deg, b0_deg, mirror=False):
    """The orthonormal matrix M [3, 3] from image coordinates (right, up, towards the observer) to heliographic Cartesian ones
    (west, the north pole, the central meridian on the equator): M = T(b0) F R(north), applied right to left.
      R = [[cos P, sin P, 0], [-sin P, cos P, 0], [0, 0, 1]]: the roll; solar north lies P = north_deg counterclockwise from image-up
          IN THE IMAGE AS GIVEN, mirrored or not, so north is (-sin P, cos P) in the image and R turns it to (0, 1);
      F = diag(-1 if mirror else 1, 1, 1): with north up, west is to the right in the sky and to the left in an east-west flipped
          image (F and T commute: the flip may stand on either side of the tilt, but not of the roll);
      T = [[1, 0, 0], [0, cos B, sin B], [0, -sin B, cos B]]: the tilt; the centre of the disk has the heliographic latitude
          B = b0_deg, so the observer stands at (0, sin B, cos B).
    north = b0 = 0 without mirror is the identity matrix.  The image's north direction (-sin P, cos P, 0) maps to (0, cos B, -sin B)."""
    if not (math.isfinite(north_deg) and math.isfinite(b0_deg) and abs(b0_deg) <= 90.0):
        raise ValueError('north and b0 are finite angles in degrees with |b0| <= 90, got %r and %r' % (north_deg, b0_deg))
    p, b = math.radians(float(north_deg)), math.radians(float(b0_deg))
    flip = np.diag([-1.0 if mirror else 1.0, 1.0, 1.0])
    roll = np.array([[math.cos(p), math.sin(p), 0.0], [-math.sin(p), math.cos(p), 0.0], [0.0, 0.0, 1.0]])
    tilt = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(b), math.sin(b)], [0.0, -math.sin(b), math.cos(b)]])
    return tilt @ flip @ roll


def rotation_law(name_or_triple='snodgrass', synodic=True):
    """(A, B, C) in radians a day: the rotation rate A + B sin^2(latitude) + C sin^4(latitude).  A name of LAWS (sidereal degrees a
    day; 'snodgrass': 14.71, -2.39, -1.78) or a triple in degrees a day; synodic: less the Earth's 0.9856 degrees a day in A, the
    rate as seen from Earth (False for a triple that is already as seen).  These are parameters, not measurements."""
    if isinstance(name_or_triple, str):
        if name_or_triple not in LAWS:
            raise ValueError('rotation law is one of %s or a triple, got %r' % (', '.join(sorted(LAWS)), name_or_triple))
        triple = LAWS[name_or_triple]
    else:
        triple = tuple(float(v) for v in name_or_triple)
        if len(triple) != 3 or not all(math.isfinite(v) for v in triple):
            raise ValueError('a rotation law is three finite rates A, B, C in degrees a day, got %r' % (name_or_triple,))
    a, b, c = triple
    if synodic:
        a = a - EARTH_DEG_PER_DAY
    return math.radians(a), math.radians(b), math.radians(c)


def ser_time(path):
    """The time of a SER file as a datetime (UTC, naive): the header's DateTime_UTC (int64 at byte 170, 100 ns ticks since
    0001-01-01), else its local DateTime (byte 162), else None (both zero: the recorder wrote none).  ValueError for a file shorter
    than the header and for a stamp no datetime holds."""
    with open(path, 'rb') as f:
        head = f.read(178)
    if len(head) < 178:
        raise ValueError('%s is shorter than a SER header' % path)
    local, utc = struct.unpack_from('<qq', head, 162)
    ticks = utc if utc != 0 else local
    if ticks <= 0:
        return None
    try:
        return datetime.datetime(1, 1, 1) + datetime.timedelta(microseconds=ticks // 10)
    except OverflowError:
        raise ValueError('%s holds a time stamp beyond the year 9999 (%d ticks): give the time' % (path, ticks))


def parse_time(value):
    """A time as a naive UTC datetime: a datetime (an aware one is converted), or ISO 8601 text ('2024-05-01T10:15:30', a trailing Z
    or an offset allowed)."""
    if isinstance(value, datetime.datetime):
        t = value
    else:
        try:
            text = str(value).strip()
            t = datetime.datetime.fromisoformat(text[:-1] + '+00:00' if text.endswith(('Z', 'z')) else text)
        except ValueError:
            raise ValueError('a time is ISO 8601 UTC text such as 2024-05-01T10:15:30, got %r' % (value,))
    if t.tzinfo is not None:
        t = t.astimezone(datetime.timezone.utc).replace(tzinfo=None)
    return t


def days_between(time, to):
    """to - time in days (float64)."""
    return (parse_time(to) - parse_time(time)).total_seconds() / 86400.0


def rates(dt_days, law='snodgrass'):
    """rate3 = (k0, k1, k2) of ops.derotate_u16: the law's radians a day, as seen from Earth, times dt_days.  law: a name of LAWS, or
    a triple A, B, C in degrees a day that is already as seen (the command lines' --rotation).  ValueError beyond |k0| + |k1| + |k2|
    = 0.5 radians, about 1.9 days at the default law."""
    if not math.isfinite(dt_days):
        raise ValueError('the time difference is finite, got %r' % (dt_days,))
    abc = rotation_law(law, synodic=isinstance(law, str))
    k = tuple(float(v) * float(dt_days) for v in abc)
    if not (all(math.isfinite(v) for v in k) and sum(abs(v) for v in k) <= MAX_RATE):
        raise ValueError('a time difference of %.4g days turns the Sun by up to %.3g radians: the limit is %g (about 1.9 days at the '
                         'default law), beyond which too much of the disk comes from behind the limb' % (dt_days, sum(abs(v) for v in k), MAX_RATE))
    return k


def largest_angle(rate3):
    """The largest |a| = |(k2 s2 + k1) s2 + k0| over s2 = sin^2(latitude) in [0, 1]: at an end or at the parabola's vertex."""
    k0, k1, k2 = (float(v) for v in rate3)
    at = [0.0, 1.0]
    if k2 != 0.0 and 0.0 < -k1 / (2.0 * k2) < 1.0:
        at.append(-k1 / (2.0 * k2))
    return max(abs((k2 * s2 + k1) * s2 + k0) for s2 in at)


def largest_displacement(circle, rate3):
    """An upper bound of any pixel's displacement, in pixels, in closed form: a point of the unit sphere turned by a about the pole
    moves along a chord of at most 2 sin(|a| / 2), and the projection shortens it: 2 rad sin(largest_angle / 2).  With B0 = 0 a point
    on the equator half the angle before the central meridian reaches it."""
    return 2.0 * float(circle[2]) * math.sin(largest_angle(rate3) / 2.0)


# shg_derotate_u16's sine and cosine (include/shg_hip.h): the float64 nearest to +-1 / k!, Horner from the highest term down
_SIN = (-7.647163731819816e-13, 1.6059043836821613e-10, -2.505210838544172e-08, 2.7557319223985893e-06, -0.0001984126984126984,
        0.008333333333333333, -0.16666666666666666, 1.0)
_COS = (4.779477332387385e-14, -1.1470745597729725e-11, 2.08767569878681e-09, -2.755731922398589e-07, 2.48015873015873e-05,
        -0.001388888888888889, 0.041666666666666664, -0.5, 1.0)


def behind_limb(shape, circle, matrix, rate3, rows=256):
    """The number of on-disk pixels with a != 0 whose source lies behind the limb -- the pixels shg_derotate_u16 leaves as they are
    for that reason --, counted on the host over the disk's bounding box with the header's own steps 1 to 5 in float64, operation
    for operation (NumPy fuses nothing), so that p_z has the kernel's bits and the count is the kernel's.  A host pass of about a
    hundred array operations over the box: about 0.4 s for a 2000 x 2000 disk."""
    h, w = int(shape[0]), int(shape[1])
    cx, cy, rad = (np.float64(v) for v in circle)
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
    k0, k1, k2 = (np.float64(v) for v in rate3)
    if not rad > 0.0:
        return 0
    c0, c1 = max(0, int(math.floor(cx - rad))), min(w, int(math.ceil(cx + rad)) + 1)
    r0, r1 = max(0, int(math.floor(cy - rad))), min(h, int(math.ceil(cy + rad)) + 1)
    cols = ((np.arange(c0, c1, dtype=np.float64) - cx) / rad)[None, :]
    count = 0
    for lo in range(r0, r1, rows):
        v = np.broadcast_to(((cy - np.arange(lo, min(lo + rows, r1), dtype=np.float64)) / rad)[:, None], (min(lo + rows, r1) - lo, c1 - c0))
        u = np.broadcast_to(cols, v.shape)
        d2 = u * u + v * v
        on = d2 < 1.0
        u, v, d2 = np.where(on, u, 0.0), np.where(on, v, 0.0), np.where(on, d2, 0.0)
        z = np.sqrt(1.0 - d2)
        qx, qy, qz = ((m[i, 0] * u + m[i, 1] * v) + m[i, 2] * z for i in range(3))
        s2 = qy * qy
        a = (k2 * s2 + k1) * s2 + k0
        a2 = a * a
        sa = np.full_like(a, _SIN[0])
        for coefficient in _SIN[1:]:
            sa = sa * a2 + coefficient
        sa = a * sa
        ca = np.full_like(a, _COS[0])
        for coefficient in _COS[1:]:
            ca = ca * a2 + coefficient
        sx, sz = qx * ca - qz * sa, qx * sa + qz * ca
        pz = (m[0, 2] * sx + m[1, 2] * qy) + m[2, 2] * sz
        count += int((on & (a != 0.0) & ~(pz > 0.0)).sum())
    return count


def measured_clv(image, circle, smooth=1):
    """The limb-darkening table of the uint16 device image: the ring medians (flatten.ring_profile), the empty rings filled from
    their nearest neighbour and the running mean (flatten.filled_profile) -- the innermost ring is empty when the centre lies off the
    image and then takes its neighbour's value --, and no value below one count: the table divides."""
    from . import flatten
    p = flatten.filled_profile(flatten.ring_profile(image, circle), smooth)
    return np.maximum(p, 1.0)


def derotate_disk(image, circle, dt_days, north, b0, mirror=False, law='snodgrass', clv='measure', smooth=1, count_behind=True):
    """The uint16 image of a disk with circle (cx, cy, r) as it would look dt_days later (negative: earlier): ops.derotate_u16 with
    orientation(north, b0, mirror) and rates(dt_days, law).  north: the angle of solar north in THIS image, degrees counterclockwise
    from image-up; b0: the heliographic latitude of the disk's centre.  clv: 'measure' (measured_clv of this image, `smooth` rings),
    None (pixels move, values stay: about 40 % of the error stays as an east-west ramp) or K = floor(r) + 1 positive, finite values.
    -> (the uint16 device image, {'dt_days', 'a_equator' (k0, radians), 'rate3', 'matrix', 'max_px' (largest_displacement: a bound in
    closed form), 'behind_limb' (behind_limb's count -- a host pass over the disk --, None with count_behind=False), 'rings' (K),
    'clv' (the host table or None)}).  dt_days = 0 returns the image bit for bit."""
    import torch
    from . import ops
    from .device import to_device_u16
    t = to_device_u16(image)
    matrix = orientation(north, b0, mirror)
    rate3 = rates(dt_days, law)
    c3 = tuple(float(v) for v in circle)
    rings = int(math.floor(c3[2])) + 1
    if isinstance(clv, str):
        if clv != 'measure':
            raise ValueError('clv is \'measure\', None or a table of %d values, got %r' % (rings, clv))
        table = measured_clv(t, c3, smooth)
    elif clv is not None:
        table = np.ascontiguousarray(clv, dtype=np.float64).reshape(-1)
        if table.shape != (rings,) or not (np.isfinite(table).all() and (table > 0.0).all()):
            raise ValueError('clv holds %d positive, finite values (floor(r) + 1)' % rings)
    else:
        table = None
    out = ops.derotate_u16(t, c3, matrix, rate3, None if table is None else torch.from_numpy(table).to(t.device))
    return out, {'dt_days': float(dt_days), 'a_equator': rate3[0], 'rate3': rate3, 'matrix': matrix,
                 'max_px': largest_displacement(c3, rate3), 'behind_limb': behind_limb(t.shape, c3, matrix, rate3) if count_behind else None,
                 'rings': rings, 'clv': table}


def north_in_scan(north, opts):
    """The angle of solar north in a scan's disk as disk.scan_disk returns it, from the angle in the product as it is written: the
    products are turned counterclockwise by img_rotate (a multiple of 90 degrees) on their way out.  north is the angle in the image
    as given whether it is mirrored or not (orientation), so the same subtraction holds with mirror."""
    return float(north) - 90.0 * (int(opts['img_rotate']) // 90)


def derotate_scan(file_or_reader, options=None, shift=0, to=None, time=None, dt_days=None, north=0.0, b0=0.0, mirror=False, law='snodgrass',
                  clv='measure', smooth=1):
    """A scan's disk at `shift` (disk.scan_disk, with its refusals) derotated to the time `to`: dt_days, or to - time with time the
    scan's (default: ser_time of the file; ValueError when it has none).  north is the angle in the product as written
    (north_in_scan takes img_rotate out).  -> scan_disk's record plus 'derotated' (the uint16 device image) and 'derotate'
    (derotate_disk's record plus 'time' and 'to')."""
    from . import SHG_MAIN
    opts = SHG_MAIN.default_options() if options is None else dict(options)
    if dt_days is None:
        if to is None:
            raise ValueError('derotating needs the time to derotate to, or the time difference')
        if time is None:
            if hasattr(file_or_reader, 'device_stack'):
                raise ValueError('a reader has no time stamp: give the scan\'s time')
            time = ser_time(file_or_reader)
            if time is None:
                raise ValueError('%s holds no time stamp: give the scan\'s time' % file_or_reader)
        dt_days = days_between(time, to)
    rates(dt_days, law)                                            # (refuse before the scan is read)
    orientation(north, b0, mirror)
    scan = disk.scan_disk(file_or_reader, opts, shift, 'derotating')
    out, record = derotate_disk(scan['image'], scan['circle'], dt_days, north_in_scan(north, opts), b0, mirror, law, clv, smooth)
    record.update(time=None if time is None else parse_time(time).isoformat(), to=None if to is None else parse_time(to).isoformat())
    return dict(scan, derotated=out, derotate=record)


def summary(record):
    """What a command line prints of derotate_disk's record."""
    return {'dt_minutes': record['dt_days'] * 1440.0, 'a_equator': record['a_equator'], 'max_px': record['max_px'],
            'behind_limb': record['behind_limb'], 'rings': record['rings']}


# ---- the flags derotate and stack --derotate share ---------------------------------------------------
def _floats(text):
    try:
        return [float(v) for v in text.split(',') if v.strip() != '']
    except ValueError:
        raise argparse.ArgumentTypeError('a comma-separated list of numbers, got %r' % text)


def add_arguments(p):
    p.add_argument('--north', type=float, default=None, help='angle of solar north in the written image, degrees counterclockwise from up')
    p.add_argument('--b0', type=float, default=None, help='heliographic latitude of the disk\'s centre in degrees (B0)')
    p.add_argument('--mirror', action='store_true', help='the image is flipped east-west')
    p.add_argument('--rotation', type=_floats, default=None,
                   help='the rotation law A,B,C in degrees a day as seen from Earth (default %g,%g,%g less %g: Snodgrass & Ulrich 1990)'
                        % (LAWS['snodgrass'] + (EARTH_DEG_PER_DAY,)))
    p.add_argument('--no-clv', action='store_true', help='move the pixels only: no limb-darkening ratio')


def check_arguments(p, args):
    """The shared flags' refusals -> the law as rates() takes it."""
    if args.north is None or args.b0 is None:
        p.error('derotating needs --north and --b0: the orientation depends on mount and camera')
    if not (math.isfinite(args.north) and math.isfinite(args.b0) and abs(args.b0) <= 90.0):
        p.error('--north and --b0 are finite angles in degrees, |b0| <= 90')
    if args.rotation is None:
        return 'snodgrass'
    if len(args.rotation) != 3 or not all(math.isfinite(v) for v in args.rotation):
        p.error('--rotation is A,B,C in degrees a day')
    return tuple(args.rotation)


# ---- a series of scans: stack --derotate -------------------------------------------------------------
def series_plan(files, options=None, north=None, b0=None, mirror=False, times=None, interval=None, law='snodgrass', clv='measure'):
    """stack_scans(derotate={...}) checked before a scan is read -> the plan {'north' (in the scans' disks: north_in_scan), 'b0',
    'mirror', 'law', 'clv', 'times' (a naive UTC datetime a file)}.  times: one a file (parse_time's), or None: `interval` seconds
    between consecutive files, or else every file's ser_time -- a file without one is a ValueError that names it."""
    from . import SHG_MAIN
    files = list(files)
    if north is None or b0 is None:
        raise ValueError('derotating needs north and b0: the orientation depends on mount and camera')
    orientation(north, b0, mirror)
    rotation_law(law, synodic=isinstance(law, str))
    if not (clv is None or (isinstance(clv, str) and clv == 'measure')):
        raise ValueError('a series measures its limb darkening or leaves it: clv is \'measure\' or None, got %r' % (clv,))
    if times is not None and interval is not None:
        raise ValueError('give the times or the interval, not both')
    if times is not None:
        times = [parse_time(t) for t in times]
        if len(times) != len(files):
            raise ValueError('%d times for %d scans' % (len(times), len(files)))
    elif interval is not None:
        if not (isinstance(interval, (int, float)) and math.isfinite(interval)):
            raise ValueError('the interval is a finite number of seconds, got %r' % (interval,))
        times = [datetime.datetime(2000, 1, 1) + datetime.timedelta(seconds=float(interval) * i) for i in range(len(files))]
    else:
        times = []
        for f in files:
            t = None if hasattr(f, 'device_stack') else ser_time(f)
            if t is None:
                raise ValueError('%s holds no time stamp: give the times or the interval' % (f,))
            times.append(t)
    opts = SHG_MAIN.default_options() if options is None else options
    return {'north': north_in_scan(north, opts), 'b0': float(b0), 'mirror': bool(mirror), 'law': law, 'clv': clv, 'times': times}


def derotate_series(images, circles, plan, reference):
    """Every image but the reference's derotated to the reference's time, on its own grid with its own circle; the reference is not
    resampled -> (the images, derotate_disk's record a file -- the reference's with rates of zero, nothing moved and no table; 'behind_limb'
    is None for the others: a series skips that host pass).  Every time difference is checked against the range before the first
    kernel runs."""
    days = [days_between(t, plan['times'][reference]) for t in plan['times']]
    for dt in days:
        rates(dt, plan['law'])
    out, records = [], []
    for i, (image, circle) in enumerate(zip(images, circles)):
        if i == reference:
            out.append(image)
            records.append({'dt_days': 0.0, 'a_equator': 0.0, 'rate3': (0.0, 0.0, 0.0), 'matrix': orientation(plan['north'], plan['b0'], plan['mirror']),
                            'max_px': 0.0, 'behind_limb': 0, 'rings': int(math.floor(circle[2])) + 1, 'clv': None})
            continue
        moved, record = derotate_disk(image, circle, days[i], plan['north'], plan['b0'], plan['mirror'], plan['law'], plan['clv'],
                                      count_behind=False)
        out.append(moved)
        records.append(record)
    return out, records


def add_series_arguments(p):
    p.add_argument('--derotate', action='store_true', help='take the differential rotation out of every scan, to the reference\'s time, before '
                                                           'the registration (needs --north and --b0)')
    add_arguments(p)
    p.add_argument('--times', default=None, help='--derotate: the scans\' times T0,T1,... in ISO 8601 UTC, one a file (default: the SER headers\')')
    p.add_argument('--interval', type=float, default=None, help='--derotate: seconds between consecutive scans (instead of --times)')


def series_from_arguments(p, args):
    """stack_scans' derotate dict from the flags of add_series_arguments, or None without --derotate (any of the others is then an error)."""
    given = [flag for flag, on in (('--north', args.north is not None), ('--b0', args.b0 is not None), ('--mirror', args.mirror),
                                   ('--times', args.times is not None), ('--interval', args.interval is not None),
                                   ('--rotation', args.rotation is not None), ('--no-clv', args.no_clv)) if on]
    if not args.derotate:
        if given:
            p.error('%s needs --derotate' % given[0])
        return None
    law = check_arguments(p, args)
    if args.times is not None and args.interval is not None:
        p.error('--times and --interval exclude each other')
    if args.interval is not None and not math.isfinite(args.interval):
        p.error('--interval is a finite number of seconds')
    times = None
    if args.times is not None:
        try:
            times = [parse_time(t) for t in args.times.split(',')]
        except ValueError as e:
            p.error(str(e))
    return {'north': args.north, 'b0': args.b0, 'mirror': args.mirror, 'times': times, 'interval': args.interval, 'law': law,
            'clv': None if args.no_clv else 'measure'}


# ---- command line ---------------------------------------------------------------------------------
def main(argv=None):
    from .linemaps import _print_json
    from .video_reader import video_reader
    p = argparse.ArgumentParser(prog='python -m solex_ser_recon_en_amd.derotate',
                                usage='%(prog)s INPUT --north P --b0 B [--mirror] (--dt-minutes M | --to ISO-UTC [--time ISO-UTC]) [--no-clv] '
                                      '[--rotation A,B,C] [--circle cx,cy,rad] [--shift S] [--contrast] [SHG_MAIN flags]',
                                description='Take the Sun\'s differential rotation out of a disk: the image as it would look at another '
                                            'time.  INPUT is a SER or AVI scan, or a 16-bit grey PNG this package wrote (with --circle).')
    add_arguments(p)
    p.add_argument('--dt-minutes', type=float, default=None, help='the time difference in minutes, target less image (instead of --to)')
    p.add_argument('--to', default=None, help='the time to derotate to, ISO 8601 UTC')
    p.add_argument('--time', default=None, help='the time of the image, ISO 8601 UTC (default: the SER header\'s)')
    p.add_argument('--circle', type=_floats, default=None, help='cx,cy,rad of the disk in a PNG')
    p.add_argument('--shift', type=int, default=0, help='pixel shift of a scan\'s disk (the -w shift; default 0: the line centre)')
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the derotated image (<base>_derot_clahe.png, ...)')
    law = []

    def checks(args):
        law.append(check_arguments(p, args))
        if (args.dt_minutes is None) == (args.to is None):
            p.error('give one of --dt-minutes and --to')
        if args.time is not None and args.to is None:
            p.error('--time goes with --to')
        if args.circle is not None and (len(args.circle) != 3 or not all(math.isfinite(v) for v in args.circle) or not 0.0 < args.circle[2] < 16384.0):
            p.error('--circle is cx,cy,rad with a radius in (0, 16384)')
        try:
            for text in (args.to, args.time):
                if text is not None:
                    parse_time(text)
            if args.dt_minutes is not None:
                rates(args.dt_minutes / 1440.0, law[0])
        except ValueError as e:
            p.error(str(e))

    def file_checks(args, files):
        is_png = files[0].lower().endswith('.png')
        if is_png and args.circle is None:
            p.error('a PNG needs --circle cx,cy,rad')
        if not is_png and args.circle is not None:
            p.error('--circle goes with a PNG: a scan brings its own limb fit')
        if is_png and args.to is not None and args.time is None:
            p.error('a PNG holds no time: give --time, or --dt-minutes')

    args, opts, (path,) = disk.parse(p, argv, 'derotate', 'derotating', checks, file_checks, need='exactly one SER, AVI or PNG file is needed',
                                     png=True)
    law = law[0]
    clv = None if args.no_clv else 'measure'
    dt_days = None if args.dt_minutes is None else args.dt_minutes / 1440.0
    try:
        if path.lower().endswith('.png'):
            img, header_source, stem = disk.png_input(path, opts)
            if dt_days is None:
                dt_days = days_between(args.time, args.to)
            out, record = derotate_disk(img, tuple(args.circle), dt_days, args.north, args.b0, args.mirror, law, clv)
            res = {'circle': tuple(args.circle), 'ratio': None, 'phi': None, 'crop': None}
            shift = None
        else:
            header_source = video_reader(path)
            res = derotate_scan(path, opts, args.shift, args.to, args.time, dt_days, args.north, args.b0, args.mirror, law, clv)
            out, record, shift = res['derotated'], res['derotate'], res['shift']
            stem = '%s_shift=%d' % (os.path.splitext(path)[0], shift)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    host, png, fits = disk.write_image(out, stem + '_derot', opts, header_source)
    line = dict(summary(record), input=path, shape=list(host.shape), shift=shift, north=args.north, b0=args.b0, mirror=bool(args.mirror),
                clv=not args.no_clv, png=png, fits=fits, contrast=None)
    if args.contrast:
        line['contrast'] = disk.contrast_products(out, tuple(res['circle']), opts, header_source, stem + '_derot')
    return _print_json(line, res)


if __name__ == '__main__':
    sys.exit(main())
