"""Dejitter a scan: a spectroheliograph builds the disk one frame a column, so every tracking error along the slit moves one whole
column of the raw disk up or down.  The midpoints of parallel chords of an ellipse -- tilted, sheared, any -- lie on a straight line:
the midpoint of a column's two limb crossings, less a line fitted through all of them, is that column's jitter in pixels, with no
model of the disk and no limb fit.  The crossings (ops.column_limb_u16) and the resampling of every column
along itself by a Keys cubic (ops.column_shift_u16) are HIP kernels, all integers; everything between them is host NumPy in float64,
written step by step so that tests/dejitter_ref.py restates it.

    python -m solex_ser_recon_en_amd.dejitter scan.ser [--shift S] [--level L | --threshold T] [--window K] [--min-chord F]
                                                        [--max-shift M] [--contrast] [SHG_MAIN flags]
"""
import argparse
import math
import os
import sys

import numpy as np

from . import disk

DEFAULT_LEVEL = 0.2
DEFAULT_WINDOW = 5
DEFAULT_MIN_CHORD = 0.3
DEFAULT_CLIP = 3.0
DEFAULT_MAX_SHIFT = 8.0
MIN_COLUMNS = 16
REFITS = 3
ONE = 16384                       # a weight of 1 in Q14


def threshold(image, level=DEFAULT_LEVEL):
    """T = lo + int(level * (hi - lo)) with lo and hi the values at ranks 5 % and 95 % of the uint16 device image (ops.select_u16:
    ranks int(0.05 (n - 1)) and int(0.95 (n - 1)), 0-based).  The level is low on purpose: the continuum limb is about 0.4 of the
    disk's centre, so the half-height of the blurred edge lies near 0.2 of the way up from the sky."""
    from . import ops
    from .device import to_device_u16
    if not (isinstance(level, (int, float, np.integer, np.floating)) and 0.0 < level < 1.0):
        raise ValueError('level lies in (0, 1), got %r' % (level,))
    t = to_device_u16(image)
    n = int(t.shape[0]) * int(t.shape[1])
    lo, hi = (int(v) for v in ops.select_u16(t, [int(0.05 * (n - 1)), int(0.95 * (n - 1))]).cpu().numpy())
    return lo + int(float(level) * (hi - lo))


_level_threshold = threshold           # (measure() has an argument of that name)


def crossings(table, window, threshold):
    """The sub-pixel crossings of ops.column_limb_u16's table (host int32 [w, 6]) -> (top, bottom) float64 [w], NaN for a column
    without a measurement: include/shg_hip.h's two formulas, one IEEE operation a step."""
    t = np.asarray(table).astype(np.int64)
    has = t[:, 0] >= 0
    kt = int(window) * int(threshold)
    half = float(int(window) - 1) / 2.0
    top = np.full(t.shape[0], np.nan)
    bot = np.full(t.shape[0], np.nan)
    i, p, c = t[has, 0], t[has, 1], t[has, 2]
    top[has] = ((i - 1).astype(np.float64) + (kt - p).astype(np.float64) / (c - p).astype(np.float64)) + half
    i, c, n = t[has, 3], t[has, 4], t[has, 5]
    bot[has] = (i.astype(np.float64) + (c - kt).astype(np.float64) / (c - n).astype(np.float64)) + half
    return top, bot


def fit_line(x, y):
    """The least-squares line through (x, y), float64: slope = sum (x - mx)(y - my) / sum (x - mx)^2 about the means, intercept =
    my - slope mx -> (slope, intercept)."""
    mx, my = x.mean(), y.mean()
    dx = x - mx
    slope = float((dx * (y - my)).sum() / (dx * dx).sum())
    return slope, float(my - slope * mx)


def shifts_from_crossings(top, bottom, min_chord=DEFAULT_MIN_CHORD, clip=DEFAULT_CLIP, max_shift=DEFAULT_MAX_SHIFT):
    """The host steps of measure(), on the crossings of every column (NaN: none) -> its record without 'threshold' and 'window'."""
    top, bottom = np.asarray(top, dtype=np.float64), np.asarray(bottom, dtype=np.float64)
    w = top.shape[0]
    x = np.arange(w, dtype=np.float64)
    has = np.isfinite(top) & np.isfinite(bottom)
    if int(has.sum()) < MIN_COLUMNS:
        raise ValueError('only %d columns cross the limb twice: %d are needed to measure the jitter' % (int(has.sum()), MIN_COLUMNS))
    mid = (top + bottom) / 2.0
    chord = bottom - top
    ok = has & (np.where(has, chord, 0.0) >= float(min_chord) * chord[has].max())
    if int(ok.sum()) < MIN_COLUMNS:
        raise ValueError('only %d columns have a chord long enough: %d are needed to measure the jitter' % (int(ok.sum()), MIN_COLUMNS))
    use = ok.copy()
    slope, intercept = fit_line(x[use], mid[use])
    for _ in range(REFITS):
        res = mid[use] - (slope * x[use] + intercept)
        centre = np.median(res)
        sigma = 1.4826 * np.median(np.abs(res - centre))
        keep = ok & (np.abs(np.where(ok, mid - (slope * x + intercept), 0.0) - centre) <= float(clip) * sigma)
        if sigma == 0.0 or int(keep.sum()) < MIN_COLUMNS or np.array_equal(keep, use):
            break
        use = keep
        slope, intercept = fit_line(x[use], mid[use])
    raw = np.where(has, mid - (slope * x + intercept), 0.0)
    measured = ok & (np.abs(raw) <= float(max_shift))
    n = int(measured.sum())
    if n < MIN_COLUMNS:
        raise ValueError('only %d columns are measured: %d are needed to correct the jitter' % (n, MIN_COLUMNS))
    # between measured columns the linear interpolation, beyond the first and the last the nearest measured value
    shift = np.interp(x, x[measured], raw[measured])
    return {'shift': shift, 'measured': measured, 'fitted': use, 'top': top, 'bottom': bottom, 'slope': slope, 'intercept': intercept,
            'rms': float(np.sqrt(np.mean(raw[measured] ** 2))), 'max': float(np.abs(raw[measured]).max()), 'n_measured': n,
            'rejected_by_max_shift': int((ok & ~measured).sum()), 'crossing': int(has.sum())}


def measure(image, threshold=None, level=DEFAULT_LEVEL, window=DEFAULT_WINDOW, min_chord=DEFAULT_MIN_CHORD, clip=DEFAULT_CLIP,
            max_shift=DEFAULT_MAX_SHIFT):
    """The jitter along the slit of a raw disk (uint16 [ih, FrameCount]: rows along the slit, one column a frame), one kernel call
    and then host float64:
      the two crossings of every column at `threshold` (None: threshold(image, level)) with a window of `window` rows;
      midpoint = (top + bottom) / 2, chord = bottom - top; the columns whose chord is at least `min_chord` of the longest one count
        (the limb grazes the short chords);
      a least-squares line through their midpoints, refitted up to three times without the columns further than `clip` robust sigma
        (1.4826 MAD about the residuals' median) from it;
      shift[c] = midpoint[c] - line(c); a column without a measurement, with a short chord or with |shift| > max_shift is unmeasured
        and takes the linear interpolation of its measured neighbours, beyond the measured span the nearest measured value.
    -> {'shift' float64 [w], 'measured' bool [w], 'fitted' bool [w], 'top', 'bottom' float64 [w] (NaN: no crossing), 'slope',
    'intercept' (the line), 'rms', 'max' (of the measured columns' shifts), 'n_measured', 'rejected_by_max_shift', 'crossing' (the
    columns with two crossings), 'threshold', 'window'}.  ValueError for fewer than 16 measured columns."""
    from . import ops
    from .device import to_device_u16
    t = to_device_u16(image)
    for name, v, lo in (('min_chord', min_chord, 0.0), ('clip', clip, 0.0), ('max_shift', max_shift, 0.0)):
        if not (isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v) and v > lo):
            raise ValueError('%s is finite and > %g, got %r' % (name, lo, v))
    if not min_chord <= 1.0:
        raise ValueError('min_chord is at most 1, got %r' % (min_chord,))
    used = _level_threshold(t, level) if threshold is None else threshold
    table = ops.column_limb_u16(t, window, used).cpu().numpy()
    top, bottom = crossings(table, window, used)
    rec = shifts_from_crossings(top, bottom, min_chord, clip, max_shift)
    rec.update(threshold=int(used), window=int(window))
    return rec


def weights(shift):
    """(offset int32 [w], weight int32 [w, 4]) of ops.column_shift_u16 for out[r][c] = img[r + shift[c]][c]: o = floor(shift),
    t = shift - o, the four Keys cubic weights (a = -0.5) of the rows o - 1 .. o + 2 in float64 -- ((-0.5 t + 1) t - 0.5) t,
    (1.5 t - 2.5) t^2 + 1, ((-1.5 t + 2) t + 0.5) t, (0.5 t - 0.5) t^2 --, each rint(. * 16384), and what is missing to 16384 added
    to the second.  Cubic, not linear: a linear shift blurs each column by an amount that depends on its own fraction."""
    s = np.ascontiguousarray(shift, dtype=np.float64).reshape(-1)
    if not np.isfinite(s).all() or (s.size and np.abs(s).max() > 16383.0):
        raise ValueError('a shift is finite and at most 16383 rows')
    o = np.floor(s)
    t = s - o
    k = np.stack([((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * (t * t) + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * (t * t)],
                 axis=1)
    q = np.rint(k * float(ONE)).astype(np.int64)
    q[:, 1] += ONE - q.sum(axis=1)
    return o.astype(np.int32), q.astype(np.int32)


def apply(planes, shift):
    """Every column c of the uint16 device planes ([h, w] or [n, h, w], n up to 64) moved by shift[c] rows in one batched call:
    out[r][c] = planes[r + shift[c]][c], a Keys cubic in Q14 along the column, the rows clamped at both ends -> a new tensor."""
    from . import ops
    offset, weight = weights(shift)
    return ops.column_shift_u16(planes, offset, weight)


def dejitter_scan(file_or_reader, options=None, shift=0, **measure_args):
    """A scan's disk at `shift` with the jitter taken out of the raw disks first: disk.scan_disk(..., dejitter=measure_args) -- the
    jitter is measured on the disk of ellipse_fit_shift, the one the limb fit reads, every extracted plane is corrected, and the
    stages continue as they do -> scan_disk's record plus 'jitter', measure's."""
    return disk.scan_disk(file_or_reader, options, shift, 'dejittering', dejitter=dict(measure_args))


# ---- command line ---------------------------------------------------------------------------------
def main(argv=None):
    from .linemaps import _print_json
    from .solex_util import output_path
    from .video_reader import video_reader
    p = argparse.ArgumentParser(prog='python -m solex_ser_recon_en_amd.dejitter',
                                usage='%(prog)s FILE [--shift S] [--level L | --threshold T] [--window K] [--min-chord F] [--max-shift M] '
                                      '[--contrast] [SHG_MAIN flags]',
                                description='Take a scan\'s jitter along the slit out of its raw disks -- measured from the midpoints of '
                                            'every column\'s two limb crossings -- and write the disk and the shifts.')
    p.add_argument('--shift', type=int, default=0, help='pixel shift of the disk to write (the -w shift; default 0: the line centre)')
    p.add_argument('--level', type=float, default=None, help='the threshold, as a fraction of the way from the sky to the disk (default %g)' % DEFAULT_LEVEL)
    p.add_argument('--threshold', type=int, default=None, help='the threshold in counts, 0 to 65535 (instead of --level)')
    p.add_argument('--window', type=int, default=DEFAULT_WINDOW, help='rows summed before the comparison (odd, 1 to 15; default %d)' % DEFAULT_WINDOW)
    p.add_argument('--min-chord', type=float, default=DEFAULT_MIN_CHORD,
                   help='use the columns whose chord is at least this fraction of the longest (default %g)' % DEFAULT_MIN_CHORD)
    p.add_argument('--max-shift', type=float, default=DEFAULT_MAX_SHIFT,
                   help='a column further than this from the line, in pixels, is interpolated instead (default %g)' % DEFAULT_MAX_SHIFT)
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the image (<base>_shift=<S>_dejitter_clahe.png, ...)')

    def checks(args):
        if args.level is not None and args.threshold is not None:
            p.error('--level and --threshold exclude each other')
        if args.level is not None and not 0.0 < args.level < 1.0:
            p.error('--level lies in (0, 1)')
        if args.threshold is not None and not 0 <= args.threshold <= 65535:
            p.error('--threshold is 0 to 65535')
        if not (1 <= args.window <= 15 and args.window % 2 == 1):
            p.error('--window must be odd and 1 to 15')
        if not (math.isfinite(args.min_chord) and 0.0 < args.min_chord <= 1.0):
            p.error('--min-chord lies in (0, 1]')
        if not (math.isfinite(args.max_shift) and args.max_shift > 0.0):
            p.error('--max-shift must be finite and > 0')

    args, opts, (path,) = disk.parse(p, argv, 'dejitter', 'dejittering', checks)
    try:
        rdr = video_reader(path)
        res = dejitter_scan(rdr, opts, args.shift, threshold=args.threshold, level=DEFAULT_LEVEL if args.level is None else args.level,
                            window=args.window, min_chord=args.min_chord, max_shift=args.max_shift)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    base = os.path.splitext(path)[0]
    stem = '%s_shift=%d_dejitter' % (base, res['shift'])
    host, png, fits = disk.write_image(res['image'], stem, opts, rdr)
    jitter = res['jitter']
    txt = output_path(base + '_jitter.txt', opts)
    with open(txt, 'w') as f:
        f.write('# column  top  bottom  midpoint  line  shift  measured\n')
        for c in range(jitter['shift'].shape[0]):
            f.write('%d %.4f %.4f %.4f %.4f %.4f %d\n' % (c, jitter['top'][c], jitter['bottom'][c], (jitter['top'][c] + jitter['bottom'][c]) / 2.0,
                                                         jitter['slope'] * c + jitter['intercept'], jitter['shift'][c], jitter['measured'][c]))
    out = dict(disk.jitter_summary(jitter), shape=list(host.shape), shift=res['shift'], png=png, fits=fits, txt=txt, contrast=None)
    if args.contrast:
        out['contrast'] = disk.contrast_products(res['image'], res['circle'], opts, rdr, stem)
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
