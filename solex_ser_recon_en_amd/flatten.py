"""Flatten the disk: the robust radial profile of a finished disk -- the median of every one-pixel ring around the fitted centre,
the centre-to-limb variation in the line -- and the disk divided by it.  The ring medians and the division
are HIP kernels (ops.ring_medians_u16, ops.ring_flatten_u16); turning K medians into K gains is host NumPy in float64, written
step by step so that tests/flatten_ref.py restates it bit for bit.

    python -m solex_ser_recon_en_amd.flatten scan.ser [--shift S] [--smooth N] [--max-gain G] [--contrast] [SHG_MAIN flags]
"""
import argparse
import math
import os
import sys

import numpy as np

from . import disk


def ring_profile(image, circle):
    """The ring statistics of the uint16 device image around circle = (cx, cy, r) -> {'count' uint32 [K], 'lo', 'hi' uint16 [K],
    'median' float64 [K] = (lo + hi) / 2, 'radius' float64 [K] = k + 0.5}, K = floor(r) + 1, on the host."""
    from . import ops
    from .device import to_device_u16
    count, lo, hi = ops.ring_medians_u16(to_device_u16(image), circle)
    count, lo, hi = disk.host_u(count, np.uint32), disk.host_u(lo, np.uint16), disk.host_u(hi, np.uint16)
    return {'count': count, 'lo': lo, 'hi': hi, 'median': (lo.astype(np.float64) + hi.astype(np.float64)) / 2.0,
            'radius': np.arange(count.shape[0], dtype=np.float64) + 0.5}


def filled_profile(profile, smooth=1):
    """gain_from_profile's P: the medians with the empty rings filled, then the running mean."""
    count = np.asarray(profile['count'])
    p = np.array(profile['median'], dtype=np.float64)
    k = p.shape[0]
    if not (isinstance(smooth, (int, np.integer)) and smooth >= 1 and smooth % 2 == 1):
        raise ValueError('smooth must be an odd integer >= 1, got %r' % (smooth,))
    have = np.flatnonzero(count > 0)
    if have.size == 0:
        raise ValueError('no ring holds a pixel: the disk lies outside the image')
    for i in np.flatnonzero(count == 0):
        p[i] = p[have[np.argmin(np.abs(have - i))]]                 # (argmin: the first, hence the lower, index on a tie)
    if smooth > 1:
        half = int(smooth) // 2
        padded = np.concatenate([np.full(half, p[0]), p, np.full(half, p[-1])])
        acc = padded[0:k].copy()
        for i in range(1, int(smooth)):
            acc = acc + padded[i:i + k]
        p = acc / float(smooth)
    return p


def default_level(p):
    """The level the gain aims at: np.median of the first max(1, K // 10) values of the profile P."""
    return np.float64(np.median(p[:max(1, p.shape[0] // 10)]))


def gain_from_profile(profile, smooth=1, level=None, max_gain=8.0):
    """The gain of every ring, float64 [K], from ring_profile's dict:
      P = the medians; a ring without pixels takes the median of the nearest ring that has some (the lower index on a tie;
          ValueError when no ring has any);
      smooth (odd, >= 1; 1: none): P = the running mean over `smooth` rings, the ends replicated: the sum of the window's values
          in index order, one addition at a time, divided by float(smooth);
      level (default): np.median of the first max(1, K // 10) values of P;
      gain = min(level / P, max_gain), and 0 where P = 0.
    The default is smooth = 1: a running mean smears the steep limb."""
    if not (math.isfinite(max_gain) and max_gain >= 0):
        raise ValueError('max_gain must be finite and >= 0')
    p = filled_profile(profile, smooth)
    level = default_level(p) if level is None else np.float64(level)
    if not (np.isfinite(level) and level >= 0):
        raise ValueError('level must be finite and >= 0')
    with np.errstate(divide='ignore', invalid='ignore'):
        gain = np.minimum(level / p, np.float64(max_gain))
    return np.where(p == 0.0, 0.0, gain)


def flatten_disk(image, circle, smooth=1, level=None, max_gain=8.0):
    """-> (the flat uint16 device image, ring_profile's dict, the gain float64 [K])."""
    from . import ops
    from .device import to_device_u16
    t = to_device_u16(image)
    profile = ring_profile(t, circle)
    gain = gain_from_profile(profile, smooth, level, max_gain)
    return ops.ring_flatten_u16(t, circle, gain), profile, gain


def flatten_scan(file_or_reader, options=None, shift=0, smooth=1, level=None, max_gain=8.0, dejitter=None):
    """A scan's disk at `shift` (disk.scan_disk), flattened by flatten_disk.  -> {'image', 'flat' (uint16 device tensors),
    'circle' (of the image), 'profile', 'gain', 'level', 'shift', 'ratio', 'phi', 'crop'}.  ValueError for ratio_fixe / slant_fix (no
    limb fit, hence no circle), de-vignette (a float64 frame) and a frame-sharded reader.  dejitter: disk.scan_disk's; the record then
    holds 'jitter'."""
    scan = disk.scan_disk(file_or_reader, options, shift, dejitter=dejitter)
    image, circle_out = scan['image'], scan['circle']
    flat, profile, gain = flatten_disk(image, circle_out, smooth, level, max_gain)
    used = float(level) if level is not None else float(default_level(filled_profile(profile, smooth)))
    res = {'image': image, 'flat': flat, 'circle': circle_out, 'profile': profile, 'gain': gain, 'level': used, 'shift': scan['shift'],
           'ratio': scan['ratio'], 'phi': scan['phi'], 'crop': scan['crop'], 'smooth': int(smooth), 'max_gain': float(max_gain)}
    if 'jitter' in scan:
        res['jitter'] = scan['jitter']
    return res


# ---- command line ---------------------------------------------------------------------------------
def main(argv=None):
    from .linemaps import _print_json
    from .solex_util import output_path
    from .video_reader import video_reader
    p = argparse.ArgumentParser(prog='python -m solex_ser_recon_en_amd.flatten',
                                usage='%(prog)s FILE [--shift S] [--smooth N] [--max-gain G] [--contrast] [--dejitter] [SHG_MAIN flags]',
                                description='Flatten a scan\'s disk: divide it by the median of every one-pixel ring around the fitted '
                                            'centre, and write that centre-to-limb profile.')
    p.add_argument('--shift', type=int, default=0, help='pixel shift of the disk to flatten (the -w shift; default 0: the line centre)')
    p.add_argument('--smooth', type=int, default=1, help='running mean over N rings (odd; default 1: none)')
    p.add_argument('--max-gain', type=float, default=8.0, help='the largest gain a ring may get (default 8)')
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the flat image (<base>_flat_clahe.png, ...)')
    disk.add_dejitter_argument(p)

    def checks(args):
        if args.smooth < 1 or args.smooth % 2 == 0:
            p.error('--smooth must be odd and >= 1')
        if not (math.isfinite(args.max_gain) and args.max_gain >= 0):
            p.error('--max-gain must be finite and >= 0')

    args, opts, (path,) = disk.parse(p, argv, 'flatten', 'flattening', checks)
    try:
        rdr = video_reader(path)
        res = flatten_scan(rdr, opts, args.shift, args.smooth, None, args.max_gain, {} if args.dejitter else None)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    stem = '%s_shift=%d' % (os.path.splitext(path)[0], res['shift'])
    flat, png, fits = disk.write_image(res['flat'], stem + '_flat', opts, rdr)
    out = {'shape': list(flat.shape), 'shift': res['shift'], 'smooth': res['smooth'], 'max_gain': res['max_gain'], 'png': png, 'fits': fits,
           'clv': None}
    profile, gain, rad = res['profile'], res['gain'], res['circle'][2]
    out['clv'] = output_path(stem + '_clv.txt', opts)
    with open(out['clv'], 'w') as f:
        f.write('# ring  r/R  count  median  gain\n')
        for i in range(gain.shape[0]):
            f.write('%d %.6f %d %.1f %.9g\n' % (i, profile['radius'][i] / rad if rad > 0 else 0.0, profile['count'][i],
                                                profile['median'][i], gain[i]))
    have = np.flatnonzero(profile['count'] > 0)
    # a pixel counts as saturated where the flat image holds 65535 and the image did not
    image = np.rot90(disk.host_u(res['image'].contiguous(), np.uint16), opts['img_rotate'] // 90)
    out.update(rings=int(gain.shape[0]), level=res['level'],
               centre_median=float(profile['median'][have[0]]) if have.size else None,
               limb_median=float(profile['median'][have[-1]]) if have.size else None,
               saturated=int(((flat == 65535) & (image != 65535)).sum()))
    if args.dejitter:
        out['jitter'] = disk.jitter_summary(res['jitter'])
    if args.contrast:
        out['contrast'] = disk.contrast_products(res['flat'], res['circle'], opts, rdr, stem + '_flat')
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
