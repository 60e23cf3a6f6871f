"""Sharpen a disk: the undecimated B3-spline ("a trous") wavelet layers of a 16-bit image, one gain a layer
and a soft noise gate on the finest layers -- the "wavelets" step that follows a stack.  The decomposition, the recombination and
the noise measure are HIP kernels in integers (ops.wavelet_sharpen_u16, ops.wavelet_noise_u16); what turns gains, a noise level and
gate factors into their integer arguments is host float64, written step by step so that the tests restate it.

    python -m solex_ser_recon_en_amd.sharpen INPUT [--levels L] [--gains g1,..] [--denoise k1,..] [--sigma X] [--circle cx,cy,rad]
        [--region F] [--shift S] [--contrast] [--limb-protect [MARGIN]] [--limb-blend B] [--limb-reach Q] [--limb-disk-only]
        [SHG_MAIN flags]

The limb's edge overshoots into the sky unless --limb-protect (limb=) is given: the layers are then taken of a disk plane and a sky
plane that have no step, and the band of the limb stays as it is (limbguard.py).  Out of scope: any change
to the stack or flatten command lines.
Deconvolution by the instrument-and-seeing blur is a step of its own, before this one (deconvolve.py): its
_deconv.png is an input here.
"""
import argparse
import math
import os
import sys

import numpy as np

from . import disk, limbguard

MAX_LEVELS = 6
MAX_GAIN = 16.0
MAX_THRESHOLD_Q6 = 1 << 22
MAD_TO_SIGMA = 0.6744897501960817            # the median of |x| of a unit normal x
DEFAULT_LEVELS = 4
DEFAULT_GAINS = (1.0, 1.8, 1.4, 1.0)
DEFAULT_DENOISE = (3.0, 1.0, 0.0, 0.0)
DEFAULT_REGION = 0.9
DEFAULT_LIMB_MARGIN = 6.0


def quantise_gains(gains):
    """rint(256 g) of every gain, int64 [L]; ValueError for none or more than six, or one outside [0, 16] (or not finite)."""
    g = np.asarray(list(gains), dtype=np.float64).reshape(-1)
    if not 1 <= g.size <= MAX_LEVELS:
        raise ValueError('1 to %d gains (one a layer), got %d' % (MAX_LEVELS, g.size))
    if not (np.isfinite(g).all() and (g >= 0.0).all() and (g <= MAX_GAIN).all()):
        raise ValueError('a gain lies in [0, %g], got %s' % (MAX_GAIN, g.tolist()))
    return np.rint(g * 256.0).astype(np.int64)


def _check_levels(levels):
    if not (isinstance(levels, (int, np.integer)) and 1 <= levels <= MAX_LEVELS):
        raise ValueError('levels is an integer from 1 to %d, got %r' % (MAX_LEVELS, levels))
    return int(levels)


def noise_factors(levels):
    """The standard deviation of unit white noise in each of the `levels` layers: the root of the sum of squares of the unrounded
    transform's response to a unit impulse, computed here in float64 on a grid that holds the widest response."""
    levels = _check_levels(levels)
    half = 2 * ((1 << levels) - 1)                                  # the reach of c_L's kernel
    n = 2 * half + 1
    c = np.zeros((n, n), dtype=np.float64)
    c[half, half] = 1.0
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    out = []
    for j in range(levels):
        hole = 1 << j
        pad = np.pad(c, 2 * hole)                                   # (zeros: the response never reaches the grid's border)
        rows = sum(k[l] * pad[:, l * hole:l * hole + n] for l in range(5))
        nxt = sum(k[i] * rows[i * hole:i * hole + n, :] for i in range(5))
        w = c - nxt
        out.append(float(np.sqrt((w * w).sum())))
        c = nxt
    return out


def sigma_from_median(median_q6):
    """The noise in counts that a median |w_1| of median_q6 (64 a count) stands for: median / 64 / 0.6745 / noise_factors(1)[0]."""
    return float(median_q6) / 64.0 / MAD_TO_SIGMA / noise_factors(1)[0]


def thresholds(sigma, denoise, levels):
    """rint(64 k_j sigma f_j) clipped to [0, 2^22], int64 [levels]: the gate of layer j at k_j of that layer's noise.  denoise shorter
    than levels is padded with 0."""
    levels = _check_levels(levels)
    k = np.asarray(list(denoise), dtype=np.float64).reshape(-1)
    if k.size > levels:
        raise ValueError('%d denoise factors for %d levels' % (k.size, levels))
    if not (np.isfinite(k).all() and (k >= 0.0).all()):
        raise ValueError('a denoise factor is finite and >= 0, got %s' % k.tolist())
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError('sigma is finite and >= 0, got %r' % (sigma,))
    k = np.concatenate([k, np.zeros(levels - k.size)])
    f = np.asarray(noise_factors(levels), dtype=np.float64)
    return np.clip(np.rint(64.0 * k * np.float64(sigma) * f), 0, MAX_THRESHOLD_Q6).astype(np.int64)


def _noise_circle(circle, region):
    if not (math.isfinite(region) and region > 0.0):
        raise ValueError('region is finite and > 0, got %r' % (region,))
    if circle is None:
        return None
    cx, cy, rad = (float(v) for v in circle)
    if (cx, cy, rad) == (-1.0, -1.0, -1.0):
        return None
    if not (math.isfinite(cx) and math.isfinite(cy) and math.isfinite(rad) and rad >= 0.0):
        raise ValueError('circle (%r, %r, %r) must be finite with a radius >= 0' % (cx, cy, rad))
    return (cx, cy, rad * float(region))


def estimate_sigma(image, circle=None, region=DEFAULT_REGION):
    """The noise of the uint16 device image in counts, from the finest wavelet layer: the lower median of |w_1| over the pixels within
    region * rad of the circle's centre (circle None: every pixel) -> (sigma, the median in Q6, the number of pixels)."""
    from . import ops
    from .device import to_device_u16
    both = ops.wavelet_noise_u16(to_device_u16(image), _noise_circle(circle, region)).cpu().numpy()
    median, count = int(both[0]), int(both[1])
    return sigma_from_median(median), median, count


def sharpen_disk(image, gains, denoise=(), sigma=None, circle=None, region=DEFAULT_REGION, limb=None):
    """The uint16 device image sharpened: len(gains) layers, layer j times gains[j] after a soft threshold at denoise[j] times the
    layer's noise (denoise shorter than gains: 0 beyond it).  sigma None: estimate_sigma(image, circle, region) -> (the sharpened
    uint16 device image, the record {'levels', 'gains' (as quantised), 'gain_q8', 'denoise', 'sigma', 'median_q6', 'pixels' (None
    with a given sigma), 'threshold_q6', 'thresholds' (in counts)}).  limb: a dict {'circle' (default: `circle`), 'margin' (default 6),
    'blend', 'reach', 'sky'} sharpens under limbguard.protect -- the disk plane and, unless sky is False, the sky plane, both with
    the thresholds of the noise measured once, on the image itself --, and the record gains 'limb', protect's."""
    from . import ops
    from .device import to_device_u16
    t = to_device_u16(image)
    gain_q8 = quantise_gains(gains)
    levels = int(gain_q8.size)
    median = pixels = None
    if sigma is None:
        sigma, median, pixels = estimate_sigma(t, circle, region)
    thr = thresholds(float(sigma), denoise, levels)
    k = [float(v) for v in denoise] + [0.0] * (levels - len(list(denoise)))
    record = {'levels': levels, 'gains': (gain_q8 / 256.0).tolist(), 'gain_q8': gain_q8.tolist(), 'denoise': k, 'sigma': float(sigma),
              'median_q6': median, 'pixels': pixels, 'threshold_q6': thr.tolist(), 'thresholds': (thr / 64.0).tolist()}
    if limb is None:
        out, _ = ops.wavelet_sharpen_u16(t, gain_q8, thr)
        return out, record
    ring, margin, blend, reach, sky = limbguard.settings(limb, DEFAULT_LIMB_MARGIN, circle)
    out, record['limb'] = limbguard.protect(t, ring, lambda plane: ops.wavelet_sharpen_u16(plane, gain_q8, thr)[0], margin, blend, reach, sky)
    return out, record


def wavelet_planes(image, levels):
    """The layers of the uint16 device image: an int32 device tensor [levels + 1, h, w] in Q6 (64 a count): w_1 .. w_L, then the
    smooth rest c_L; they sum to 64 * image."""
    from . import ops
    from .device import to_device_u16
    return ops.wavelet_sharpen_u16(to_device_u16(image), [256] * _check_levels(levels), want_planes=True)[1]


def sharpen_scan(file_or_reader, options=None, shift=0, gains=DEFAULT_GAINS, denoise=DEFAULT_DENOISE, sigma=None, region=DEFAULT_REGION,
                 limb=None, dejitter=None):
    """A scan's disk at `shift` (disk.scan_disk, with its refusals: ratio_fixe / slant_fix, de-vignette, a frame
    shard), sharpened by sharpen_disk with the noise measured inside region * rad of the fitted circle -> {'image', 'sharp' (uint16
    device tensors), 'circle', 'record', 'shift', 'ratio', 'phi', 'crop'}.  limb: sharpen_disk's dict without 'circle': the scan's own
    limb fit is the circle.  dejitter: disk.scan_disk's; the result then holds 'jitter'."""
    scan = disk.scan_disk(file_or_reader, options, shift, 'sharpening', dejitter)
    if limb is not None and (not isinstance(limb, dict) or limb.get('circle') is not None):
        raise ValueError('a scan brings its own limb fit: limb is a dict without a circle')
    sharp, record = sharpen_disk(scan['image'], gains, denoise, sigma, scan['circle'], region, limb)
    res = {'image': scan['image'], 'sharp': sharp, 'circle': scan['circle'], 'record': record, 'shift': scan['shift'],
           'ratio': scan['ratio'], 'phi': scan['phi'], 'crop': scan['crop']}
    if 'jitter' in scan:
        res['jitter'] = scan['jitter']
    return res


# ---- command line ---------------------------------------------------------------------------------
def _floats(text):
    try:
        return [float(v) for v in text.split(',') if v.strip() != '']
    except ValueError:
        raise argparse.ArgumentTypeError('a comma-separated list of numbers, got %r' % text)


def main(argv=None):
    from .linemaps import _print_json
    from .video_reader import video_reader
    p = argparse.ArgumentParser(
        prog='python -m solex_ser_recon_en_amd.sharpen',
        usage='%(prog)s INPUT [--levels L] [--gains g1,..] [--denoise k1,..] [--sigma X] [--circle cx,cy,rad] [--region F] [--shift S] '
              '[--contrast] [--limb-protect [MARGIN]] [--limb-blend B] [--limb-reach Q] [--limb-disk-only] [--dejitter] [SHG_MAIN flags]',
        description='Sharpen a disk with B3-spline a-trous wavelet layers: one gain a layer and a soft noise gate on the finest layers.  '
                    'INPUT is a SER or AVI scan, or a 16-bit grey PNG this package wrote (_stack.png, _flat.png, _uncontrasted.png).  '
                    'For a PNG without --circle the noise is measured over the whole image: a black sky biases the estimate low '
                    '(--circle confines it to the disk, --sigma skips the estimate).  The limb\'s edge overshoots into the sky unless '
                    '--limb-protect is given.')
    p.add_argument('--levels', type=int, default=None, help='layers, 1 to 6 (default %d, or as many as --gains names)' % DEFAULT_LEVELS)
    p.add_argument('--gains', type=_floats, default=None,
                   help='gain of every layer, finest first, 0 to 16 (default %s; fewer than --levels: the rest 1)' % ','.join('%g' % g for g in DEFAULT_GAINS))
    p.add_argument('--denoise', type=_floats, default=None,
                   help='gate of every layer in units of its noise (default %s; fewer than --levels: the rest 0)' % ','.join('%g' % k for k in DEFAULT_DENOISE))
    p.add_argument('--sigma', type=float, default=None, help='the noise in counts (default: estimated from the finest layer; skips the estimate)')
    p.add_argument('--circle', type=_floats, default=None, help='cx,cy,rad of the disk in a PNG: the noise is measured inside it')
    p.add_argument('--region', type=float, default=DEFAULT_REGION, help='fraction of the radius the noise is measured within (default %g)' % DEFAULT_REGION)
    p.add_argument('--shift', type=int, default=0, help='pixel shift of a scan\'s disk (the -w shift; default 0: the line centre)')
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the sharpened image (<base>_sharp_clahe.png, ...)')
    limbguard.add_arguments(p, '%g' % DEFAULT_LIMB_MARGIN)
    disk.add_dejitter_argument(p)
    limb = []

    def file_checks(args, files):
        disk.check_dejitter(p, args, files)
        if limb[0] is not None and args.circle is None and any(f.lower().endswith('.png') for f in files):
            p.error('--limb-protect on a PNG needs --circle cx,cy,rad')

    def checks(args):
        levels = args.levels
        if levels is None:
            levels = len(args.gains) if args.gains else DEFAULT_LEVELS
        if not 1 <= levels <= MAX_LEVELS:
            p.error('--levels is 1 to %d' % MAX_LEVELS)
        gains = list(DEFAULT_GAINS[:levels]) if args.gains is None else args.gains
        denoise = list(DEFAULT_DENOISE[:levels]) if args.denoise is None else args.denoise
        if len(gains) > levels or len(denoise) > levels:
            p.error('more --gains or --denoise values than --levels')
        args.gains = gains + [1.0] * (levels - len(gains))
        args.denoise = denoise + [0.0] * (levels - len(denoise))
        if args.circle is not None and len(args.circle) != 3:
            p.error('--circle is cx,cy,rad')
        try:
            quantise_gains(args.gains)
            thresholds(0.0 if args.sigma is None else args.sigma, args.denoise, levels)
            _noise_circle(args.circle, args.region)
        except ValueError as e:
            p.error(str(e))
        limb.append(limbguard.from_arguments(p, args, args.circle, DEFAULT_LIMB_MARGIN))

    args, opts, (path,) = disk.parse(p, argv, 'sharpen', 'sharpening', checks, file_checks, need='exactly one SER, AVI or PNG file is needed',
                                     png=True)
    is_png = path.lower().endswith('.png')
    limb = limb[0]
    try:
        if is_png:
            img, header_source, stem = disk.png_input(path, opts)
            circle = None if args.circle is None else tuple(args.circle)
            sharp, record = sharpen_disk(img, args.gains, args.denoise, args.sigma, circle, args.region, limb)
            res = {'circle': circle if circle is not None else (-1, -1, -1), 'ratio': None, 'phi': None, 'crop': None}
        else:
            if args.circle is not None:
                raise ValueError('--circle goes with a PNG: a scan brings its own limb fit')
            header_source = video_reader(path)
            if limb is not None:
                limb.pop('circle', None)
            res = sharpen_scan(header_source, opts, args.shift, args.gains, args.denoise, args.sigma, args.region, limb,
                               {} if args.dejitter else None)
            sharp, record = res['sharp'], res['record']
            stem = '%s_shift=%d' % (os.path.splitext(path)[0], res['shift'])
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    host, png, fits = disk.write_image(sharp, stem + '_sharp', opts, header_source)
    out = {'input': path, 'shape': list(host.shape), 'levels': record['levels'], 'gains': record['gains'], 'denoise': record['denoise'],
           'sigma': record['sigma'], 'median': None if record['median_q6'] is None else record['median_q6'] / 64.0,
           'pixels': record['pixels'], 'thresholds': record['thresholds'], 'shift': None if is_png else res['shift'], 'png': png,
           'fits': fits, 'contrast': None}
    if limb is not None:
        out['limb'] = record['limb']
    if args.dejitter:
        out['jitter'] = disk.jitter_summary(res['jitter'])
    if args.contrast:
        out['contrast'] = disk.contrast_products(sharp, tuple(res['circle']), opts, header_source, stem + '_sharp')
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
