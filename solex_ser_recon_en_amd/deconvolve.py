"""Deconvolve a disk: Richardson-Lucy iterations of a 16-bit image with a separable point-spread function --
the step between a stack and its wavelets, which inverts the instrument-and-seeing blur where the wavelet gains only weigh scales.
The iterations are HIP kernels in float32 whose arithmetic include/shg_hip.h states exactly (ops.rl_deconvolve_u16); the Gaussian
taps are host float64, written step by step so that the tests restate them.

    python -m solex_ser_recon_en_amd.deconvolve INPUT [--psf-sigma X | SX,SY | auto] [--iterations N] [--radius R] [--shift S] [--contrast]
        [--circle cx,cy,rad] [--limb-protect [MARGIN]] [--limb-blend B] [--limb-reach Q] [--limb-disk-only] [SHG_MAIN flags]

Richardson-Lucy amplifies noise: it suits a stack, and a single scan only for a few iterations.  The limb is a step, and the
iterations ring on it: --limb-protect (limb=) runs them on a disk plane and a sky plane that have no step and leaves the band of
the limb as it is (limbguard.py).  The blur need not be guessed nor round: --psf-sigma auto measures a width an
axis from the limb (psf.py), and SX,SY gives the two.  Out of scope: point-spread functions that are not
separable, damping against ringing, regularised or blind variants, stopping rules, and any change to the stack or
flatten command lines.
"""
import argparse
import math
import os
import sys

import numpy as np

from . import disk, limbguard

MAX_RADIUS = 16
MAX_ITERATIONS = 200
MIN_SIGMA, MAX_SIGMA = 0.3, 4.0
MIN_TAP = 2.0 ** -30
DEFAULT_SIGMA = 1.2
DEFAULT_ITERATIONS = 10


def gaussian_taps(sigma, radius=None):
    """The 2 R + 1 taps of a Gaussian of `sigma` pixels (0.3 to 4): exp(-i^2 / (2 sigma^2)) over i = -R .. R in float64, normalised to
    sum 1, cast to float32; a tap that comes out below 2^-30, the smallest non-zero tap the kernel takes, is 0 (on a full-scale pixel
    it is worth 2^-14 of a count).  radius None: ceil(4 sigma); else an integer from 0 to 16.  ValueError outside the ranges."""
    if not (isinstance(sigma, (int, float, np.integer, np.floating)) and math.isfinite(sigma) and MIN_SIGMA <= sigma <= MAX_SIGMA):
        raise ValueError('sigma lies in [%g, %g], got %r' % (MIN_SIGMA, MAX_SIGMA, sigma))
    if radius is None:
        radius = int(math.ceil(4.0 * float(sigma)))
    if not (isinstance(radius, (int, np.integer)) and 0 <= radius <= MAX_RADIUS):
        raise ValueError('radius is an integer from 0 to %d, got %r' % (MAX_RADIUS, radius))
    i = np.arange(-int(radius), int(radius) + 1, dtype=np.float64)
    k = np.exp(-(i * i) / (2.0 * float(sigma) * float(sigma)))
    k = (k / k.sum()).astype(np.float32)
    k[k < np.float32(MIN_TAP)] = 0.0
    return k


def _check_iterations(iterations):
    if not (isinstance(iterations, (int, np.integer)) and 1 <= iterations <= MAX_ITERATIONS):
        raise ValueError('iterations is an integer from 1 to %d, got %r' % (MAX_ITERATIONS, iterations))
    return int(iterations)


def _is_pair(v):
    return isinstance(v, (tuple, list)) and len(v) == 2


def _deconvolve_disk_xy(image, sigma, iterations, taps, radius, limb):
    """deconvolve_disk with a pair: sigma (sx, sy) or taps (along x, along y)."""
    from . import ops
    from .device import to_device_u16
    if taps is None:
        sigma = tuple(float(v) for v in sigma)
        kx, ky = gaussian_taps(sigma[0], radius), gaussian_taps(sigma[1], radius)
    else:
        if sigma is not None or radius is not None:
            raise ValueError('taps come without sigma and radius')
        kx, ky = (np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in taps)
    if kx.tobytes() == ky.tobytes():                                  # not a bit apart: the one-set call
        out, record = deconvolve_disk(image, None, iterations, kx, None, limb)
        if sigma is not None:
            record['sigma'] = list(sigma)
        return out, record
    run = lambda plane: ops.rl_deconvolve_xy_u16(plane, kx, ky, iterations)[0]
    record = {'sigma': None if sigma is None else list(sigma), 'radius': [int(kx.size // 2), int(ky.size // 2)],
              'taps': [[float(v) for v in kx], [float(v) for v in ky]], 'iterations': iterations}
    if limb is None:
        return run(to_device_u16(image)), record
    circle, margin, blend, reach, sky = limbguard.settings(limb, float(max(kx.size, ky.size) // 2))
    out, record['limb'] = limbguard.protect(image, circle, run, margin, blend, reach, sky)
    return out, record


def deconvolve_disk(image, sigma=None, iterations=DEFAULT_ITERATIONS, taps=None, radius=None, limb=None):
    """The uint16 device image after `iterations` Richardson-Lucy iterations with the separable blur of `taps` (2 R + 1 float32
    values, as ops.rl_deconvolve_u16 takes them), or, without taps, of gaussian_taps(sigma, radius) (sigma None: 1.2) -> (the
    deconvolved uint16 device image, the record {'sigma' (None with given taps), 'radius', 'taps', 'iterations'}).  limb: a dict
    {'circle': (cx, cy, rad), 'margin' (default: the taps' radius), 'blend', 'reach', 'sky'} runs the iterations under
    limbguard.protect -- on the disk plane and, unless sky is False, on the sky plane --, and the record gains 'limb', protect's.
    sigma may be a pair (sx, sy) and taps a pair of arrays (along a row, down a column): a blur an axis, as psf.estimate_psf
    measures it (radius applies to both; default ceil(4 sigma) an axis; the limb's default margin is the larger radius).  Two sets
    that differ in any bit go through ops.rl_deconvolve_xy_u16, and the record's 'radius' and 'taps' are then pairs as well."""
    from . import ops
    from .device import to_device_u16
    iterations = _check_iterations(iterations)
    if _is_pair(sigma) or (taps is not None and _is_pair(taps) and np.ndim(taps[0]) == 1):
        return _deconvolve_disk_xy(image, sigma, iterations, taps, radius, limb)
    if taps is None:
        sigma = DEFAULT_SIGMA if sigma is None else float(sigma)
        k = gaussian_taps(sigma, radius)
    else:
        if sigma is not None or radius is not None:
            raise ValueError('taps come without sigma and radius')
        k = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    record = {'sigma': sigma, 'radius': int(k.size // 2), 'taps': [float(v) for v in k], 'iterations': iterations}
    if limb is None:
        out, _ = ops.rl_deconvolve_u16(to_device_u16(image), k, iterations)
        return out, record
    circle, margin, blend, reach, sky = limbguard.settings(limb, float(k.size // 2))
    out, record['limb'] = limbguard.protect(image, circle, lambda plane: ops.rl_deconvolve_u16(plane, k, iterations)[0], margin, blend,
                                            reach, sky)
    return out, record


def _sigma_of(sigma, image, circle):
    """sigma as deconvolve_disk takes it, and what was measured: 'auto' -> ((sx, sy) clipped to the range of gaussian_taps,
    psf.estimate_psf's answer without its per-sector list); anything else -> (sigma, None)."""
    if not (isinstance(sigma, str) and sigma == 'auto'):
        return sigma, None
    from . import psf
    if circle is None:
        raise ValueError('sigma \'auto\' needs the disk\'s circle (cx, cy, rad)')
    est = psf.estimate_psf(image, circle)
    measured = {k: est[k] for k in ('sigma_x', 'sigma_y', 'isotropic', 'n_used', 'rms')}
    return tuple(min(max(est[k], MIN_SIGMA), MAX_SIGMA) for k in ('sigma_x', 'sigma_y')), measured


def deconvolve_scan(file_or_reader, options=None, shift=0, sigma=None, iterations=DEFAULT_ITERATIONS, taps=None, radius=None, limb=None,
                    dejitter=None):
    """A scan's disk at `shift` (disk.scan_disk, with its refusals: ratio_fixe / slant_fix, de-vignette, a frame shard),
    deconvolved by deconvolve_disk -> {'image', 'deconv' (uint16 device tensors), 'circle', 'record', 'shift', 'ratio', 'phi',
    'crop'}.  limb: deconvolve_disk's dict without 'circle': the scan's own limb fit is the circle.  sigma 'auto': the widths
    psf.estimate_psf measures on the scan's own limb, and the record gains 'psf', what it measured.  dejitter: disk.scan_disk's; the
    result then holds 'jitter'."""
    scan = disk.scan_disk(file_or_reader, options, shift, 'deconvolution', dejitter)
    sigma, measured = _sigma_of(sigma, scan['image'], scan['circle'])
    if limb is not None:
        if not isinstance(limb, dict) or limb.get('circle') is not None:
            raise ValueError('a scan brings its own limb fit: limb is a dict without a circle')
        limb = dict(limb, circle=scan['circle'])
    deconv, record = deconvolve_disk(scan['image'], sigma, iterations, taps, radius, limb)
    if measured is not None:
        record['psf'] = measured
    res = {'image': scan['image'], 'deconv': deconv, 'circle': scan['circle'], 'record': record, 'shift': scan['shift'],
           'ratio': scan['ratio'], 'phi': scan['phi'], 'crop': scan['crop']}
    if 'jitter' in scan:
        res['jitter'] = scan['jitter']
    return res


# ---- command line ---------------------------------------------------------------------------------
def psf_sigma_argument(text):
    """--psf-sigma: a float, as ever; 'auto' -> the string; 'SX,SY' -> a pair of floats."""
    if text.strip().lower() == 'auto':
        return 'auto'
    try:
        values = [float(v) for v in text.split(',')]
    except ValueError:
        values = []
    if len(values) not in (1, 2):
        raise argparse.ArgumentTypeError('invalid float value: %r' % text)
    return values[0] if len(values) == 1 else tuple(values)


def _floats(text):
    try:
        return [float(v) for v in text.split(',') if v.strip() != '']
    except ValueError:
        raise argparse.ArgumentTypeError('a comma-separated list of numbers, got %r' % text)


def main(argv=None):
    from .linemaps import _print_json
    from .video_reader import video_reader
    p = argparse.ArgumentParser(
        prog='python -m solex_ser_recon_en_amd.deconvolve',
        usage='%(prog)s INPUT [--psf-sigma X | SX,SY | auto] [--iterations N] [--radius R] [--shift S] [--contrast] [--circle cx,cy,rad] '
              '[--limb-protect [MARGIN]] [--limb-blend B] [--limb-reach Q] [--limb-disk-only] [--dejitter] [SHG_MAIN flags]',
        description='Deconvolve a disk: Richardson-Lucy iterations with a Gaussian point-spread function.  INPUT is a SER or AVI scan, or '
                    'a 16-bit grey PNG this package wrote (_stack.png, _flat.png, _uncontrasted.png).  The iterations amplify noise: '
                    'give a stack many, a single scan few.  The limb rings unless --limb-protect is given.')
    p.add_argument('--psf-sigma', type=psf_sigma_argument, default=DEFAULT_SIGMA,
                   help='the blur\'s Gaussian sigma in pixels, %g to %g (default %g); SX,SY: one along the rows and one down the columns; '
                        'auto: measured from the limb (a PNG needs --circle)' % (MIN_SIGMA, MAX_SIGMA, DEFAULT_SIGMA))
    p.add_argument('--iterations', type=int, default=DEFAULT_ITERATIONS, help='1 to %d (default %d)' % (MAX_ITERATIONS, DEFAULT_ITERATIONS))
    p.add_argument('--radius', type=int, default=None, help='the taps reach this far, 0 to %d (default: ceil(4 sigma))' % MAX_RADIUS)
    p.add_argument('--shift', type=int, default=0, help='pixel shift of a scan\'s disk (the -w shift; default 0: the line centre)')
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the deconvolved image (<base>_deconv_clahe.png, ...)')
    p.add_argument('--circle', type=_floats, default=None, help='cx,cy,rad of the disk in a PNG: what --limb-protect and --contrast go by')
    limbguard.add_arguments(p, 'the radius of the taps')
    disk.add_dejitter_argument(p)
    limb = []

    def checks(args):
        try:
            # (auto: the widths are not known yet; the margin's default is checked on the widest taps there are)
            sigmas = (MAX_SIGMA,) if args.psf_sigma == 'auto' else args.psf_sigma if _is_pair(args.psf_sigma) else (args.psf_sigma,)
            reach = max(gaussian_taps(s, args.radius).size // 2 for s in sigmas)
            _check_iterations(args.iterations)
        except ValueError as e:
            p.error(str(e))
        if args.circle is not None and len(args.circle) != 3:
            p.error('--circle is cx,cy,rad')
        limb.append(limbguard.from_arguments(p, args, args.circle, float(reach)))

    def file_checks(args, files):
        disk.check_dejitter(p, args, files)
        if limb[0] is not None and args.circle is None and any(f.lower().endswith('.png') for f in files):
            p.error('--limb-protect on a PNG needs --circle cx,cy,rad')
        if args.psf_sigma == 'auto' and args.circle is None and any(f.lower().endswith('.png') for f in files):
            p.error('--psf-sigma auto on a PNG needs --circle cx,cy,rad')

    args, opts, (path,) = disk.parse(p, argv, 'deconvolve', 'deconvolution', checks, file_checks,
                                     need='exactly one SER, AVI or PNG file is needed', png=True)
    is_png = path.lower().endswith('.png')
    limb = limb[0]
    measured = None
    try:
        if is_png:
            img, header_source, stem = disk.png_input(path, opts)
            sigma, measured = _sigma_of(args.psf_sigma, img, args.circle)
            deconv, record = deconvolve_disk(img, sigma, args.iterations, radius=args.radius, limb=limb)
            res = {'circle': (-1, -1, -1) if args.circle is None else tuple(args.circle), 'ratio': None, 'phi': None, 'crop': None}
            total = float(img.astype(np.float64).sum())
        else:
            if args.circle is not None:
                raise ValueError('--circle goes with a PNG: a scan brings its own limb fit')
            header_source = video_reader(path)
            res = deconvolve_scan(header_source, opts, args.shift, args.psf_sigma, args.iterations, radius=args.radius, limb=limb,
                                  dejitter={} if args.dejitter else None)
            measured = res['record'].pop('psf', None)
            deconv, record = res['deconv'], res['record']
            stem = '%s_shift=%d' % (os.path.splitext(path)[0], res['shift'])
            total = float(disk.host_u(res['image'].contiguous(), np.uint16).astype(np.float64).sum())
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    host, png, fits = disk.write_image(deconv, stem + '_deconv', opts, header_source)
    out = {'input': path, 'shape': list(host.shape), 'psf_sigma': record['sigma'], 'radius': record['radius'], 'taps': record['taps'],
           'iterations': record['iterations'], 'flux': float(host.astype(np.float64).sum()) / total if total else None,
           'shift': None if is_png else res['shift'], 'png': png, 'fits': fits, 'contrast': None}
    if limb is not None:
        out['limb'] = record['limb']
    if measured is not None:
        out['psf'] = measured
    if args.dejitter:
        out['jitter'] = disk.jitter_summary(res['jitter'])
    if args.contrast:
        out['contrast'] = disk.contrast_products(deconv, tuple(res['circle']), opts, header_source, stem + '_deconv')
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
