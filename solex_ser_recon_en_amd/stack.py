"""Stack a series of scans of one line into one disk: every scan's 16-bit disk and fitted circle, one global
similarity transform a scan -- scale from the radii, translation from the centres, refined by an exact search over integer offsets
and a parabola through its minimum --, then all disks resampled into the reference scan's grid and combined pixel by pixel in one
launch.  The resample-and-combine and the sums of squared differences are HIP kernels (ops.stack_combine_u16, ops.shift_ssd_u16);
the arithmetic between them is host float64, written step by step so that tests/stack_ref.py restates it bit for bit.

    python -m solex_ser_recon_en_amd.stack A.ser B.ser ... [--shift S] [--reference K] [--mode mean|median|sigma] [--kappa X]
        [--iterations I] [--search S] [--coverage] [--contrast] [SHG_MAIN flags]
"""
import argparse
import math
import os
import sys

import numpy as np

from . import disk

MAX_SCANS = 32
MAX_SEARCH = 8
MODES = ('mean', 'median', 'sigma')


def scan_disk(file_or_reader, options=None, shift=0):
    """A scan's disk at `shift` and its circle, as flatten_scan computes them before it flattens -> {'image' (a uint16 device
    tensor), 'circle', 'shift', 'ratio', 'phi', 'crop'}.  ValueError for ratio_fixe / slant_fix, de-vignette and a frame shard."""
    return disk.scan_disk(file_or_reader, options, shift, 'stacking')


def disk_level(image, circle):
    """The robust brightness of a disk: flatten.default_level of its filled ring profile."""
    from .flatten import default_level, filled_profile, ring_profile
    return float(default_level(filled_profile(ring_profile(image, circle))))


def parabola_offset(e_minus, e_0, e_plus):
    """The abscissa of the vertex of the parabola through (-1, e_minus), (0, e_0), (1, e_plus), float64:
    0.5 (e_minus - e_plus) / ((e_minus - 2 e_0) + e_plus) when that denominator is > 0, else 0."""
    e_minus, e_0, e_plus = np.float64(e_minus), np.float64(e_0), np.float64(e_plus)
    den = (e_minus - np.float64(2.0) * e_0) + e_plus
    if not den > 0.0:
        return np.float64(0.0)
    return np.float64(0.5) * (e_minus - e_plus) / den


def refine_offset(ssd, search):
    """From shift_ssd_u16's table (host, (2 S + 1)^2 + 1 integers) -> {'u', 'v': the first minimum in row-major order; 'du', 'dv':
    the parabola's correction on each axis (0 on the window's border); 'ssd': the minimum; 'pixels'; 'rejected': the set is empty,
    or S >= 1 and the minimum lies on the window's border}."""
    s = int(search)
    side = 2 * s + 1
    table = np.asarray(ssd).reshape(-1)
    if table.shape[0] != side * side + 1:
        raise ValueError('a table of %d entries for a search of %d' % (table.shape[0], s))
    pixels = int(table[-1])
    e = table[:-1].astype(np.float64).reshape(side, side)
    k = int(np.argmin(table[:-1]))                              # (integers: the first minimum in row-major order)
    iv, iu = divmod(k, side)
    border = s >= 1 and (iu in (0, side - 1) or iv in (0, side - 1))
    du = dv = np.float64(0.0)
    if not border and s >= 1:
        du = parabola_offset(e[iv, iu - 1], e[iv, iu], e[iv, iu + 1])
        dv = parabola_offset(e[iv - 1, iu], e[iv, iu], e[iv + 1, iu])
    return {'u': iu - s, 'v': iv - s, 'du': float(du), 'dv': float(dv), 'ssd': int(table[k]), 'pixels': pixels,
            'rejected': bool(border or pixels == 0)}


def initial_transform(circle, ref_circle):
    """(s, tx, ty): scale from the radii, translation from the centres -- the reference grid's pixel (r, c) lies at
    (tx + s c, ty + s r) in the frame."""
    cx, cy, rad = (np.float64(v) for v in circle)
    cx0, cy0, rad0 = (np.float64(v) for v in ref_circle)
    if not (rad > 0.0 and rad0 > 0.0):
        raise ValueError('a circle without a radius cannot be registered')
    s = rad / rad0
    return s, cx - s * cx0, cy - s * cy0


def refined_transform(s, tx, ty, fit):
    """tx' = tx + s (u + du), ty' = ty + s (v + dv)."""
    s, tx, ty = np.float64(s), np.float64(tx), np.float64(ty)
    return tx + s * (np.float64(fit['u']) + np.float64(fit['du'])), ty + s * (np.float64(fit['v']) + np.float64(fit['dv']))


def register_disks(images, circles, reference=0, search=8, region=0.9):
    """One record a frame: {'s', 'tx', 'ty' (the refined transform into the frame), 'gain' (level of the reference / level of the
    frame), 'level', 'offset' (u + du, v + dv), 'ssd_per_pixel', 'pixels', 'rejected'}.  The frame is resampled alone into the
    reference's grid, compared with the reference over the disk (cx_0, cy_0, region rad_0) at every integer offset within `search`
    pixels, and the first minimum refined by a parabola an axis.  The reference's own record is the identity.  ValueError for a
    level of 0."""
    from . import ops
    from .device import to_device_u16
    images = [to_device_u16(t) for t in images]
    n = len(images)
    if n < 1 or len(circles) != n:
        raise ValueError('%d images and %d circles' % (n, len(circles)))
    if not 0 <= int(reference) < n:
        raise ValueError('reference %r outside the %d frames' % (reference, n))
    if not 0 <= int(search) <= MAX_SEARCH:
        raise ValueError('search must be 0 to %d pixels, got %r' % (MAX_SEARCH, search))
    if not (math.isfinite(region) and region > 0):
        raise ValueError('region must be a positive fraction of the radius')
    reference, search = int(reference), int(search)
    levels = [disk_level(images[i], circles[i]) for i in range(n)]
    for i, level in enumerate(levels):
        if not level > 0:
            raise ValueError('frame %d has a brightness level of %r: nothing to scale' % (i, level))
    ref_circle = tuple(float(v) for v in circles[reference])
    ref_img = images[reference]
    shape = tuple(ref_img.shape)
    disk = (ref_circle[0], ref_circle[1], float(np.float64(region) * np.float64(ref_circle[2])))
    records = []
    for i in range(n):
        if i == reference:
            records.append({'s': 1.0, 'tx': 0.0, 'ty': 0.0, 'gain': 1.0, 'level': levels[i], 'offset': (0.0, 0.0), 'ssd_per_pixel': 0.0,
                            'pixels': None, 'rejected': False})
            continue
        s, tx, ty = initial_transform(circles[i], ref_circle)
        gain = np.float64(levels[reference]) / np.float64(levels[i])
        plane, _ = ops.stack_combine_u16([images[i]], [(s, tx, ty, gain)], shape, 'mean', want_count=False)
        fit = refine_offset(ops.shift_ssd_u16(ref_img, plane, search, disk).cpu().numpy(), search)
        tx2, ty2 = refined_transform(s, tx, ty, fit)
        records.append({'s': float(s), 'tx': float(tx2), 'ty': float(ty2), 'gain': float(gain), 'level': levels[i],
                        'offset': (fit['u'] + fit['du'], fit['v'] + fit['dv']),
                        'ssd_per_pixel': fit['ssd'] / fit['pixels'] if fit['pixels'] else float('nan'), 'pixels': fit['pixels'],
                        'rejected': fit['rejected']})
    return records


def stack_disks(images, transforms, mode='sigma', kappa=2.5, iterations=2, shape=None):
    """The fused call: the images resampled by their transforms -- rows (s, tx, ty, gain) or register_disks' records -- into a grid
    of `shape` (default: the first image's) and combined -> (stack uint16, count uint8) on the device."""
    from . import ops
    from .device import to_device_u16
    images = [to_device_u16(t) for t in images]
    rows = [(t['s'], t['tx'], t['ty'], t['gain']) if isinstance(t, dict) else tuple(t) for t in transforms]
    if len(images) > MAX_SCANS:
        raise ValueError('at most %d frames are stacked at a time, got %d' % (MAX_SCANS, len(images)))
    return ops.stack_combine_u16(images, rows, tuple(images[0].shape) if shape is None else shape, mode, kappa, iterations)


def check_combine(mode, kappa, iterations):
    if mode not in MODES:
        raise ValueError('mode is one of %s, got %r' % (', '.join(MODES), mode))
    if not kappa >= 1:
        raise ValueError('kappa must be >= 1, got %r' % (kappa,))
    if not 1 <= int(iterations) <= 3:
        raise ValueError('iterations must be 1 to 3, got %r' % (iterations,))


def stack_scans(files, options=None, shift=0, reference=0, mode='sigma', kappa=2.5, iterations=2, search=8, region=0.9):
    """The scans' disks at `shift` registered to the one of files[reference] and stacked -> {'stack' uint16, 'count' uint8 (device
    tensors on the reference's grid), 'circle' (the reference's), 'records' (register_disks', one a file), 'used', 'rejected' (indices
    into files), 'images', 'circles', 'shift', 'mode', 'ratio', 'phi', 'crop' (the reference's)}.  ValueError for fewer than 2 or more
    than 32 files, for ratio_fixe / slant_fix, de-vignette and a frame shard, and when fewer than two files survive the
    registration."""
    files = list(files)
    if len(files) < 2:
        raise ValueError('stacking needs at least two scans, got %d' % len(files))
    if len(files) > MAX_SCANS:
        raise ValueError('at most %d scans are stacked at a time, got %d' % (MAX_SCANS, len(files)))
    if not 0 <= int(reference) < len(files):
        raise ValueError('reference %r outside the %d scans' % (reference, len(files)))
    check_combine(mode, kappa, iterations)
    disks = [scan_disk(f, options, shift) for f in files]
    images, circles = [d['image'] for d in disks], [d['circle'] for d in disks]
    records = register_disks(images, circles, reference, search, region)
    used = [i for i, rec in enumerate(records) if not rec['rejected']]
    if len(used) < 2:
        raise ValueError('only %d of %d scans could be registered: nothing to stack' % (len(used), len(files)))
    ref = disks[int(reference)]
    stack, count = stack_disks([images[i] for i in used], [records[i] for i in used], mode, kappa, iterations, tuple(ref['image'].shape))
    return {'stack': stack, 'count': count, 'circle': ref['circle'], 'records': records, 'used': used,
            'rejected': [i for i in range(len(files)) if i not in used], 'images': images, 'circles': circles, 'shift': ref['shift'],
            'mode': mode, 'kappa': float(kappa), 'iterations': int(iterations), 'reference': int(reference), 'ratio': ref['ratio'],
            'phi': ref['phi'], 'crop': ref['crop']}


# ---- command line ---------------------------------------------------------------------------------
def main(argv=None):
    from .linemaps import _print_json
    from .png_io import write_png
    from .solex_util import output_path
    from .video_reader import video_reader
    p = argparse.ArgumentParser(prog='python -m solex_ser_recon_en_amd.stack',
                                usage='%(prog)s FILE FILE ... [--shift S] [--reference K] [--mode mean|median|sigma] [--kappa X] '
                                      '[--iterations I] [--search S] [--coverage] [--contrast] [SHG_MAIN flags]',
                                description='Stack a series of scans of one line: register every scan\'s disk to the reference scan\'s '
                                            'and combine them into one image.')
    p.add_argument('--shift', type=int, default=0, help='pixel shift of the disks to stack (the -w shift; default 0: the line centre)')
    p.add_argument('--reference', type=int, default=0, help='index of the scan whose grid the stack is made on (default 0: the first)')
    p.add_argument('--mode', choices=MODES, default='sigma', help='how the frames are combined (default sigma: the clipped mean)')
    p.add_argument('--kappa', type=float, default=2.5, help='sigma mode: reject beyond kappa standard deviations (>= 1; default 2.5, which clips nothing below nine '
                                                                 'scans: none of n samples lies further than (n - 1) / sqrt(n) from their mean)')
    p.add_argument('--iterations', type=int, default=2, help='sigma mode: clipping passes (1 to 3; default 2)')
    p.add_argument('--search', type=int, default=8, help='half-width of the offset search in pixels (0 to 8; default 8)')
    p.add_argument('--coverage', action='store_true', help='also the number of frames behind every pixel (<base>_stack_count.png)')
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the stack (<base>_stack_clahe.png, ...)')

    def checks(args):
        if not args.kappa >= 1:
            p.error('--kappa must be >= 1')
        if not 1 <= args.iterations <= 3:
            p.error('--iterations must be 1 to 3')
        if not 0 <= args.search <= MAX_SEARCH:
            p.error('--search must be 0 to %d' % MAX_SEARCH)

    def file_checks(args, files):
        if len(files) > MAX_SCANS:
            p.error('at most %d scans are stacked at a time (got %d)' % (MAX_SCANS, len(files)))
        if not 0 <= args.reference < len(files):
            p.error('--reference must be 0 to %d' % (len(files) - 1))

    args, opts, files = disk.parse(p, argv, 'stack', 'stacking', checks, file_checks, least=2, most=None,
                                   need='at least two SER or AVI files are needed')
    try:
        res = stack_scans(files, opts, args.shift, args.reference, args.mode, args.kappa, args.iterations, args.search)
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    ref_path = files[args.reference]
    rdr = video_reader(ref_path)                                    # (for the headers: the scans themselves were read above)
    stem = '%s_shift=%d_stack' % (os.path.splitext(ref_path)[0], res['shift'])
    stack, png, fits = disk.write_image(res['stack'], stem, opts, rdr)
    out = {'shape': list(stack.shape), 'mode': res['mode'], 'kappa': res['kappa'], 'iterations': res['iterations'], 'shift': res['shift'],
           'reference': res['reference'], 'files': [files[i] for i in res['used']], 'rejected': [files[i] for i in res['rejected']],
           'frames': [{'file': files[i], 'scale': rec['s'], 'offset': list(rec['offset']), 'gain': rec['gain'],
                       'rms': None if rec['rejected'] and not rec['pixels'] else math.sqrt(rec['ssd_per_pixel']),
                       'rejected': rec['rejected']} for i, rec in enumerate(res['records'])],
           'png': png, 'fits': fits, 'count_png': None}
    if args.coverage:
        out['count_png'] = output_path(stem + '_count.png', opts)
        write_png(out['count_png'], np.ascontiguousarray(np.rot90(res['count'].contiguous().cpu().numpy(), opts['img_rotate'] // 90)), 0)
    if args.contrast:
        out['contrast'] = disk.contrast_products(res['stack'], res['circle'], opts, rdr, stem)
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
