"""Stack a series of scans of one line into one disk: every scan's 16-bit disk and fitted circle, one global
similarity transform a scan -- scale from the radii, translation from the centres, refined by an exact search over integer offsets
and a parabola through its minimum --, then all disks resampled into the reference scan's grid and combined pixel by pixel in one
launch.  The resample-and-combine and the sums of squared differences are HIP kernels (ops.stack_combine_u16, ops.shift_ssd_u16);
the arithmetic between them is host float64, written step by step so that tests/stack_ref.py restates it bit for bit.  With
--local every scan is also bent by a field of local alignment points: one offset search a lattice node
(ops.patch_ssd_u16), refined and filled on the host, and the combine that reads each scan through its field
(ops.stack_combine_field_u16); tests/align_ref.py restates those.

    python -m solex_ser_recon_en_amd.stack A.ser B.ser ... [--shift S] [--reference K] [--mode mean|median|sigma] [--kappa X]
        [--iterations I] [--search S] [--local [--ap-size P] [--ap-step D] [--ap-search S] [--ap-min-contrast X]] [--coverage]
        [--contrast] [SHG_MAIN flags]
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


# ---- local alignment points ----
LOCAL_DEFAULTS = {'step': 16, 'size': 33, 'search': 4, 'region': 0.9, 'min_contrast': 0.0}


def check_local(step, size, search, min_contrast=0.0):
    if not 8 <= int(step) <= 128:
        raise ValueError('the alignment points\' step must be 8 to 128 pixels, got %r' % (step,))
    if not (3 <= int(size) <= 65 and int(size) % 2 == 1):
        raise ValueError('the alignment patches\' size must be odd and 3 to 65 pixels, got %r' % (size,))
    if not 0 <= int(search) <= MAX_SEARCH:
        raise ValueError('the alignment points\' search must be 0 to %d pixels, got %r' % (MAX_SEARCH, search))
    if not min_contrast >= 0:
        raise ValueError('min_contrast must be >= 0, got %r' % (min_contrast,))


def align_lattice(shape, step):
    """The lattice of alignment points over a grid of `shape`: nodes at (j step, i step), as many as cover the grid -> (gh, gw,
    points int32 [gh gw, 2] of (row, col) in row-major order): gh = (oh - 1 + step - 1) // step + 1, gw alike.  (The last row or
    column of nodes may lie beyond the grid.)"""
    oh, ow, step = int(shape[0]), int(shape[1]), int(step)
    if oh < 1 or ow < 1 or step < 1:
        raise ValueError('a lattice needs a grid and a step of at least one pixel')
    gh, gw = (oh - 1 + step - 1) // step + 1, (ow - 1 + step - 1) // step + 1
    points = np.empty((gh, gw, 2), dtype=np.int32)
    points[:, :, 0] = (np.arange(gh, dtype=np.int32) * step)[:, None]
    points[:, :, 1] = (np.arange(gw, dtype=np.int32) * step)[None, :]
    return gh, gw, points.reshape(-1, 2)


def fill_field(field, measured):
    """The unmeasured nodes of a field (float64 [gh, gw, 2]; measured bool [gh, gw]) filled in passes: in each pass every unfilled
    node with at least one filled 8-neighbour takes the mean of those neighbours -- summed in row-major neighbour order, float64,
    from the state before the pass --, until nothing changes.  With no measured node the field is all zero.  -> a new array.
    (Whole-array passes over the eight shifted copies of the state: an unfilled neighbour adds +0.0 to a sum that began as +0.0,
    which changes no bit.)"""
    filled = np.array(measured, dtype=bool)
    field = np.where(filled[:, :, None], np.asarray(field, dtype=np.float64), 0.0)
    gh, gw = filled.shape
    if not filled.any():
        return field
    while not filled.all():
        had = np.zeros((gh + 2, gw + 2), dtype=bool)
        had[1:-1, 1:-1] = filled
        before = np.zeros((gh + 2, gw + 2, 2), dtype=np.float64)
        before[1:-1, 1:-1] = field
        total = np.zeros((gh, gw, 2), dtype=np.float64)
        count = np.zeros((gh, gw), dtype=np.int64)
        for dj in (0, 1, 2):
            for di in (0, 1, 2):
                if (dj, di) != (1, 1):
                    have = had[dj:dj + gh, di:di + gw]
                    total = total + np.where(have[:, :, None], before[dj:dj + gh, di:di + gw], 0.0)
                    count = count + have
        new = ~filled & (count > 0)
        field = np.where(new[:, :, None], total / np.maximum(count, 1).astype(np.float64)[:, :, None], field)
        filled = filled | new
    return field


def measure_field(table, gh, gw, half, search, min_contrast=0.0):
    """From patch_ssd_u16's tables of one frame (host, [gh gw, (2 S + 1)^2 + 3] integers) -> (field float64 [gh, gw, 2] of (dx, dy),
    the unmeasured nodes still 0; measured bool [gh, gw]).  refine_offset on a node's sums and pixel count; the node is measured
    unless its set holds fewer than half of (2 B + 1)^2 pixels, its minimum lies on the window's border, or -- with min_contrast > 0
    -- its contrast sqrt(sum ref^2 / n - (sum ref / n)^2) / (sum ref / n) is below min_contrast."""
    side = 2 * int(search) + 1
    n_off = side * side
    table = np.asarray(table).reshape(gh * gw, n_off + 3)
    full = (2 * int(half) + 1) ** 2
    field = np.zeros((gh, gw, 2), dtype=np.float64)
    measured = np.zeros((gh, gw), dtype=bool)
    for p in range(gh * gw):
        pixels = int(table[p, n_off])
        if 2 * pixels < full:
            continue
        fit = refine_offset(table[p, :n_off + 1], search)
        if fit['rejected']:
            continue
        if min_contrast > 0:
            n = np.float64(pixels)
            mean = np.float64(int(table[p, n_off + 1])) / n
            var = np.float64(int(table[p, n_off + 2])) / n - mean * mean
            with np.errstate(invalid='ignore', divide='ignore'):
                contrast = np.sqrt(var) / mean
            if contrast < np.float64(min_contrast):
                continue
        j, i = divmod(p, gw)
        field[j, i, 0] = np.float64(fit['u']) + np.float64(fit['du'])
        field[j, i, 1] = np.float64(fit['v']) + np.float64(fit['dv'])
        measured[j, i] = True
    return field, measured


def field_stats(field, measured):
    """{'points', 'used', 'rms', 'max'} of the measured displacements: the nodes, the measured ones, sqrt(sum (dx^2 + dy^2) / used)
    summed in node order, and the longest (0 and 0 when none is measured)."""
    d2 = [field[j, i, 0] * field[j, i, 0] + field[j, i, 1] * field[j, i, 1] for j, i in zip(*np.nonzero(measured))]
    total = np.float64(0.0)
    for t in d2:
        total = total + t
    used = len(d2)
    return {'points': int(measured.size), 'used': used, 'rms': float(np.sqrt(total / np.float64(used))) if used else 0.0,
            'max': float(np.sqrt(max(d2))) if used else 0.0}


def local_fields(images, records, circles, reference=0, step=16, size=33, search=4, region=0.9, min_contrast=0.0):
    """One displacement field a frame on the lattice align_lattice(reference's shape, step) -> (fields: float64 [gh, gw, 2] device
    tensors of (dx, dy), None for the reference and for a rejected frame; stats: field_stats' dicts, None where the field is).
    The frame is resampled alone into the reference's grid by its refined transform (records: register_disks'), one patch of
    size x size around every node compared with the reference over the disk (cx_0, cy_0, region rad_0) at every integer offset
    within `search` pixels (ops.patch_ssd_u16), each node refined as the global offset is (measure_field) and the unmeasured nodes
    filled from their neighbours (fill_field).  The output pixel (r, c) then reads the frame at (tx + s (c + dx), ty + s (r + dy))."""
    import torch
    from . import ops
    from .device import to_device_u16
    images = [to_device_u16(t) for t in images]
    n = len(images)
    if n < 1 or len(circles) != n or len(records) != n:
        raise ValueError('%d images, %d records and %d circles' % (n, len(records), len(circles)))
    if not 0 <= int(reference) < n:
        raise ValueError('reference %r outside the %d frames' % (reference, n))
    check_local(step, size, search, min_contrast)
    if not (math.isfinite(region) and region > 0):
        raise ValueError('region must be a positive fraction of the radius')
    reference, step, search, half = int(reference), int(step), int(search), (int(size) - 1) // 2
    ref_circle = tuple(float(v) for v in circles[reference])
    ref_img = images[reference]
    shape = tuple(ref_img.shape)
    disk = (ref_circle[0], ref_circle[1], float(np.float64(region) * np.float64(ref_circle[2])))
    gh, gw, points = align_lattice(shape, step)
    points_dev = torch.from_numpy(points).to(ref_img.device)
    fields, stats = [], []
    for i in range(n):
        rec = records[i]
        if i == reference or rec['rejected']:
            fields.append(None), stats.append(None)
            continue
        plane, _ = ops.stack_combine_u16([images[i]], [(rec['s'], rec['tx'], rec['ty'], rec['gain'])], shape, 'mean', want_count=False)
        table = ops.patch_ssd_u16(ref_img, plane, points_dev, half, search, disk).cpu().numpy()
        raw, measured = measure_field(table, gh, gw, half, search, min_contrast)
        fields.append(torch.from_numpy(fill_field(raw, measured)).to(ref_img.device))
        stats.append(field_stats(raw, measured))
    return fields, stats


def stack_disks(images, transforms, mode='sigma', kappa=2.5, iterations=2, shape=None, fields=None, step=None):
    """The fused call: the images resampled by their transforms -- rows (s, tx, ty, gain) or register_disks' records -- into a grid
    of `shape` (default: the first image's) and combined -> (stack uint16, count uint8) on the device.  fields (local_fields', one
    an image, None for none) and their lattice's step: each image is bent by its field as well."""
    from . import ops
    from .device import to_device_u16
    images = [to_device_u16(t) for t in images]
    rows = [(t['s'], t['tx'], t['ty'], t['gain']) if isinstance(t, dict) else tuple(t) for t in transforms]
    if len(images) > MAX_SCANS:
        raise ValueError('at most %d frames are stacked at a time, got %d' % (MAX_SCANS, len(images)))
    if fields is not None and step is None:
        raise ValueError('fields need their lattice\'s step')
    shape = tuple(images[0].shape) if shape is None else shape
    if fields is None:
        return ops.stack_combine_u16(images, rows, shape, mode, kappa, iterations)
    return ops.stack_combine_field_u16(images, rows, fields, step, shape, mode, kappa, iterations)


def check_combine(mode, kappa, iterations):
    if mode not in MODES:
        raise ValueError('mode is one of %s, got %r' % (', '.join(MODES), mode))
    if not kappa >= 1:
        raise ValueError('kappa must be >= 1, got %r' % (kappa,))
    if not 1 <= int(iterations) <= 3:
        raise ValueError('iterations must be 1 to 3, got %r' % (iterations,))


def stack_scans(files, options=None, shift=0, reference=0, mode='sigma', kappa=2.5, iterations=2, search=8, region=0.9, local=None):
    """The scans' disks at `shift` registered to the one of files[reference] and stacked -> {'stack' uint16, 'count' uint8 (device
    tensors on the reference's grid), 'circle' (the reference's), 'records' (register_disks', one a file), 'used', 'rejected' (indices
    into files), 'images', 'circles', 'shift', 'mode', 'ratio', 'phi', 'crop' (the reference's), 'local'}.  local: None, or a dict of
    local_fields' parameters ('step', 'size', 'search', 'region', 'min_contrast'; LOCAL_DEFAULTS for those left out): every used
    frame is also bent by its field of alignment points, and 'local' is {'step', 'size', 'search', 'region', 'min_contrast',
    'fields', 'frames' (local_fields' two lists, one entry a file)} instead of None.  ValueError for fewer than 2 or more than 32
    files, for ratio_fixe / slant_fix, de-vignette and a frame shard, and when fewer than two files survive the registration."""
    files = list(files)
    if len(files) < 2:
        raise ValueError('stacking needs at least two scans, got %d' % len(files))
    if len(files) > MAX_SCANS:
        raise ValueError('at most %d scans are stacked at a time, got %d' % (MAX_SCANS, len(files)))
    if not 0 <= int(reference) < len(files):
        raise ValueError('reference %r outside the %d scans' % (reference, len(files)))
    check_combine(mode, kappa, iterations)
    if local is not None:
        unknown = sorted(set(local) - set(LOCAL_DEFAULTS))
        if unknown:
            raise ValueError('local knows %s, got %s' % (', '.join(LOCAL_DEFAULTS), ', '.join(unknown)))
        local = dict(LOCAL_DEFAULTS, **local)
        check_local(local['step'], local['size'], local['search'], local['min_contrast'])
    disks = [scan_disk(f, options, shift) for f in files]
    images, circles = [d['image'] for d in disks], [d['circle'] for d in disks]
    records = register_disks(images, circles, reference, search, region)
    used = [i for i, rec in enumerate(records) if not rec['rejected']]
    if len(used) < 2:
        raise ValueError('only %d of %d scans could be registered: nothing to stack' % (len(used), len(files)))
    ref = disks[int(reference)]
    fields = None
    if local is not None:
        fields, frames = local_fields(images, records, circles, reference, **local)
        local = dict(local, fields=fields, frames=frames)
        fields = [fields[i] for i in used]
    stack, count = stack_disks([images[i] for i in used], [records[i] for i in used], mode, kappa, iterations, tuple(ref['image'].shape),
                               fields, None if local is None else local['step'])
    return {'local': local, 'stack': stack, 'count': count, 'circle': ref['circle'], 'records': records, 'used': used,
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
                                      '[--iterations I] [--search S] [--local [--ap-size P] [--ap-step D] [--ap-search S] '
                                      '[--ap-min-contrast X]] [--coverage] [--contrast] [SHG_MAIN flags]',
                                description='Stack a series of scans of one line: register every scan\'s disk to the reference scan\'s '
                                            'and combine them into one image.')
    p.add_argument('--shift', type=int, default=0, help='pixel shift of the disks to stack (the -w shift; default 0: the line centre)')
    p.add_argument('--reference', type=int, default=0, help='index of the scan whose grid the stack is made on (default 0: the first)')
    p.add_argument('--mode', choices=MODES, default='sigma', help='how the frames are combined (default sigma: the clipped mean)')
    p.add_argument('--kappa', type=float, default=2.5, help='sigma mode: reject beyond kappa standard deviations (>= 1; default 2.5, which clips nothing below nine '
                                                                 'scans: none of n samples lies further than (n - 1) / sqrt(n) from their mean)')
    p.add_argument('--iterations', type=int, default=2, help='sigma mode: clipping passes (1 to 3; default 2)')
    p.add_argument('--search', type=int, default=8, help='half-width of the offset search in pixels (0 to 8; default 8)')
    p.add_argument('--local', action='store_true', help='after the global registration, bend every scan by a field of local alignment points')
    p.add_argument('--ap-size', type=int, default=None, help='--local: side of an alignment patch in pixels (odd, 3 to 65; default 33)')
    p.add_argument('--ap-step', type=int, default=None, help='--local: distance of the alignment points in pixels (8 to 128; default 16)')
    p.add_argument('--ap-search', type=int, default=None, help='--local: half-width of a point\'s offset search in pixels (1 to 8; default 4)')
    p.add_argument('--ap-min-contrast', type=float, default=None, help='--local: leave out the points whose patch of the reference has a standard '
                                                                         'deviation below this fraction of its mean (default 0: none)')
    p.add_argument('--coverage', action='store_true', help='also the number of frames behind every pixel (<base>_stack_count.png)')
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the stack (<base>_stack_clahe.png, ...)')

    def checks(args):
        if not args.kappa >= 1:
            p.error('--kappa must be >= 1')
        if not 1 <= args.iterations <= 3:
            p.error('--iterations must be 1 to 3')
        if not 0 <= args.search <= MAX_SEARCH:
            p.error('--search must be 0 to %d' % MAX_SEARCH)
        given = [flag for flag, value in (('--ap-size', args.ap_size), ('--ap-step', args.ap_step), ('--ap-search', args.ap_search),
                                          ('--ap-min-contrast', args.ap_min_contrast)) if value is not None]
        if given and not args.local:
            p.error('%s needs --local' % given[0])
        if args.ap_size is not None and not (3 <= args.ap_size <= 65 and args.ap_size % 2 == 1):
            p.error('--ap-size must be odd and 3 to 65')
        if args.ap_step is not None and not 8 <= args.ap_step <= 128:
            p.error('--ap-step must be 8 to 128')
        if args.ap_search is not None and not 1 <= args.ap_search <= MAX_SEARCH:
            p.error('--ap-search must be 1 to %d' % MAX_SEARCH)
        if args.ap_min_contrast is not None and not args.ap_min_contrast >= 0:
            p.error('--ap-min-contrast must be >= 0')

    def file_checks(args, files):
        if len(files) > MAX_SCANS:
            p.error('at most %d scans are stacked at a time (got %d)' % (MAX_SCANS, len(files)))
        if not 0 <= args.reference < len(files):
            p.error('--reference must be 0 to %d' % (len(files) - 1))

    args, opts, files = disk.parse(p, argv, 'stack', 'stacking', checks, file_checks, least=2, most=None,
                                   need='at least two SER or AVI files are needed')
    local = None
    if args.local:
        local = {key: value for key, value in (('size', args.ap_size), ('step', args.ap_step), ('search', args.ap_search),
                                               ('min_contrast', args.ap_min_contrast)) if value is not None}
    try:
        res = stack_scans(files, opts, args.shift, args.reference, args.mode, args.kappa, args.iterations, args.search, local=local)
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
    if res['local'] is not None:
        for frame, stats in zip(out['frames'], res['local']['frames']):
            frame['local'] = stats
    if args.coverage:
        out['count_png'] = output_path(stem + '_count.png', opts)
        write_png(out['count_png'], np.ascontiguousarray(np.rot90(res['count'].contiguous().cpu().numpy(), opts['img_rotate'] // 90)), 0)
    if args.contrast:
        out['contrast'] = disk.contrast_products(res['stack'], res['circle'], opts, rdr, stem)
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
