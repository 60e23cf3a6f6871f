"""Stack a series of scans of one line into one disk: every scan's 16-bit disk and fitted circle, one global
similarity transform a scan -- scale from the radii, translation from the centres, refined by an exact search over integer offsets
and a parabola through its minimum --, then all disks resampled into the reference scan's grid and combined pixel by pixel in one
launch.  The resample-and-combine and the sums of squared differences are HIP kernels (ops.stack_combine_u16, ops.shift_ssd_u16);
the arithmetic between them is host float64, written step by step so that tests/stack_ref.py restates it bit for bit.  With
--local every scan is also bent by a field of local alignment points: one offset search a lattice node
(ops.patch_ssd_u16), refined and filled on the host, and the combine that reads each scan through its field
(ops.stack_combine_field_u16); tests/align_ref.py restates those.  With the quality flags every scan's
sharpness is measured on a lattice of patches (ops.patch_sharpness_u16): the best scans are selected, the sharpest may be the
reference, and --lucky keeps the best scans node by node through a weight lattice a scan (ops.stack_combine_weighted_u16);
tests/quality_ref.py restates those.

    python -m solex_ser_recon_en_amd.stack A.ser B.ser ... [--shift S] [--reference K|best] [--mode mean|median|sigma] [--kappa X]
        [--iterations I] [--search S] [--local [--ap-size P] [--ap-step D] [--ap-search S] [--ap-min-contrast X]] [--quality]
        [--best K] [--min-quality X] [--lucky K] [--quality-power P] [--quality-arm D] [--quality-size N] [--quality-step N]
        [--coverage] [--contrast] [SHG_MAIN flags]
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


def _series(images, circles, reference, records=None, fields=None):
    """(the images on the device, how many): circles -- and records and fields, where given -- are as many, and the reference is
    one of them (ValueError else)."""
    from .device import to_device_u16
    images = [to_device_u16(t) for t in images]
    n = len(images)
    if n < 1 or any(t is not None and len(t) != n for t in (circles, records, fields)):
        raise ValueError('%d images and %d circles' % (n, len(circles)) if records is None else
                         '%d images, %d records and %d circles' % (n, len(records), len(circles)))
    if not 0 <= int(reference) < n:
        raise ValueError('reference %r outside the %d frames' % (reference, n))
    return images, n


def _check_region(region):
    if not (math.isfinite(region) and region > 0):
        raise ValueError('region must be a positive fraction of the radius')


def _region_disk(circle, region):
    """The disk two planes are compared over, or one is measured over: (cx, cy, region rad), one float64 product."""
    cx, cy, rad = (float(v) for v in circle)
    return cx, cy, float(np.float64(region) * np.float64(rad))


def _resampled_alone(image, row, shape):
    """One image resampled alone by its row (s, tx, ty, gain) into a grid of `shape`."""
    from . import ops
    return ops.stack_combine_u16([image], [row], shape, 'mean', want_count=False)[0]


def register_disks(images, circles, reference=0, search=8, region=0.9):
    """One record a frame: {'s', 'tx', 'ty' (the refined transform into the frame), 'gain' (level of the reference / level of the
    frame), 'level', 'offset' (u + du, v + dv), 'ssd_per_pixel', 'pixels', 'rejected'}.  The frame is resampled alone into the
    reference's grid, compared with the reference over the disk (cx_0, cy_0, region rad_0) at every integer offset within `search`
    pixels, and the first minimum refined by a parabola an axis.  The reference's own record is the identity.  ValueError for a
    level of 0."""
    from . import ops
    images, n = _series(images, circles, reference)
    if not 0 <= int(search) <= MAX_SEARCH:
        raise ValueError('search must be 0 to %d pixels, got %r' % (MAX_SEARCH, search))
    _check_region(region)
    reference, search = int(reference), int(search)
    levels = [disk_level(images[i], circles[i]) for i in range(n)]
    for i, level in enumerate(levels):
        if not level > 0:
            raise ValueError('frame %d has a brightness level of %r: nothing to scale' % (i, level))
    ref_circle = tuple(float(v) for v in circles[reference])
    ref_img = images[reference]
    shape = tuple(ref_img.shape)
    disk = _region_disk(ref_circle, region)
    records = []
    for i in range(n):
        if i == reference:
            records.append({'s': 1.0, 'tx': 0.0, 'ty': 0.0, 'gain': 1.0, 'level': levels[i], 'offset': (0.0, 0.0), 'ssd_per_pixel': 0.0,
                            'pixels': None, 'rejected': False})
            continue
        s, tx, ty = initial_transform(circles[i], ref_circle)
        gain = np.float64(levels[reference]) / np.float64(levels[i])
        plane = _resampled_alone(images[i], (s, tx, ty, gain), shape)
        fit = refine_offset(ops.shift_ssd_u16(ref_img, plane, search, disk).cpu().numpy(), search)
        tx2, ty2 = refined_transform(s, tx, ty, fit)
        records.append({'s': float(s), 'tx': float(tx2), 'ty': float(ty2), 'gain': float(gain), 'level': levels[i],
                        'offset': (fit['u'] + fit['du'], fit['v'] + fit['dv']),
                        'ssd_per_pixel': fit['ssd'] / fit['pixels'] if fit['pixels'] else float('nan'), 'pixels': fit['pixels'],
                        'rejected': fit['rejected']})
    return records


# ---- local alignment points ----
LOCAL_DEFAULTS = {'step': 16, 'size': 33, 'search': 4, 'region': 0.9, 'min_contrast': 0.0}


def _check_patches(step, size, lattice, patches):
    """The ranges of a lattice's step and its patches' size, in the caller's wording."""
    if not 8 <= int(step) <= 128:
        raise ValueError('the %s step must be 8 to 128 pixels, got %r' % (lattice, step))
    if not (3 <= int(size) <= 65 and int(size) % 2 == 1):
        raise ValueError('the %s size must be odd and 3 to 65 pixels, got %r' % (patches, size))


def check_local(step, size, search, min_contrast=0.0):
    _check_patches(step, size, 'alignment points\'', 'alignment patches\'')
    if not 0 <= int(search) <= MAX_SEARCH:
        raise ValueError('the alignment points\' search must be 0 to %d pixels, got %r' % (MAX_SEARCH, search))
    if not min_contrast >= 0:
        raise ValueError('min_contrast must be >= 0, got %r' % (min_contrast,))


def align_lattice(shape, step):
    """The lattice of alignment points over a grid of `shape`: nodes at (j step, i step), as many as cover the grid -> (gh, gw,
    points int32 [gh gw, 2] of (row, col) in row-major order): (gh, gw) = ops.lattice_shape(shape, step).  (The last row or
    column of nodes may lie beyond the grid.)"""
    from .ops import lattice_shape
    step = int(step)
    if int(shape[0]) < 1 or int(shape[1]) < 1 or step < 1:
        raise ValueError('a lattice needs a grid and a step of at least one pixel')
    gh, gw = lattice_shape(shape, step)
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
    images, n = _series(images, circles, reference, records)
    check_local(step, size, search, min_contrast)
    _check_region(region)
    reference, step, search, half = int(reference), int(step), int(search), (int(size) - 1) // 2
    ref_img = images[reference]
    shape = tuple(ref_img.shape)
    disk = _region_disk(circles[reference], region)
    gh, gw, points = align_lattice(shape, step)
    points_dev = torch.from_numpy(points).to(ref_img.device)
    fields, stats = [], []
    for i in range(n):
        rec = records[i]
        if i == reference or rec['rejected']:
            fields.append(None), stats.append(None)
            continue
        plane = _resampled_alone(images[i], (rec['s'], rec['tx'], rec['ty'], rec['gain']), shape)
        table = ops.patch_ssd_u16(ref_img, plane, points_dev, half, search, disk).cpu().numpy()
        raw, measured = measure_field(table, gh, gw, half, search, min_contrast)
        fields.append(torch.from_numpy(fill_field(raw, measured)).to(ref_img.device))
        stats.append(field_stats(raw, measured))
    return fields, stats


# ---- ranking scans by sharpness ----
QUALITY_DEFAULTS = {'step': 16, 'size': 33, 'arm': 3, 'region': 0.9, 'best': None, 'min_quality': None, 'lucky': None, 'power': 0.0}
MAX_WEIGHT = float(2 ** 20)


def check_quality(step, size, arm, region=0.9, best=None, min_quality=None, lucky=None, power=0.0):
    _check_patches(step, size, 'quality lattice\'s', 'quality patches\'')
    if not 1 <= int(arm) <= 8:
        raise ValueError('the Laplacian\'s arm must be 1 to 8 pixels, got %r' % (arm,))
    _check_region(region)
    if best is not None and int(best) < 2:
        raise ValueError('best must keep at least two scans, got %r' % (best,))
    if min_quality is not None and not 0 <= min_quality <= 1:
        raise ValueError('min_quality is a fraction of the best scan\'s quality, 0 to 1, got %r' % (min_quality,))
    if lucky is not None and int(lucky) < 1:
        raise ValueError('lucky must keep at least one scan a node, got %r' % (lucky,))
    if not (math.isfinite(power) and power >= 0):
        raise ValueError('power must be finite and >= 0, got %r' % (power,))


def patch_quality(table, half):
    """From patch_sharpness_u16's rows (host, [n, 4] integers: pixels, sum I, sum I^2, sum L^2) -> q float64 [n], the mean squared
    Laplacian over the squared mean: q = ((double)sum L^2 * (double)pixels) / ((double)sum I * (double)sum I), each product and the
    quotient one float64 operation.  q is NaN where 2 pixels < (2 half + 1)^2 or sum I = 0."""
    table = np.asarray(table).reshape(-1, 4).astype(np.int64)
    pixels, total, lap = table[:, 0], table[:, 1], table[:, 3]
    bad = (2 * pixels < (2 * int(half) + 1) ** 2) | (total == 0)
    num = lap.astype(np.float64) * pixels.astype(np.float64)
    den = total.astype(np.float64) * total.astype(np.float64)
    return np.where(bad, np.nan, num / np.where(bad, 1.0, den))


def map_figure(qmap):
    """(np.median of a map's finite nodes -- 0.0 when there is none --, how many they are)."""
    finite = qmap[np.isfinite(qmap)]
    return (float(np.median(finite)) if finite.size else 0.0), int(finite.size)


def disk_quality(image, circle, step=16, size=33, arm=3, region=0.9):
    """The sharpness of one scan on its own grid, before any registration -> {'map': float64 [gh, gw] (host), patch_quality of the
    size x size patches around the nodes of align_lattice(image.shape, step) over the disk (cx, cy, region rad) with the Laplacian's
    arm `arm` (ops.patch_sharpness_u16); 'quality': the median of the map's finite nodes (0.0 when there is none); 'nodes': how many
    those are}."""
    from . import ops
    from .device import to_device_u16
    check_quality(step, size, arm, region)
    image = to_device_u16(image)
    half = (int(size) - 1) // 2
    gh, gw, points = align_lattice(tuple(image.shape), int(step))
    table = ops.patch_sharpness_u16(image, points, half, int(arm), _region_disk(circle, region)).cpu().numpy()
    qmap = patch_quality(table, half).reshape(gh, gw)
    figure, nodes = map_figure(qmap)
    return {'map': qmap, 'quality': figure, 'nodes': nodes}


def local_quality(images, records, circles, reference, fields=None, step=16, size=33, arm=3, region=0.9):
    """One quality map a scan on the REFERENCE's lattice align_lattice(reference's shape, step), measured on each scan's OWN pixels
    (a resampled plane is blurred by an amount that depends on the fractional offset, so it is never measured) -> a list of float64
    [gh, gw] host arrays, None for a rejected scan.  Node (j, i) at the reference's pixel (r, c) = (j step, i step) maps to the
    scan's point (rint(ty + s (r + dy)), rint(tx + s (c + dx))) -- float64, one operation a step, (dx, dy) the scan's field at the
    node (fields: local_fields', device or host arrays) or 0 without one, the result clipped to int32 --; the patch is `size`
    source pixels a side, the disk the scan's own (cx_s, cy_s, region rad_s), and the figure patch_quality's."""
    from . import ops
    check_quality(step, size, arm, region)
    images, n = _series(images, circles, reference, records, fields)
    half = (int(size) - 1) // 2
    gh, gw, points = align_lattice(tuple(images[int(reference)].shape), int(step))
    r, c = points[:, 0].astype(np.float64), points[:, 1].astype(np.float64)
    maps = []
    for i in range(n):
        rec = records[i]
        if rec['rejected']:
            maps.append(None)
            continue
        s, tx, ty = np.float64(rec['s']), np.float64(rec['tx']), np.float64(rec['ty'])
        rr, cc = r, c
        if fields is not None and fields[i] is not None:
            f = fields[i]
            f = np.asarray(f.cpu().numpy() if hasattr(f, 'cpu') else f, dtype=np.float64).reshape(gh * gw, 2)
            cc, rr = c + f[:, 0], r + f[:, 1]
        src = np.stack([np.rint(ty + s * rr), np.rint(tx + s * cc)], axis=1)
        src = np.clip(src, -2.0 ** 31, 2.0 ** 31 - 1.0).astype(np.int32)
        table = ops.patch_sharpness_u16(images[i], src, half, int(arm), _region_disk(circles[i], region)).cpu().numpy()
        maps.append(patch_quality(table, half).reshape(gh, gw))
    return maps


def quality_ranks(maps):
    """(q float64 [n, gh, gw], rank int64 [n, gh, gw]): at every node the scans ranked by q descending, ties to the lower index,
    NaN last (among NaNs the lower index first)."""
    q = np.stack([np.asarray(m, dtype=np.float64) for m in maps])
    key = np.where(np.isnan(q), -np.inf, q)
    order = np.argsort(-key, axis=0, kind='stable')
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(q.shape[0])[:, None, None], q.shape), axis=0)
    return q, rank


def quality_weights(maps, keep=None, power=0.0):
    """One weight lattice a scan from the scans' quality maps (float64 [gh, gw] each) -> a list of float64 [gh, gw] host arrays.  At
    each node the scans are ranked by q descending, ties to the lower index, NaN last; w = 1 for rank < keep, else 0 (keep None
    keeps all).  With power > 0 and a largest q at the node that is > 0, w is multiplied by np.power(q / that largest q, power), and
    by 0 where q is NaN.  A node where every q is NaN (the limb, the sky) gets weight 1 for every scan: it stacks as it always
    did.  Every weight is finite and in [0, 1]."""
    if not maps:
        raise ValueError('no quality map')
    if keep is not None and int(keep) < 1:
        raise ValueError('keep must be at least 1, got %r' % (keep,))
    if not (math.isfinite(power) and power >= 0):
        raise ValueError('power must be finite and >= 0, got %r' % (power,))
    q, rank = quality_ranks(maps)
    n = q.shape[0]
    w = np.ones(q.shape, dtype=np.float64) if keep is None else (rank < int(keep)).astype(np.float64)
    nan = np.isnan(q)
    if power > 0:
        best = np.max(np.where(nan, -np.inf, q), axis=0)
        with np.errstate(invalid='ignore', divide='ignore'):
            factor = np.power(np.where(nan, 0.0, q) / np.where(best > 0.0, best, 1.0)[None], np.float64(power))
        w = np.where((best > 0.0)[None], w * np.where(nan, 0.0, factor), w)
    w = np.where(nan.all(axis=0)[None], 1.0, w)
    return [np.ascontiguousarray(w[k]) for k in range(n)]


def node_shares(maps):
    """The share of the nodes with a finite q that each scan wins (rank 0), one float a scan; zeros when no node has one."""
    q, rank = quality_ranks(maps)
    some = ~np.isnan(q).all(axis=0)
    total = int(some.sum())
    return [float(((rank[k] == 0) & some).sum() / total) if total else 0.0 for k in range(q.shape[0])]


def select_scans(qualities, best=None, min_quality=None):
    """The indices (ascending) of the scans that pass: with `best` the K of the largest quality (ties to the lower index), with
    `min_quality` those whose quality is >= min_quality x the largest (one float64 product); with both, the best K of those.
    ValueError when fewer than two pass (also for best < 2)."""
    q = [np.float64(t) for t in qualities]
    keep = list(range(len(q)))
    if min_quality is not None and q:
        floor = np.float64(min_quality) * max(q)
        keep = [i for i in keep if q[i] >= floor]
    if best is not None:
        if int(best) < 2:
            raise ValueError('best must keep at least two scans, got %r' % (best,))
        keep = sorted(sorted(keep, key=lambda i: (-q[i], i))[:int(best)])
    if len(keep) < 2:
        raise ValueError('only %d of %d scans pass the quality selection: nothing to stack' % (len(keep), len(q)))
    return keep


def check_weights(weights, shape):
    """The weight lattices as the combine wants them: host float64 arrays of `shape`, finite, >= 0 and <= 2^20 (ValueError else)."""
    out = []
    for k, w in enumerate(weights):
        if w is None:
            out.append(None)
            continue
        w = np.ascontiguousarray(w.cpu().numpy() if hasattr(w, 'cpu') else w, dtype=np.float64)
        if w.shape != tuple(shape):
            raise ValueError('weight lattice %d is %r, the lattice %r' % (k, w.shape, tuple(shape)))
        if not (np.isfinite(w).all() and (w >= 0).all() and (w <= MAX_WEIGHT).all()):
            raise ValueError('weight lattice %d has a node that is not finite, negative or above 2^20' % k)
        out.append(w)
    return out


def stack_disks(images, transforms, mode='sigma', kappa=2.5, iterations=2, shape=None, fields=None, step=None, weights=None):
    """The fused call: the images resampled by their transforms -- rows (s, tx, ty, gain) or register_disks' records -- into a grid
    of `shape` (default: the first image's) and combined -> (stack uint16, count uint8) on the device.  fields (local_fields', one
    an image, None for none) and their lattice's step: each image is bent by its field as well.  weights (quality_weights', one
    host or device float64 [gh, gw] lattice an image on the lattice of `step`, None for 1): the weighted combine
    (ops.stack_combine_weighted_u16), after the lattices were checked on the host to be finite, >= 0 and <= 2^20; ValueError with
    mode 'median'."""
    from . import ops
    from .device import to_device_u16
    images = [to_device_u16(t) for t in images]
    rows = [(t['s'], t['tx'], t['ty'], t['gain']) if isinstance(t, dict) else tuple(t) for t in transforms]
    if len(images) > MAX_SCANS:
        raise ValueError('at most %d frames are stacked at a time, got %d' % (MAX_SCANS, len(images)))
    if fields is not None and step is None:
        raise ValueError('fields need their lattice\'s step')
    if weights is not None:
        if mode == 'median':
            raise ValueError('there is no weighted median: weights go with mode mean or sigma')
        if step is None:
            raise ValueError('weights need their lattice\'s step')
        if len(weights) != len(images):
            raise ValueError('%d images and %d weight lattices' % (len(images), len(weights)))
    shape = tuple(images[0].shape) if shape is None else shape
    if weights is not None:
        import torch
        lattices = [None if w is None else torch.from_numpy(w).to(images[0].device)
                    for w in check_weights(weights, ops.lattice_shape(shape, step))]
        return ops.stack_combine_weighted_u16(images, rows, fields, lattices, step, shape, mode, kappa, iterations)
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


def stack_scans(files, options=None, shift=0, reference=0, mode='sigma', kappa=2.5, iterations=2, search=8, region=0.9, local=None,
                quality=None, dejitter=None, derotate=None):
    """The scans' disks at `shift` registered to the one of files[reference] and stacked -> {'stack' uint16, 'count' uint8 (device
    tensors on the reference's grid), 'circle' (the reference's), 'records' (register_disks', one a file), 'used', 'rejected' (indices
    into files), 'images', 'circles', 'shift', 'mode', 'ratio', 'phi', 'crop' (the reference's), 'local'}.  local: None, or a dict of
    local_fields' parameters ('step', 'size', 'search', 'region', 'min_contrast'; LOCAL_DEFAULTS for those left out): every used
    frame is also bent by its field of alignment points, and 'local' is {'step', 'size', 'search', 'region', 'min_contrast',
    'fields', 'frames' (local_fields' two lists, one entry a file)} instead of None.  ValueError for fewer than 2 or more than 32
    files, for ratio_fixe / slant_fix, de-vignette and a frame shard, and when fewer than two files survive the registration.
    quality: None, or a dict of {'step', 'size', 'arm', 'region', 'best', 'min_quality', 'lucky', 'power'} (QUALITY_DEFAULTS for those
    left out; reference 'best' alone measures with the defaults).  Every scan's disk_quality is measured on its own grid; reference
    'best' is the first scan of the largest figure; of the scans that register, select_scans(best, min_quality) keeps some -- the
    others are in 'rejected' as well and alone in the new 'unselected'; the reference's grid is used even when the reference is not
    kept --; with 'lucky' K or 'power' > 0 the kept scans' local_quality maps become quality_weights(maps, K, power) and the combine is
    the weighted one.  With `local` the quality lattice's step is local['step'] (the combine has one lattice): giving quality['step']
    as well is a ValueError, as are weights with mode 'median'.  'quality' is None, or the parameters and 'figures' (a float a
    file), 'maps' (disk_quality's, a file), 'selected' (a bool a file), 'local_maps', 'weights' (host lattices a file, None for a
    file that is not stacked; both None without lucky / power) and 'shares' (node_shares of the kept scans' maps a file, or None).
    dejitter: disk.scan_disk's, for every scan; the result then holds 'jitter', dejitter.measure's record a file.
    derotate: None, or a dict of derotate.series_plan's arguments ('north', 'b0', and 'mirror', 'times', 'interval', 'law', 'clv'):
    once the reference is chosen, every other scan's disk is derotated to the reference's time on its own grid with its own circle
     and the registration and everything after it see the derotated images; the reference is not resampled.
    The result then holds 'derotate', derotate_disk's record a file (derotate.derotate_series: the reference's with rates of zero and
    nothing moved, 'behind_limb' None for the others), and 'images' are the derotated ones."""
    files = list(files)
    if len(files) < 2:
        raise ValueError('stacking needs at least two scans, got %d' % len(files))
    if len(files) > MAX_SCANS:
        raise ValueError('at most %d scans are stacked at a time, got %d' % (MAX_SCANS, len(files)))
    if reference != 'best' and not (isinstance(reference, (int, np.integer)) and 0 <= int(reference) < len(files)):
        raise ValueError('reference %r is neither \'best\' nor one of the %d scans' % (reference, len(files)))
    check_combine(mode, kappa, iterations)
    if quality is None and reference == 'best':
        quality = {}
    if quality is not None:
        unknown = sorted(set(quality) - set(QUALITY_DEFAULTS))
        if unknown:
            raise ValueError('quality knows %s, got %s' % (', '.join(QUALITY_DEFAULTS), ', '.join(unknown)))
        if local is not None and quality.get('step') is not None:
            raise ValueError('with local alignment the quality lattice is the alignment points\': give local[\'step\'] alone')
        quality = dict(QUALITY_DEFAULTS, **{k: v for k, v in quality.items() if v is not None})
        if local is not None:
            quality['step'] = dict(LOCAL_DEFAULTS, **local)['step']
        check_quality(**quality)
        if (quality['lucky'] is not None or quality['power'] > 0) and mode == 'median':
            raise ValueError('there is no weighted median: lucky regions go with mode mean or sigma')
    if local is not None:
        unknown = sorted(set(local) - set(LOCAL_DEFAULTS))
        if unknown:
            raise ValueError('local knows %s, got %s' % (', '.join(LOCAL_DEFAULTS), ', '.join(unknown)))
        local = dict(LOCAL_DEFAULTS, **local)
        check_local(local['step'], local['size'], local['search'], local['min_contrast'])
    if derotate is not None:
        from . import derotate as dr
        unknown = sorted(set(derotate) - set(dr.SERIES_KEYS))
        if unknown:
            raise ValueError('derotate knows %s, got %s' % (', '.join(dr.SERIES_KEYS), ', '.join(unknown)))
        derotate = dr.series_plan(files, options, **derotate)
    disks = [disk.scan_disk(f, options, shift, 'stacking', dejitter) for f in files]
    images, circles = [d['image'] for d in disks], [d['circle'] for d in disks]
    measured = None
    if quality is not None:
        measured = [disk_quality(images[i], circles[i], quality['step'], quality['size'], quality['arm'], quality['region'])
                    for i in range(len(files))]
        if reference == 'best':
            reference = max(range(len(files)), key=lambda i: (measured[i]['quality'], -i))
    if derotate is not None:
        images, derotated = dr.derotate_series(images, circles, derotate, int(reference))
    records = register_disks(images, circles, reference, search, region)
    used = [i for i, rec in enumerate(records) if not rec['rejected']]
    if len(used) < 2:
        raise ValueError('only %d of %d scans could be registered: nothing to stack' % (len(used), len(files)))
    unselected = []
    if quality is not None and (quality['best'] is not None or quality['min_quality'] is not None):
        keep = select_scans([measured[i]['quality'] for i in used], quality['best'], quality['min_quality'])
        unselected = [i for k, i in enumerate(used) if k not in keep]
        used = [used[k] for k in keep]
    ref = disks[int(reference)]
    fields = None
    if local is not None:
        fields, frames = local_fields(images, records, circles, reference, **local)
        local = dict(local, fields=fields, frames=frames)
        fields = [fields[i] for i in used]
    weights, step = None, None if local is None else local['step']
    if quality is not None:
        quality = dict(quality, figures=[m['quality'] for m in measured], maps=[m['map'] for m in measured],
                       selected=[i in used for i in range(len(files))], local_maps=None, weights=None, shares=None)
        if quality['lucky'] is not None or quality['power'] > 0:
            step = quality['step']
            # (every file is measured, the reference for the lattice among them, kept or not; the kept scans are ranked)
            maps = local_quality(images, records, circles, reference, None if local is None else local['fields'], step, quality['size'],
                                 quality['arm'], quality['region'])
            maps = [maps[i] for i in used]
            weights = quality_weights(maps, quality['lucky'], quality['power'])

            def per_file(values):
                return [values[used.index(i)] if i in used else None for i in range(len(files))]

            quality.update(local_maps=per_file(maps), weights=per_file(weights), shares=per_file(node_shares(maps)))
    stack, count = stack_disks([images[i] for i in used], [records[i] for i in used], mode, kappa, iterations, tuple(ref['image'].shape),
                               fields, step, weights)
    res = {'quality': quality, 'unselected': unselected, 'local': local, 'stack': stack, 'count': count, 'circle': ref['circle'],
           'records': records, 'used': used,
           'rejected': [i for i in range(len(files)) if i not in used], 'images': images, 'circles': circles, 'shift': ref['shift'],
           'mode': mode, 'kappa': float(kappa), 'iterations': int(iterations), 'reference': int(reference), 'ratio': ref['ratio'],
           'phi': ref['phi'], 'crop': ref['crop']}
    if dejitter is not None:
        res['jitter'] = [d['jitter'] for d in disks]
    if derotate is not None:
        res['derotate'] = derotated
    return res


# ---- command line ---------------------------------------------------------------------------------
def main(argv=None):
    from .linemaps import _print_json
    from .png_io import write_png
    from .solex_util import output_path
    from .video_reader import video_reader
    p = argparse.ArgumentParser(prog='python -m solex_ser_recon_en_amd.stack',
                                usage='%(prog)s FILE FILE ... [--shift S] [--reference K|best] [--mode mean|median|sigma] [--kappa X] '
                                      '[--iterations I] [--search S] [--local [--ap-size P] [--ap-step D] [--ap-search S] '
                                      '[--ap-min-contrast X]] [--quality] [--best K] [--min-quality X] [--lucky K] [--quality-power P] '
                                      '[--quality-arm D] [--quality-size N] [--quality-step N] [--coverage] [--contrast] [--dejitter] '
                                      '[--derotate --north P --b0 B [--mirror] [--times T0,T1,.. | --interval SECONDS] [--rotation A,B,C] '
                                      '[--no-clv]] [SHG_MAIN flags]',
                                description='Stack a series of scans of one line: register every scan\'s disk to the reference scan\'s '
                                            'and combine them into one image.')
    p.add_argument('--shift', type=int, default=0, help='pixel shift of the disks to stack (the -w shift; default 0: the line centre)')
    def reference_arg(text):
        return 'best' if text == 'best' else int(text)

    p.add_argument('--reference', type=reference_arg, default=0, help='index of the scan whose grid the stack is made on (default 0: the '
                                                                      'first), or "best": the sharpest scan')
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
    p.add_argument('--quality', action='store_true', help='measure every scan\'s sharpness and report it; the stack is the usual one')
    p.add_argument('--best', type=int, default=None, help='stack only the K sharpest scans (at least 2)')
    p.add_argument('--min-quality', type=float, default=None, help='stack only the scans whose sharpness is at least this fraction (0 to 1) of '
                                                                   'the sharpest scan\'s')
    p.add_argument('--lucky', type=int, default=None, help='lucky regions: at every lattice node keep the K sharpest scans, blended between nodes')
    p.add_argument('--quality-power', type=float, default=None, help='weight a kept scan by (its sharpness / the node\'s best)^P (default 0: '
                                                                     'equal weights)')
    p.add_argument('--quality-arm', type=int, default=None, help='arm of the Laplacian the sharpness is measured with, pixels (1 to 8; default 3)')
    p.add_argument('--quality-size', type=int, default=None, help='side of a quality patch in pixels (odd, 3 to 65; default 33)')
    p.add_argument('--quality-step', type=int, default=None, help='distance of the quality lattice\'s nodes in pixels (8 to 128; default 16; '
                                                                  'with --local the alignment points\' step is used)')
    p.add_argument('--coverage', action='store_true', help='also the number of frames behind every pixel (<base>_stack_count.png)')
    p.add_argument('--contrast', action='store_true', help='also the contrast products of the stack (<base>_stack_clahe.png, ...)')
    disk.add_dejitter_argument(p)
    from . import derotate as dr
    dr.add_series_arguments(p)
    series = []

    def checks(args):
        series.append(dr.series_from_arguments(p, args))
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
        if args.best is not None and args.best < 2:
            p.error('--best must be at least 2')
        if args.min_quality is not None and not 0 <= args.min_quality <= 1:
            p.error('--min-quality must be 0 to 1')
        if args.lucky is not None and args.lucky < 1:
            p.error('--lucky must be at least 1')
        if args.quality_power is not None and not (math.isfinite(args.quality_power) and args.quality_power >= 0):
            p.error('--quality-power must be finite and >= 0')
        if args.quality_arm is not None and not 1 <= args.quality_arm <= 8:
            p.error('--quality-arm must be 1 to 8')
        if args.quality_size is not None and not (3 <= args.quality_size <= 65 and args.quality_size % 2 == 1):
            p.error('--quality-size must be odd and 3 to 65')
        if args.quality_step is not None and not 8 <= args.quality_step <= 128:
            p.error('--quality-step must be 8 to 128')
        if args.quality_step is not None and args.local:
            p.error('--quality-step cannot be given with --local: the quality lattice is the alignment points\' (--ap-step)')
        if args.mode == 'median' and (args.lucky is not None or args.quality_power is not None):
            p.error('--lucky and --quality-power need --mode mean or sigma: there is no weighted median')

    def file_checks(args, files):
        if len(files) > MAX_SCANS:
            p.error('at most %d scans are stacked at a time (got %d)' % (MAX_SCANS, len(files)))
        if args.reference != 'best' and not 0 <= args.reference < len(files):
            p.error('--reference must be 0 to %d' % (len(files) - 1))
        if series[0] is not None and series[0]['times'] is not None and len(series[0]['times']) != len(files):
            p.error('--times names %d times for %d scans' % (len(series[0]['times']), len(files)))

    args, opts, files = disk.parse(p, argv, 'stack', 'stacking', checks, file_checks, least=2, most=None,
                                   need='at least two SER or AVI files are needed')
    local = None
    if args.local:
        local = {key: value for key, value in (('size', args.ap_size), ('step', args.ap_step), ('search', args.ap_search),
                                               ('min_contrast', args.ap_min_contrast)) if value is not None}
    quality = {key: value for key, value in (('best', args.best), ('min_quality', args.min_quality), ('lucky', args.lucky),
                                             ('power', args.quality_power), ('arm', args.quality_arm), ('size', args.quality_size),
                                             ('step', args.quality_step)) if value is not None}
    if not (quality or args.quality or args.reference == 'best'):
        quality = None
    try:
        res = stack_scans(files, opts, args.shift, args.reference, args.mode, args.kappa, args.iterations, args.search, local=local,
                          quality=quality, dejitter={} if args.dejitter else None, derotate=series[0])
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    ref_path = files[res['reference']]
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
    if res['quality'] is not None:
        q = res['quality']
        for frame, figure in zip(out['frames'], q['figures']):
            frame['quality'] = figure
        out['quality'] = {'step': q['step'], 'size': q['size'], 'arm': q['arm'], 'region': q['region'], 'best': q['best'],
                          'min_quality': q['min_quality'], 'lucky': q['lucky'], 'power': q['power'], 'reference': res['reference'],
                          'unselected': [files[i] for i in res['unselected']], 'shares': q['shares']}
    if args.dejitter:
        out['jitter'] = [disk.jitter_summary(j) for j in res['jitter']]
    if args.derotate:
        for frame, record in zip(out['frames'], res['derotate']):
            frame['derotate'] = {'dt_minutes': record['dt_days'] * 1440.0, 'a_equator': record['a_equator'], 'max_px': record['max_px']}
    if args.coverage:
        out['count_png'] = output_path(stem + '_count.png', opts)
        write_png(out['count_png'], np.ascontiguousarray(np.rot90(res['count'].contiguous().cpu().numpy(), opts['img_rotate'] // 90)), 0)
    if args.contrast:
        out['contrast'] = disk.contrast_products(res['stack'], res['circle'], opts, rdr, stem)
    return _print_json(out, res)


if __name__ == '__main__':
    sys.exit(main())
