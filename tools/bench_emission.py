"""Time the emission-line kernels on HBM-resident synthetic stacks next to the line-profile kernels they share their walks with:
shg_line_emission against shg_line_profile at C2 (2000 x 2000x200) 16-bit and 8-bit, H = 5 and H = 12, and
shg_line_emission_finish against shg_line_profile_finish on the C2 planes at H = 12 (limb circle or ring, square crop, display
planes).  The synthetic line is in absorption, so the emission kernel is timed twice: on the stack as it is (nearly every pixel
fails the bracket rule, as empty sky does) and on the complemented stack (every pixel of the disk is measured: the same work as
the profile's).  HIP events bracket each call.  For the kernels alone run it under rocprofv3 and split the trace by launch order
(the two emission workloads, and H = 5 and H = 12, launch the same kernel, so --stats would mix them):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/bench_emission.py
    python3 tools/bench_emission.py --trace DIR
prints, in launch order, the median of the last 30 launches of every run of 36 or more consecutive launches of one kernel (each
timed call is 6 warm-up launches and 30 timed ones), which is the order of the figures in the lines printed by the first command."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import ops, synth  # noqa: E402

PEAK = 8e12


def timeit(fn, iters=30, warmup=6):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in evs)
    return t[len(t) // 2] * 1e-3


def complement(stack):
    """The stack with every sample p replaced by its complement (65535 - p, 255 - p), in a buffer of the same strides."""
    out = torch.empty_strided(stack.shape, stack.stride(), dtype=stack.dtype, device=stack.device)
    if stack.dtype == torch.uint8:
        out.copy_(torch.bitwise_not(stack))
    else:
        out.view(torch.int16).copy_(torch.bitwise_not(stack.view(torch.int16)))
    return out


def case(n, w, h, bits, half_width):
    stack = synth.synth_frames_torch(n, w, h, bits, seed=0, padded=True)
    mirror = complement(stack)
    ih, iw = max(w, h), min(w, h)
    curve = synth.curve_of_row(np.arange(ih, dtype=np.float64), ih, iw)
    fit = np.stack([np.floor(curve), curve - np.floor(curve), np.arange(ih, dtype=float), curve], axis=1)
    fit_d = torch.from_numpy(fit).cuda()
    c = fit[:, 0].astype(np.int64)
    band = int(np.minimum(c + half_width, iw - 2).max() - np.maximum(c - half_width, 1).min() + 1)
    alg = n * ih * band * stack.element_size() + n * ih * 20
    prof = ops.line_profile(stack, fit_d, half_width)
    emis = ops.line_emission(mirror, fit_d, half_width)
    t_prof = timeit(lambda: ops.line_profile(stack, fit_d, half_width, out=prof))
    t_emis = timeit(lambda: ops.line_emission(mirror, fit_d, half_width, out=emis))
    valid = float(torch.isfinite(emis[2]).float().mean())
    t_sky = timeit(lambda: ops.line_emission(stack, fit_d, half_width, out=emis))
    print('%dx%dx%d %d-bit H=%d, band %d rows: line_profile %.1f us (%.2f of 8 TB/s); line_emission on the complement %.1f us (%.2f) = '
          '%.2fx, widths valid %.3f; on the absorption stack %.1f us, finite %.4f'
          % (n, w, h, bits, half_width, band, t_prof * 1e6, alg / t_prof / PEAK, t_emis * 1e6, alg / t_emis / PEAK, t_emis / t_prof, valid,
             t_sky * 1e6, float(torch.isfinite(emis[1]).float().mean())))
    return ops.line_emission(mirror, fit_d, half_width)


def finish(raw, half_width):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    h, w = raw.shape[-2:]
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(0.05, 1.1, h, w)
    circle = (out_w / 2.0, out_h / 2.0, 0.42 * out_h)
    crop, _ = crop_plan(out_h, out_w, circle, dict(SHG_MAIN.default_options(), crop_width_square=True))
    ring = circle[:2] + (circle[2], 1.4 * circle[2])
    geometry = (mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w)
    t_prof = timeit(lambda: ops.line_profile_finish(raw, *geometry, circle, crop, half_width, 2.0))
    t_emis = timeit(lambda: ops.line_emission_finish(raw, *geometry, ring, crop, half_width, 2.0))
    print('finish 5 x %dx%d -> %dx%d (square crop, display planes): line_profile_finish (circle) %.1f us, line_emission_finish (ring) '
          '%.1f us = %.2fx (both include the output allocations)' % (h, w, out_h, crop[0], t_prof * 1e6, t_emis * 1e6, t_emis / t_prof))


def trace_medians(directory):
    """The kernel trace under `directory` split into runs of consecutive launches of one kernel: (kernel, launches, median of the
    last 30 in us) of every run of at least 36, in launch order."""
    import csv
    import glob
    import re
    path = max(glob.glob(directory + '/**/*kernel_trace.csv', recursive=True), key=os.path.getmtime)
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(path)))
    runs = []
    for start, end, name in rows:
        if not runs or runs[-1][0] != name:
            runs.append((name, []))
        runs[-1][1].append(end - start)
    out = []
    for name, d in runs:
        if len(d) >= 36:
            m = re.search(r'\bk_[a-z0-9_]+(<[^(]*>)?', name)
            out.append((m.group(0) if m else name[:60], len(d), float(np.median(d[-30:])) * 1e-3))
    return out


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--trace':
        for name, launches, med in trace_medians(sys.argv[2]):
            print('%-60s %3d launches, median of the last 30: %8.1f us' % (name, launches, med))
        sys.exit(0)
    for hw in (5, 12):
        planes = case(2000, 2000, 200, 16, hw)
        case(2000, 2000, 200, 8, hw)
    finish(planes, 12)
