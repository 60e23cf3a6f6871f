"""Time the Dopplergram's kernels on HBM-resident synthetic stacks: shg_line_core_shift at C2 (2000 x 2000x200, 16-bit), C2 8-bit
and C5's frame shape (4000 x 2560x256), and shg_doppler_finish on the C2 map (with a limb circle, the square crop and the display
plane).  HIP events bracket each call (run it under rocprofv3 --kernel-trace --stats for the kernels alone).  Algorithmic bytes of
the line-core pass: n x ih x (band rows) x B read, band = [min lo, max hi] of the whole scan, plus n x ih x 4 written; `lane bytes`
are what the kernel's lanes actually need (each lane's own eight windows, whole 16-byte pieces)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import ops, synth  # noqa: E402

PEAK = 8e12
HALF_WIDTH = 5


def timeit(fn, iters=30, warmup=5):
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
    return t[len(t) // 2] * 1e-3, t[0] * 1e-3


def windows(fit, iw):
    c = fit[:, 0].astype(np.int64)
    lo, hi = np.maximum(c - HALF_WIDTH, 1), np.minimum(c + HALF_WIDTH, iw - 2)
    return lo, hi


def line_core(n, w, h, bits):
    stack = synth.synth_frames_torch(n, w, h, bits, seed=0, padded=True)
    ih, iw = max(w, h), min(w, h)
    curve = synth.curve_of_row(np.arange(ih, dtype=np.float64), ih, iw)
    fit = np.stack([np.floor(curve), curve - np.floor(curve), np.arange(ih, dtype=float), curve], axis=1)
    fit_d = torch.from_numpy(fit).cuda()
    out = ops.line_core_shift(stack, fit_d, HALF_WIDTH)
    med, best = timeit(lambda: ops.line_core_shift(stack, fit_d, HALF_WIDTH, out=out))
    lo, hi = windows(fit, iw)
    b = stack.element_size()
    band = int(hi.max() - lo.min() + 1)
    alg = n * ih * band * b + n * ih * 4
    # rotated: lane = 8 slit rows (raw columns 8m .. 8m + 7, slit row W - 1 - x)
    x = np.arange(ih)
    y = ih - 1 - x
    lane_rows = sum(int(hi[y[s:s + 8]].max() - lo[y[s:s + 8]].min() + 1) for s in range(0, ih, 8))
    lane = n * lane_rows * 8 * b + n * ih * 4
    print('line_core_shift %dx%dx%d %d-bit H=%d: %.1f us median %.1f best; band %d rows, algorithmic %.1f MB -> %.2f TB/s = %.2f of 8 TB/s; '
          'lane bytes %.1f MB -> %.2f TB/s; valid %.3f' % (n, w, h, bits, HALF_WIDTH, med * 1e6, best * 1e6, band, alg / 1e6, alg / med / 1e12,
                                                            alg / med / PEAK, lane / 1e6, lane / med / 1e12, float(torch.isfinite(out).float().mean())))
    return out


def finish(raw):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    h, w = raw.shape
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(0.05, 1.1, h, w)
    circle = (out_w / 2.0, out_h / 2.0, 0.42 * out_h)
    crop, _ = crop_plan(out_h, out_w, circle, dict(SHG_MAIN.default_options(), crop_width_square=True))
    args = (raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, circle, crop, 2.0)
    ops.doppler_finish(*args)
    med, best = timeit(lambda: ops.doppler_finish(*args))
    nw = crop[0]
    alg = out_h * nw * (4 + 2) + h * w * 4        # map + display plane written, the raw map read once
    print('doppler_finish %dx%d -> %dx%d (circle, square crop, display plane): %.1f us median %.1f best; algorithmic %.1f MB -> %.2f TB/s '
          '(includes the output allocations)' % (h, w, out_h, nw, med * 1e6, best * 1e6, alg / 1e6, alg / med / 1e12))


if __name__ == '__main__':
    raw = line_core(2000, 2000, 200, 16)
    line_core(2000, 2000, 200, 8)
    line_core(4000, 2560, 256, 16)
    finish(raw)
