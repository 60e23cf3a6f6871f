"""Time the line-profile kernels on HBM-resident synthetic stacks next to the Dopplergram's: shg_line_profile and
shg_line_core_shift at C2 (2000 x 2000x200, 16-bit), C2 8-bit and C5's frame shape (4000 x 2560x256) at H = 5 and H = 12, and
shg_doppler_finish on the C2 map at H = 5 and shg_line_profile_finish on the C2 planes at H = 12 (limb circle, square crop, display
planes).  HIP events bracket each call (run it under
rocprofv3 --kernel-trace --stats for the kernels alone).  Algorithmic bytes: n x ih x (band rows) x B read once, band = [min lo,
max hi] of the whole scan, plus n x ih x 4 per plane written (20 B for the profile, 4 B for the line core)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import ops, synth  # noqa: E402

PEAK = 8e12


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


def case(n, w, h, bits, half_width):
    stack = synth.synth_frames_torch(n, w, h, bits, seed=0, padded=True)
    ih, iw = max(w, h), min(w, h)
    curve = synth.curve_of_row(np.arange(ih, dtype=np.float64), ih, iw)
    fit = np.stack([np.floor(curve), curve - np.floor(curve), np.arange(ih, dtype=float), curve], axis=1)
    fit_d = torch.from_numpy(fit).cuda()
    c = fit[:, 0].astype(np.int64)
    band = int(np.minimum(c + half_width, iw - 2).max() - np.maximum(c - half_width, 1).min() + 1)
    read = n * ih * band * stack.element_size()
    core = ops.line_core_shift(stack, fit_d, half_width)
    planes = ops.line_profile(stack, fit_d, half_width)
    t_core, _ = timeit(lambda: ops.line_core_shift(stack, fit_d, half_width, out=core))
    t_prof, best = timeit(lambda: ops.line_profile(stack, fit_d, half_width, out=planes))
    a_core, a_prof = read + n * ih * 4, read + n * ih * 20
    print('%dx%dx%d %d-bit H=%d, band %d rows: line_core_shift %.1f us (%.1f MB, %.2f of 8 TB/s); line_profile %.1f us median %.1f best '
          '(%.1f MB, %.2f of 8 TB/s) = %.2fx; widths valid %.3f'
          % (n, w, h, bits, half_width, band, t_core * 1e6, a_core / 1e6, a_core / t_core / PEAK, t_prof * 1e6, best * 1e6, a_prof / 1e6,
             a_prof / t_prof / PEAK, t_prof / t_core, float(torch.isfinite(planes[2]).float().mean())))
    return core, planes


def finish(raw, half_width=None):
    """shg_doppler_finish on a map [h, w], or shg_line_profile_finish on planes [5, h, w] with half_width."""
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    planes = 1 if raw.dim() == 2 else raw.shape[0]
    h, w = raw.shape[-2:]
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(0.05, 1.1, h, w)
    circle = (out_w / 2.0, out_h / 2.0, 0.42 * out_h)
    crop, _ = crop_plan(out_h, out_w, circle, dict(SHG_MAIN.default_options(), crop_width_square=True))
    args = (raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, circle, crop) + ((2.0,) if planes == 1 else (half_width, 2.0))
    fn = ops.doppler_finish if planes == 1 else ops.line_profile_finish
    fn(*args)
    med, best = timeit(lambda: fn(*args))
    nw = crop[0]
    alg = planes * (out_h * nw * (4 + 2) + h * w * 4)         # maps + display planes written, the raw planes read once
    print('%s %d x %dx%d -> %dx%d (circle, square crop, display planes): %.1f us median %.1f best; algorithmic %.1f MB -> %.2f TB/s '
          '(includes the output allocations)' % (fn.__name__, planes, h, w, out_h, nw, med * 1e6, best * 1e6, alg / 1e6, alg / med / 1e12))


if __name__ == '__main__':
    for hw in (5, 12):
        core, planes = case(2000, 2000, 200, 16, hw)
        case(2000, 2000, 200, 8, hw)
        case(4000, 2560, 256, 16, hw)
        if hw == 5:
            finish(core)
    finish(planes, 12)
