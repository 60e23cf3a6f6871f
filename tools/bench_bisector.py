"""Time the line-bisector kernel on HBM-resident synthetic stacks next to the line-profile kernel, in the same process:
shg_line_bisector at K = 1, 4 and 8 levels and shg_line_profile, at C2 (2000 x 2000x200, 16-bit), C2 8-bit and C5's frame shape
(4000 x 2560x256) at H = 5 and H = 12, and shg_line_bisector_finish on the C2 planes (K = 4, H = 12: limb circle, square crop,
display planes).  HIP events bracket each call (run it under rocprofv3 --kernel-trace --stats for the kernels alone).  Algorithmic
bytes: n x ih x (band rows) x B read once, band = [min lo, max hi] of the whole scan, plus n x ih x 4 per plane written (8 K B for
the bisectors, 20 B for the profile)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import ops, synth  # noqa: E402
from tools.bench_lineprofile import PEAK, timeit  # noqa: E402

LEVELS = {1: (0.5,), 4: (0.2, 0.4, 0.6, 0.8), 8: (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)}


def case(n, w, h, bits, half_width):
    stack = synth.synth_frames_torch(n, w, h, bits, seed=0, padded=True)
    ih, iw = max(w, h), min(w, h)
    curve = synth.curve_of_row(np.arange(ih, dtype=np.float64), ih, iw)
    fit = np.stack([np.floor(curve), curve - np.floor(curve), np.arange(ih, dtype=float), curve], axis=1)
    fit_d = torch.from_numpy(fit).cuda()
    c = fit[:, 0].astype(np.int64)
    band = int(np.minimum(c + half_width, iw - 2).max() - np.maximum(c - half_width, 1).min() + 1)
    read = n * ih * band * stack.element_size()
    planes = ops.line_profile(stack, fit_d, half_width)
    t_prof, _ = timeit(lambda: ops.line_profile(stack, fit_d, half_width, out=planes))
    a_prof = read + n * ih * 20
    print('%dx%dx%d %d-bit H=%d, band %d rows: line_profile %.1f us (%.1f MB, %.2f of 8 TB/s)'
          % (n, w, h, bits, half_width, band, t_prof * 1e6, a_prof / 1e6, a_prof / t_prof / PEAK), flush=True)
    out = None
    for k, levels in LEVELS.items():
        bis = ops.line_bisector(stack, fit_d, half_width, levels)
        t, best = timeit(lambda: ops.line_bisector(stack, fit_d, half_width, levels, out=bis))
        a = read + n * ih * 8 * k
        print('    line_bisector K=%d: %.1f us median %.1f best (%.1f MB, %.2f of 8 TB/s) = %.2fx line_profile; chords valid %.3f'
              % (k, t * 1e6, best * 1e6, a / 1e6, a / t / PEAK, t / t_prof, float(torch.isfinite(bis[k:]).float().mean())), flush=True)
        if k == 4:
            out = bis
    return out


def finish_bisector(raw, half_width):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    planes, h, w = raw.shape
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(0.05, 1.1, h, w)
    circle = (out_w / 2.0, out_h / 2.0, 0.42 * out_h)
    crop, _ = crop_plan(out_h, out_w, circle, dict(SHG_MAIN.default_options(), crop_width_square=True))
    args = (raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, circle, crop, half_width, 2.0)
    ops.line_bisector_finish(*args)
    med, best = timeit(lambda: ops.line_bisector_finish(*args))
    nw = crop[0]
    alg = planes * (out_h * nw * (4 + 2) + h * w * 4)
    print('line_bisector_finish %d x %dx%d -> %dx%d (circle, square crop, display planes): %.1f us median %.1f best; algorithmic '
          '%.1f MB -> %.2f TB/s (includes the output allocations)' % (planes, h, w, out_h, nw, med * 1e6, best * 1e6, alg / 1e6,
                                                                       alg / med / 1e12))


if __name__ == '__main__':
    c2 = None
    for hw in (5, 12):
        c2 = case(2000, 2000, 200, 16, hw)
        case(2000, 2000, 200, 8, hw)
        case(4000, 2560, 256, 16, hw)
    finish_bisector(c2, 12)
