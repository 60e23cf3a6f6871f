"""Time the plane removal's two kernels beside shg_doppler_finish on the C2 map: a 2000 x 2000 raw map through the finish (limb
circle, square crop, display plane: tools/bench_lineprofile.py's geometry), then on the finished map shg_map_plane_moments without
and with a previous plane, shg_map_detrend with its display plane, and linemaps.detrend_plane as a whole (launches, 80-byte
readbacks and exact solves).  Each call is timed two ways: HIP events around single calls (median, includes the launch and the
wrapper's allocations) and a train of calls between two events (the rate the stream sustains).  Run it under
rocprofv3 --kernel-trace --stats for the kernels alone; --sweep also times the moments launch at several workgroup counts
(SHG_MOMENTS_GROUPS).  Algorithmic bytes: the moments read 4 B a pixel; the detrend reads 4 and writes 4 + 2."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import SHG_MAIN, linemaps, ops  # noqa: E402
from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry  # noqa: E402
from solex_ser_recon_en_amd.Solex_recon import crop_plan  # noqa: E402


def timeit(fn, iters=50, warmup=10):
    """(median of single calls between events, mean of a train of calls) in seconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    single = sorted(a.elapsed_time(b) for a, b in evs)[iters // 2] * 1e-3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return single, a.elapsed_time(b) * 1e-3 / iters


def main(sweep):
    rng = np.random.default_rng(0)
    h = w = 2000
    field = 1.5 * (2.0 * np.arange(w)[None, :] / (w - 1) - 1.0) + rng.normal(0.0, 0.1, (h, w))
    field[rng.random((h, w)) < 0.03] += 2.0
    raw = torch.from_numpy(field.astype(np.float32)).cuda()
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(0.05, 1.1, h, w)
    circle = (out_w / 2.0, out_h / 2.0, 0.42 * out_h)
    crop, circle_out = crop_plan(out_h, out_w, circle, dict(SHG_MAIN.default_options(), crop_width_square=True))
    fc = linemaps.finish_circle(circle, crop, circle_out)
    args = (raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, fc, crop, 2.0)
    m, _ = ops.doppler_finish(*args)
    mh, mw = m.shape
    own = (fc[0] - crop[1] + crop[2], fc[1], fc[2])                   # the circle in the map's own columns
    slots = torch.empty(10, dtype=torch.int64, device='cuda')
    out = torch.empty_like(m)
    a, b, g, sigma, n = linemaps.plane_from_moments(ops.map_plane_moments(m, own, None, slots).cpu().numpy())
    prev = (a, b, g, 3.0 * sigma)
    print('map %d x %d (pitch %d), %d pixels on the disk; pass 0: a %.4f b %.6f g %.6f sigma %.4f'
          % (mh, mw, m.stride(0), n, a, b, g, sigma))
    rows = []

    def report(name, fn, alg_bytes):
        single, train = timeit(fn)
        rows.append((name, single, train))
        print('%-34s %7.1f us a call (median, events around one call)  %7.1f us in a train  algorithmic %.1f MB -> %.2f TB/s in the train'
              % (name, single * 1e6, train * 1e6, alg_bytes / 1e6, alg_bytes / train / 1e12))

    report('doppler_finish', lambda: ops.doppler_finish(*args), h * w * 4 + mh * mw * 6)
    report('map_plane_moments (pass 0)', lambda: ops.map_plane_moments(m, own, None, slots), mh * mw * 4)
    report('map_plane_moments (clipped)', lambda: ops.map_plane_moments(m, own, prev, slots), mh * mw * 4)
    report('map_plane_moments (no circle)', lambda: ops.map_plane_moments(m, None, prev, slots), mh * mw * 4)
    report('map_detrend (display plane)', lambda: ops.map_detrend(m, (a, b, g), 2.0, out), mh * mw * 10)
    finish, moments = rows[0], rows[2]
    print('moments (clipped) / finish: %.2f by single calls, %.2f in trains' % (moments[1] / finish[1], moments[2] / finish[2]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        _, _, info = linemaps.detrend_plane(m, own, display_range=2.0)
    torch.cuda.synchronize()
    print('detrend_plane: %.1f us a call on the host clock (%d passes, %d of %d pixels used, b %.6f)'
          % ((time.perf_counter() - t0) / reps * 1e6, info['passes'], info['n_used'], info['n_valid'], info['b']))
    if sweep:
        for groups in (64, 128, 256, 512, 1024, 2048, 4096):
            os.environ['SHG_MOMENTS_GROUPS'] = str(groups)
            report('moments (clipped), %4d groups' % groups, lambda: ops.map_plane_moments(m, own, prev, slots), mh * mw * 4)
        del os.environ['SHG_MOMENTS_GROUPS']


if __name__ == '__main__':
    main('--sweep' in sys.argv[1:])
