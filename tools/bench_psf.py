"""Time the blur measurement in one process on a C2-sized product (2000 x 2000, circle (1000, 1000, 900)): shg_limb_profile_u16
(reach 12, sub 4, 32 sectors: one read of the annulus's tiles, 2 bytes a pixel of the image at most) beside a device-to-device copy
of the image's bytes, then shg_rl_deconvolve_xy_u16 beside shg_rl_deconvolve_u16 at equal taps (sigma 1.2, radius 5, 10
iterations) and at the widths an anisotropic blur gives (1.0 and 2.0: radii 4 and 8), and psf.estimate_psf as a whole with its
host fit.  Every buffer is allocated once; each call is timed two ways, as tools/bench_deconvolve.py does: HIP events around single
calls (median; includes the launches) and a train of 20 calls between two events (the rate the stream sustains).  Each step runs
under its own time limit (SIGALRM ends the process: nothing is started after a step that hangs), and nothing is retried.

    python tools/bench_psf.py [--out profiles/psf_timings.txt]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sharpen import SIZE, disk, limit, timeit  # noqa: E402
from solex_ser_recon_en_amd import _lib, deconvolve, ops, psf  # noqa: E402

CIRCLE = (1000.0, 1000.0, 900.0)
REACH, SUB, SECTORS = 12, 4, 32
ITERATIONS, TRAIN = 10, 20


def blurred(img, sigma=1.5):
    """The device image under a Gaussian of `sigma` pixels an axis, on the host: the synthetic disk is sampled at points and has no
    blur of its own to measure."""
    a = img.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.float64)
    r = int(np.ceil(4 * sigma))
    k = np.exp(-np.arange(-r, r + 1) ** 2 / (2.0 * sigma * sigma))
    k /= k.sum()
    for axis in (0, 1):
        a = sum(k[i] * np.roll(a, i - r, axis=axis) for i in range(2 * r + 1))
    return np.clip(np.rint(a), 0, 65535).astype(np.uint16)


def main(argv):
    lib, st = _lib.lib, ops._stream
    lines = ['bench_psf on %s, a %d x %d disk, circle %s, reach %d, sub %d, %d sectors (one run)'
             % (torch.cuda.get_device_name(0), SIZE, SIZE, CIRCLE, REACH, SUB, SECTORS)]
    img, _ = disk(SIZE, 0)
    pixels = SIZE * SIZE
    src = torch.empty(2 * pixels, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    with limit():
        copy = timeit(lambda: dst.copy_(src), iters=TRAIN)
    lines.append('device-to-device copy of the image\'s bytes (%.0f MB):  %8.1f us a call, %8.1f us in a train' % (2 * pixels / 1e6, copy[0] * 1e6, copy[1] * 1e6))
    circle = np.ascontiguousarray(CIRCLE, dtype=np.float64)
    table = ops.sector_thresholds(SECTORS)
    shape = (SECTORS, 2 * REACH * SUB)
    count = torch.empty(shape, dtype=torch.uint32, device='cuda')
    total, sumsq = (torch.empty(shape, dtype=torch.uint64, device='cuda') for _ in range(2))

    def profile():
        _lib.check(lib.shg_limb_profile_u16(img.data_ptr(), SIZE, SIZE, img.stride(0), circle.ctypes.data, REACH, SUB, SECTORS, table.ctypes.data,
                                            count.data_ptr(), total.data_ptr(), sumsq.data_ptr(), st()), 'shg_limb_profile_u16')

    with limit():
        t = timeit(profile, iters=TRAIN)
    annulus = 2.0 * np.pi * CIRCLE[2] * 2 * REACH
    lines.append('shg_limb_profile_u16 (three clears, one launch):     %8.1f us a call (median, events around one call)  %8.1f us in a train: '
                 '%.2f of the copy\'s time; about %.0f pixels in the annulus' % (t[0] * 1e6, t[1] * 1e6, t[1] / copy[1], annulus))
    out = torch.empty((SIZE, SIZE), dtype=torch.uint16, device='cuda')
    need = lib.shg_rl_workspace_bytes(SIZE, SIZE)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')

    def one(k):
        _lib.check(lib.shg_rl_deconvolve_u16(img.data_ptr(), SIZE, SIZE, img.stride(0), k.ctypes.data, k.size // 2, ITERATIONS, out.data_ptr(), SIZE,
                                             None, ws.data_ptr(), need, st()), 'shg_rl_deconvolve_u16')

    def two(kx, ky):
        _lib.check(lib.shg_rl_deconvolve_xy_u16(img.data_ptr(), SIZE, SIZE, img.stride(0), kx.ctypes.data, kx.size // 2, ky.ctypes.data, ky.size // 2,
                                                ITERATIONS, out.data_ptr(), SIZE, None, ws.data_ptr(), need, st()), 'shg_rl_deconvolve_xy_u16')

    k = deconvolve.gaussian_taps(1.2)
    with limit():
        base = timeit(lambda: one(k), iters=TRAIN)
    with limit():
        same = timeit(lambda: two(k, k), iters=TRAIN)
    lines.append('shg_rl_deconvolve_u16, sigma 1.2, radius %d, %d iterations:     %8.1f us a call  %8.1f us in a train' % (k.size // 2, ITERATIONS, base[0] * 1e6, base[1] * 1e6))
    lines.append('shg_rl_deconvolve_xy_u16 at the same taps on both axes:         %8.1f us a call  %8.1f us in a train: %.3f of the one-set call'
                 % (same[0] * 1e6, same[1] * 1e6, same[1] / base[1]))
    kx, ky = deconvolve.gaussian_taps(1.0), deconvolve.gaussian_taps(2.0)
    with limit():
        wide = timeit(lambda: one(ky), iters=TRAIN)
    with limit():
        pair = timeit(lambda: two(kx, ky), iters=TRAIN)
    lines.append('shg_rl_deconvolve_u16, sigma 2.0, radius %d:                     %8.1f us a call  %8.1f us in a train' % (ky.size // 2, wide[0] * 1e6, wide[1] * 1e6))
    lines.append('shg_rl_deconvolve_xy_u16, sigma (1.0, 2.0), radii (%d, %d):       %8.1f us a call  %8.1f us in a train: %.3f of the one-set call at '
                 'the larger radius (the tile is sized by it)' % (kx.size // 2, ky.size // 2, pair[0] * 1e6, pair[1] * 1e6, pair[1] / wide[1]))
    soft = torch.from_numpy(np.ascontiguousarray(blurred(img)).view(np.int16)).cuda().view(torch.uint16)
    with limit():
        psf.estimate_psf(soft, CIRCLE)                               # (the bases are tabulated on the first call)
        torch.cuda.synchronize()
        began = time.perf_counter()
        est = psf.estimate_psf(soft, CIRCLE)
        whole = time.perf_counter() - began
    lines.append('psf.estimate_psf as a whole (the tables to the host, the fit of %d sectors, the regression): %.1f ms, %.1f ms of it the fit; '
                 'sigma (%.3f, %.3f) on %d sectors of a disk blurred by 1.5 px' % (SECTORS, whole * 1e3, est['fit_seconds'] * 1e3, est['sigma_x'], est['sigma_y'], est['n_used']))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
