"""Time the sharpening's two calls in one process on a C2-sized product (2000 x 2000): shg_wavelet_sharpen_u16 at 4 and 6 levels,
with and without the planes, and shg_wavelet_noise_u16 with a disk of 0.9 R, beside a device-to-device copy of the algorithmic
bytes (the image read once and written once: 16 MB; the noise call reads 8 MB).  Every buffer is allocated once; each call is timed
two ways, as tools/bench_stack.py does: HIP events around single calls (median; includes the launches) and a train of calls between
two events (the rate the stream sustains).  Each step runs under its own time limit (SIGALRM ends the process: nothing is started
after a step that hangs), and nothing is retried.

    python tools/bench_sharpen.py [--out profiles/sharpen_timings.txt]
"""
import contextlib
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import _lib, ops, sharpen  # noqa: E402

STEP_SECONDS = 60
SIZE = 2000


@contextlib.contextmanager
def limit(seconds=STEP_SECONDS):
    """The step inside runs at most `seconds`: SIGALRM's default action ends the process."""
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def timeit(fn, iters=30, warmup=5):
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


def disk(n, seed):
    """An n x n limb-darkened disk with noise (the synthetic scenes' law), its circle, on the device."""
    rng = np.random.default_rng(seed)
    circle = (n / 2.0 + 0.3, n / 2.0 - 0.4, 0.45 * n)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    r2 = ((x - circle[0]) ** 2 + (y - circle[1]) ** 2) / circle[2] ** 2
    img = np.where(r2 <= 1.0, 0.6 * (0.35 + 0.65 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))), 0.01) + 0.004 * rng.standard_normal((n, n))
    img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
    return torch.from_numpy(img.view(np.int16)).cuda().view(torch.uint16), circle


def main(argv):
    lib, st = _lib.lib, ops._stream
    lines = ['bench_sharpen on %s, a %d x %d disk' % (torch.cuda.get_device_name(0), SIZE, SIZE)]
    img, circle = disk(SIZE, 0)
    out = torch.empty((SIZE, SIZE), dtype=torch.uint16, device='cuda')
    planes = torch.empty((7, SIZE, SIZE), dtype=torch.int32, device='cuda')
    need = lib.shg_wavelet_workspace_bytes(SIZE, SIZE, 6)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    plane = SIZE * SIZE * 2
    alg = 2 * plane
    copy_src = torch.empty(plane, dtype=torch.uint8, device='cuda')
    copy_dst = torch.empty_like(copy_src)

    def copy():
        copy_dst.copy_(copy_src)                                     # reads 8 MB and writes 8 MB

    with limit():
        copied = timeit(copy)
    lines.append('algorithmic %.1f MB (one read and one write of the image); device-to-device copy moving as much: %8.1f us a call, %8.1f us '
                 'in a train -> %.3f TB/s (everything sits in the Infinity Cache: no HBM figure)'
                 % (alg / 1e6, copied[0] * 1e6, copied[1] * 1e6, alg / copied[1] / 1e12))
    sigma, _, _ = sharpen.estimate_sigma(img, circle)
    for levels in (4, 6):
        gain = np.ascontiguousarray(sharpen.quantise_gains(list(sharpen.DEFAULT_GAINS) + [1.0] * (levels - 4)), dtype=np.int32)
        thr = np.ascontiguousarray(sharpen.thresholds(sigma, sharpen.DEFAULT_DENOISE, levels), dtype=np.int32)
        for with_planes in (False, True):
            def run():
                _lib.check(lib.shg_wavelet_sharpen_u16(img.data_ptr(), SIZE, SIZE, img.stride(0), levels, gain.ctypes.data, thr.ctypes.data,
                                                       out.data_ptr(), out.stride(0), planes.data_ptr() if with_planes else None,
                                                       ws.data_ptr(), need, st()), 'shg_wavelet_sharpen_u16')

            with limit():
                t = timeit(run)
            lines.append('shg_wavelet_sharpen_u16 L = %d %-14s %8.1f us a call (median, events around one call)  %8.1f us in a train -> %6.1f GB/s '
                         'of the algorithmic bytes in the train, %.2f of the copy\'s time'
                         % (levels, 'with planes' if with_planes else 'without planes', t[0] * 1e6, t[1] * 1e6, alg / t[1] / 1e9, t[1] / copied[1]))
    circle3 = np.ascontiguousarray([circle[0], circle[1], 0.9 * circle[2]], dtype=np.float64)
    out2 = torch.empty(2, dtype=torch.int64, device='cuda')

    def noise():
        _lib.check(lib.shg_wavelet_noise_u16(img.data_ptr(), SIZE, SIZE, img.stride(0), circle3.ctypes.data, out2.data_ptr(), ws.data_ptr(),
                                             need, st()), 'shg_wavelet_noise_u16')

    with limit():
        t = timeit(noise)
    lines.append('shg_wavelet_noise_u16 (disk of 0.9 R, %d pixels, sigma %.1f counts): %8.1f us a call  %8.1f us in a train -> %6.1f GB/s of its '
                 '%.1f MB, %.2f of the copy\'s time' % (int(out2[1]), sigma, t[0] * 1e6, t[1] * 1e6, plane / t[1] / 1e9, plane / 1e6,
                                                         t[1] / copied[1]))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
