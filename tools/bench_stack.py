"""Time the stacking's two calls in one process on C2-sized products (2000 x 2000): shg_stack_combine_u16 for N = 4, 8 and 16 disks
in each mode, beside a device-to-device copy of its algorithmic bytes (N reads plus one write of 2 B a pixel; the count plane's
1 B a pixel is on top), and shg_shift_ssd_u16 for S = 8 with a disk of 0.9 R (algorithmic: both images read once).  Every buffer is
allocated once; each call is timed two ways, as tools/bench_flatten.py does: HIP events around single calls (median; includes the
launches) and a train of calls between two events (the rate the stream sustains).  Each step runs under its own time limit (SIGALRM
ends the process: nothing is started after a step that hangs), and nothing is retried.

    python tools/bench_stack.py [--out profiles/stack_timings.txt]
"""
import contextlib
import ctypes
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import _lib, ops  # noqa: E402

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
    n_max = 16
    lines = ['bench_stack on %s, %d x %d disks' % (torch.cuda.get_device_name(0), SIZE, SIZE)]
    images = []
    for j in range(n_max):
        img, circle = disk(SIZE, j)
        images.append(img)
    rng = np.random.default_rng(1)
    # scales within a per cent, offsets within three pixels, gains within a fifth: what a series of scans gives
    xf = np.ascontiguousarray([(1.0 + rng.uniform(-0.01, 0.01), rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0.8, 1.2))
                               for _ in range(n_max)], dtype=np.float64)
    xf[0] = (1.0, 0.0, 0.0, 1.0)
    ptrs = (ctypes.c_void_p * n_max)(*[t.data_ptr() for t in images])
    dims = np.ascontiguousarray([[SIZE, SIZE, t.stride(0)] for t in images], dtype=np.int64)
    out = torch.empty((SIZE, SIZE), dtype=torch.uint16, device='cuda')
    count = torch.empty((SIZE, SIZE), dtype=torch.uint8, device='cuda')
    plane = SIZE * SIZE * 2
    copy_src = torch.empty((n_max + 1) * plane // 2, dtype=torch.uint8, device='cuda')
    copy_dst = torch.empty_like(copy_src)
    for n in (4, 8, 16):
        alg = (n + 1) * plane
        half = alg // 2                                              # a copy of `half` bytes reads half and writes half: alg bytes moved

        def copy():
            copy_dst[:half].copy_(copy_src[:half])

        with limit():
            copied = timeit(copy)
        lines.append('N = %d: algorithmic %.1f MB; device-to-device copy moving as much: %8.1f us a call, %8.1f us in a train -> %.3f TB/s'
                     % (n, alg / 1e6, copied[0] * 1e6, copied[1] * 1e6, alg / copied[1] / 1e12))
        for mode, code in (('mean', 0), ('median', 1), ('sigma', 2)):
            def combine():
                _lib.check(lib.shg_stack_combine_u16(ptrs, dims.ctypes.data, xf.ctypes.data, n, code, 2.5, 2, out.data_ptr(), SIZE, SIZE,
                                                     out.stride(0), count.data_ptr(), count.stride(0), st()), 'shg_stack_combine_u16')

            with limit():
                t = timeit(combine)
            lines.append('  shg_stack_combine_u16 %-6s %8.1f us a call (median, events around one call)  %8.1f us in a train -> %6.1f GB/s '
                         'in the train, %.2f of the copy\'s time' % (mode, t[0] * 1e6, t[1] * 1e6, alg / t[1] / 1e9, t[1] / copied[1]))
    circle3 = np.ascontiguousarray([circle[0], circle[1], 0.9 * circle[2]], dtype=np.float64)
    table = torch.empty(17 * 17 + 1, dtype=torch.int64, device='cuda')
    for search in (8, 2):
        def ssd():
            _lib.check(lib.shg_shift_ssd_u16(images[0].data_ptr(), images[0].stride(0), images[1].data_ptr(), images[1].stride(0), SIZE, SIZE,
                                             search, circle3.ctypes.data, table.data_ptr(), st()), 'shg_shift_ssd_u16')

        with limit():
            t = timeit(ssd)
        lines.append('shg_shift_ssd_u16 S = %d (%d offsets, disk of 0.9 R): %8.1f us a call  %8.1f us in a train -> %6.1f GB/s of its %.1f MB, '
                     '%.1f G differences a second' % (search, (2 * search + 1) ** 2, t[0] * 1e6, t[1] * 1e6, 2 * plane / t[1] / 1e9,
                                                      2 * plane / 1e6, int(table[(2 * search + 1) ** 2]) * (2 * search + 1) ** 2 / t[1] / 1e9))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
