"""Time shg_rl_deconvolve_u16 in one process on a C2-sized product (2000 x 2000): Gaussian blurs of sigma 1.2 (radius 5) and 2.5
(radius 10), 10 and 30 iterations, beside a device-to-device copy of the bytes one iteration moves (the forward launch reads e and
the image and writes q, the adjoint launch reads q and e and writes e: 22 bytes a pixel, 88 MB; the copy reads 44 MB and writes
44 MB).  Every buffer is allocated once; each call is timed two ways, as tools/bench_sharpen.py does: HIP events around single calls
(median; includes the launches) and a train of calls between two events (the rate the stream sustains).  Each step runs under its
own time limit (SIGALRM ends the process: nothing is started after a step that hangs), and nothing is retried.

    python tools/bench_deconvolve.py [--out profiles/deconvolve_timings.txt]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sharpen import SIZE, disk, limit, timeit  # noqa: E402
from solex_ser_recon_en_amd import _lib, deconvolve, ops  # noqa: E402

BYTES_A_PIXEL = 22                                   # one iteration: 14 read, 8 written


def main(argv):
    lib, st = _lib.lib, ops._stream
    lines = ['bench_deconvolve on %s, a %d x %d disk (one run)' % (torch.cuda.get_device_name(0), SIZE, SIZE)]
    img, _ = disk(SIZE, 0)
    out = torch.empty((SIZE, SIZE), dtype=torch.uint16, device='cuda')
    need = lib.shg_rl_workspace_bytes(SIZE, SIZE)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    moved = BYTES_A_PIXEL * SIZE * SIZE
    copy_src = torch.empty(moved // 2, dtype=torch.uint8, device='cuda')
    copy_dst = torch.empty_like(copy_src)

    def copy():
        copy_dst.copy_(copy_src)

    with limit():
        copied = timeit(copy)
    lines.append('one iteration moves %.1f MB (14 bytes a pixel read, 8 written); device-to-device copy moving as much: %8.1f us a call, '
                 '%8.1f us in a train -> %.3f TB/s' % (moved / 1e6, copied[0] * 1e6, copied[1] * 1e6, moved / copied[1] / 1e12))
    for sigma in (1.2, 2.5):
        taps = deconvolve.gaussian_taps(sigma)
        radius = taps.size // 2
        for iterations in (10, 30):
            def run():
                _lib.check(lib.shg_rl_deconvolve_u16(img.data_ptr(), SIZE, SIZE, img.stride(0), taps.ctypes.data, radius, iterations,
                                                     out.data_ptr(), out.stride(0), None, ws.data_ptr(), need, st()), 'shg_rl_deconvolve_u16')

            with limit():
                t = timeit(run, iters=20, warmup=3)
            lines.append('shg_rl_deconvolve_u16 sigma %.1f (radius %2d) %2d iterations: %9.1f us a call (median, events around one call)  '
                         '%9.1f us in a train -> %7.1f us an iteration, %5.2f of the copy\'s time, %6.1f GB/s of the bytes moved'
                         % (sigma, radius, iterations, t[0] * 1e6, t[1] * 1e6, t[1] / iterations * 1e6, t[1] / iterations / copied[1],
                            moved * iterations / t[1] / 1e9))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
