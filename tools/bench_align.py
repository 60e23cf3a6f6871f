"""Time the local alignment's two calls in one process on C2-sized products (2000 x 2000): shg_patch_ssd_u16 on the lattice of
step 16 (126 x 126 points) with patches of 33 x 33 and S = 4, over a disk of 0.9 R, and shg_stack_combine_field_u16 against
shg_stack_combine_u16 on the same inputs for N = 4, 8 and 16 disks in each mode -- every source but the first with a smooth field
of up to 1.5 px.  Every buffer is allocated once; each call is timed two ways, as tools/bench_stack.py does: HIP events around
single calls (median; includes the launch) and a train of 30 calls between two events (the rate the stream sustains).  The field
combine is reported as a ratio to the plain combine of the same run.  Each step runs under its own time limit (SIGALRM ends the
process: nothing is started after a step that hangs), and nothing is retried.

    python tools/bench_align.py [--out profiles/align_timings.txt]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_stack import SIZE, disk, limit, timeit  # noqa: E402
from solex_ser_recon_en_amd import _lib, ops, stack  # noqa: E402

STEP, PATCH, SEARCH = 16, 33, 4


def smooth_field(gh, gw, step, seed):
    """A field as a scan's seeing and drift give it: dx a sine along the rows, dy along the columns, 1.5 px, period 120 px."""
    rng = np.random.default_rng(seed)
    phi, psi = rng.uniform(0.0, 2.0 * np.pi, 2)
    r, c = np.arange(gh, dtype=np.float64)[:, None] * step, np.arange(gw, dtype=np.float64)[None, :] * step
    field = np.empty((gh, gw, 2), dtype=np.float64)
    field[:, :, 0] = 1.5 * np.sin(2.0 * np.pi * r / 120.0 + phi) + 0.0 * c
    field[:, :, 1] = 1.5 * np.cos(2.0 * np.pi * c / 120.0 + psi) + 0.0 * r
    return torch.from_numpy(field).cuda()


def main(argv):
    lib, st = _lib.lib, ops._stream
    n_max = 16
    lines = ['bench_align on %s, %d x %d disks' % (torch.cuda.get_device_name(0), SIZE, SIZE)]
    images = []
    for j in range(n_max):
        img, circle = disk(SIZE, j)
        images.append(img)
    # ---- the patch SSD ----
    gh, gw, points = stack.align_lattice((SIZE, SIZE), STEP)
    points_dev = torch.from_numpy(points).cuda()
    half, words = (PATCH - 1) // 2, (2 * SEARCH + 1) ** 2 + 3
    circle3 = np.ascontiguousarray([circle[0], circle[1], 0.9 * circle[2]], dtype=np.float64)
    table = torch.empty((gh * gw, words), dtype=torch.int64, device='cuda')

    def ssd():
        _lib.check(lib.shg_patch_ssd_u16(images[0].data_ptr(), images[0].stride(0), images[1].data_ptr(), images[1].stride(0), SIZE, SIZE,
                                         points_dev.data_ptr(), gh * gw, half, SEARCH, circle3.ctypes.data, table.data_ptr(), st()),
                   'shg_patch_ssd_u16')

    with limit():
        t = timeit(ssd)
    host = table.cpu().numpy()
    terms = int(host[:, words - 3].sum()) * (2 * SEARCH + 1) ** 2
    lines.append('shg_patch_ssd_u16: %d x %d = %d points at step %d, patches of %d x %d, S = %d (%d offsets), disk of 0.9 R; %d points '
                 'with pixels, %.1f M pixels in all: %8.1f us a call (median, events around one call)  %8.1f us in a train -> '
                 '%.1f G differences a second' % (gh, gw, gh * gw, STEP, PATCH, PATCH, SEARCH, (2 * SEARCH + 1) ** 2,
                                                  int((host[:, words - 3] > 0).sum()), host[:, words - 3].sum() / 1e6, t[0] * 1e6, t[1] * 1e6,
                                                  terms / t[1] / 1e9))
    # ---- the combine with fields against the plain combine ----
    rng = np.random.default_rng(1)
    xf = np.ascontiguousarray([(1.0 + rng.uniform(-0.01, 0.01), rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0.8, 1.2))
                               for _ in range(n_max)], dtype=np.float64)
    xf[0] = (1.0, 0.0, 0.0, 1.0)
    fields = [None] + [smooth_field(gh, gw, STEP, j) for j in range(1, n_max)]
    ptrs = (ctypes.c_void_p * n_max)(*[t.data_ptr() for t in images])
    fptrs = (ctypes.c_void_p * n_max)(*[None if f is None else f.data_ptr() for f in fields])
    dims = np.ascontiguousarray([[SIZE, SIZE, t.stride(0)] for t in images], dtype=np.int64)
    out = torch.empty((SIZE, SIZE), dtype=torch.uint16, device='cuda')
    count = torch.empty((SIZE, SIZE), dtype=torch.uint8, device='cuda')
    lines.append('shg_stack_combine_field_u16 (every source but the first with a field of %d x %d nodes) against shg_stack_combine_u16 on the '
                 'same sources and transforms; us a call (median) / us in a train' % (gh, gw))
    for n in (4, 8, 16):
        for mode, code in (('mean', 0), ('median', 1), ('sigma', 2)):
            def plain():
                _lib.check(lib.shg_stack_combine_u16(ptrs, dims.ctypes.data, xf.ctypes.data, n, code, 2.5, 2, out.data_ptr(), SIZE, SIZE,
                                                     out.stride(0), count.data_ptr(), count.stride(0), st()), 'shg_stack_combine_u16')

            def bent():
                _lib.check(lib.shg_stack_combine_field_u16(ptrs, dims.ctypes.data, xf.ctypes.data, fptrs, gh, gw, STEP, n, code, 2.5, 2,
                                                           out.data_ptr(), SIZE, SIZE, out.stride(0), count.data_ptr(), count.stride(0), st()),
                           'shg_stack_combine_field_u16')

            with limit():
                a = timeit(plain)
            with limit():
                b = timeit(bent)
            lines.append('  N = %2d %-6s plain %8.1f / %8.1f   with fields %8.1f / %8.1f   ratio in the train %.2f'
                         % (n, mode, a[0] * 1e6, a[1] * 1e6, b[0] * 1e6, b[1] * 1e6, b[1] / a[1]))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
