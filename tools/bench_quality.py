"""Time the quality ranking's two calls in one process on C2-sized products (2000 x 2000): shg_patch_sharpness_u16 on the default
lattice (step 16: 126 x 126 points, patches of 33 x 33, arm 3, a disk of 0.9 R), and shg_stack_combine_weighted_u16 against
shg_stack_combine_field_u16 on the same inputs for N = 8 and 32 disks under mean and sigma -- every source but the first with a
smooth field of up to 1.5 px, every source with a lucky-region lattice that keeps it at about half of the nodes.  Every buffer is
allocated once; each call is timed two ways, as tools/bench_stack.py does: HIP events around single calls (median; includes the
launch) and a train of 30 calls between two events (the rate the stream sustains).  The weighted combine is reported as a ratio to
the field combine of the same run.  Each step runs under its own time limit (SIGALRM ends the process: nothing is started after a
step that hangs), and nothing is retried.

    python tools/bench_quality.py [--out profiles/quality_timings.txt]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_align import smooth_field  # noqa: E402
from bench_stack import SIZE, disk, limit, timeit  # noqa: E402
from solex_ser_recon_en_amd import _lib, ops, stack  # noqa: E402

STEP, PATCH, ARM = 16, 33, 3


def main(argv):
    lib, st = _lib.lib, ops._stream
    n_max = 32
    lines = ['bench_quality on %s, %d x %d disks; a single run on one MI355X' % (torch.cuda.get_device_name(0), SIZE, SIZE)]
    images = []
    for j in range(n_max):
        img, circle = disk(SIZE, j % 16)
        images.append(img)
    # ---- the sharpness ----
    gh, gw, points = stack.align_lattice((SIZE, SIZE), STEP)
    points_dev = torch.from_numpy(points).cuda()
    half = (PATCH - 1) // 2
    circle3 = np.ascontiguousarray([circle[0], circle[1], 0.9 * circle[2]], dtype=np.float64)
    table = torch.empty((gh * gw, 4), dtype=torch.int64, device='cuda')

    def sharpness():
        _lib.check(lib.shg_patch_sharpness_u16(images[0].data_ptr(), images[0].stride(0), SIZE, SIZE, points_dev.data_ptr(), gh * gw, half, ARM,
                                               circle3.ctypes.data, table.data_ptr(), st()), 'shg_patch_sharpness_u16')

    with limit():
        t = timeit(sharpness)
    host = table.cpu().numpy()
    lines.append('shg_patch_sharpness_u16: %d x %d = %d points at step %d, patches of %d x %d, arm %d, disk of 0.9 R; %d points with pixels, '
                 '%.1f M pixels in all: %8.1f us a call (median, events around one call)  %8.1f us in a train -> %.1f G pixels a second'
                 % (gh, gw, gh * gw, STEP, PATCH, PATCH, ARM, int((host[:, 0] > 0).sum()), host[:, 0].sum() / 1e6, t[0] * 1e6, t[1] * 1e6,
                    host[:, 0].sum() / t[1] / 1e9))
    # ---- the weighted combine against the field combine ----
    rng = np.random.default_rng(1)
    xf = np.ascontiguousarray([(1.0 + rng.uniform(-0.01, 0.01), rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(0.8, 1.2))
                               for _ in range(n_max)], dtype=np.float64)
    xf[0] = (1.0, 0.0, 0.0, 1.0)
    fields = [None] + [smooth_field(gh, gw, STEP, j) for j in range(1, n_max)]
    out = torch.empty((SIZE, SIZE), dtype=torch.uint16, device='cuda')
    count = torch.empty((SIZE, SIZE), dtype=torch.uint8, device='cuda')
    dims = np.ascontiguousarray([[SIZE, SIZE, t.stride(0)] for t in images], dtype=np.int64)
    lines.append('shg_stack_combine_weighted_u16 (lucky regions: the better half of the sources a node, by a random quality map a source) '
                 'against shg_stack_combine_field_u16 on the same sources, transforms and fields (%d x %d nodes); us a call (median) / us in a '
                 'train' % (gh, gw))
    for n in (8, 32):
        weights = [torch.from_numpy(w).cuda() for w in stack.quality_weights([rng.random((gh, gw)) for _ in range(n)], n // 2)]
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in images[:n]])
        fptrs = (ctypes.c_void_p * n)(*[None if f is None else f.data_ptr() for f in fields[:n]])
        wptrs = (ctypes.c_void_p * n)(*[w.data_ptr() for w in weights])
        for mode, code in (('mean', 0), ('sigma', 2)):
            def bent():
                _lib.check(lib.shg_stack_combine_field_u16(ptrs, dims.ctypes.data, xf.ctypes.data, fptrs, gh, gw, STEP, n, code, 2.5, 2,
                                                           out.data_ptr(), SIZE, SIZE, out.stride(0), count.data_ptr(), count.stride(0), st()),
                           'shg_stack_combine_field_u16')

            def lucky():
                _lib.check(lib.shg_stack_combine_weighted_u16(ptrs, dims.ctypes.data, xf.ctypes.data, fptrs, wptrs, gh, gw, STEP, n, code, 2.5,
                                                              2, out.data_ptr(), SIZE, SIZE, out.stride(0), count.data_ptr(), count.stride(0),
                                                              st()), 'shg_stack_combine_weighted_u16')

            with limit():
                a = timeit(bent)
            with limit():
                b = timeit(lucky)
            lines.append('  N = %2d %-6s with fields %8.1f / %8.1f   with fields and weights %8.1f / %8.1f   ratio in the train %.2f'
                         % (n, mode, a[0] * 1e6, a[1] * 1e6, b[0] * 1e6, b[1] * 1e6, b[1] / a[1]))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
