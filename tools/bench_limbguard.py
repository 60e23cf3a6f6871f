"""Time the limb protection in one process on a C2-sized product (2000 x 2000, circle (1000, 1000, 900)): shg_limb_split_u16 (both
planes: 2 bytes a pixel read, 4 written; the inner plane alone) and shg_limb_merge_u16 (with the sky plane: 6 read, 2 written;
without) beside device-to-device copies that move as many bytes, then deconvolve_disk (sigma 1.2, 10 iterations) and sharpen_disk
(default gains) as wholes, with and without limb=: the expectation is twice the filter plus the two launches.  Every buffer of the
two calls is allocated once; each call is timed two ways, as tools/bench_deconvolve.py does: HIP events around single calls (median;
includes the launches) and a train of 20 calls between two events (the rate the stream sustains).  Each step runs under its own time
limit (SIGALRM ends the process: nothing is started after a step that hangs), and nothing is retried.

    python tools/bench_limbguard.py [--out profiles/limbguard_timings.txt]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sharpen import SIZE, disk, limit, timeit  # noqa: E402
from solex_ser_recon_en_amd import _lib, deconvolve, ops, sharpen  # noqa: E402

CIRCLE = (1000.0, 1000.0, 900.0)
MARGIN, BLEND, REACH = 6.0, 4.0, 32.0
TRAIN = 20


def main(argv):
    lib, st = _lib.lib, ops._stream
    lines = ['bench_limbguard on %s, a %d x %d disk, circle %s, margin %g, blend %g, reach %g (one run)'
             % (torch.cuda.get_device_name(0), SIZE, SIZE, CIRCLE, MARGIN, BLEND, REACH)]
    img, _ = disk(SIZE, 0)
    inner, outer, out = (torch.empty((SIZE, SIZE), dtype=torch.uint16, device='cuda') for _ in range(3))
    circle = np.ascontiguousarray(CIRCLE, dtype=np.float64)
    pixels = SIZE * SIZE
    copies = {}
    for moved in (4, 6, 8):                                          # bytes a pixel: half read, half written
        src = torch.empty(moved // 2 * pixels, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        with limit():
            copies[moved] = timeit(lambda: dst.copy_(src), iters=TRAIN)
        lines.append('device-to-device copy moving %d bytes a pixel (%.0f MB): %8.1f us a call, %8.1f us in a train -> %.3f TB/s'
                     % (moved, moved * pixels / 1e6, copies[moved][0] * 1e6, copies[moved][1] * 1e6, moved * pixels / copies[moved][1] / 1e12))

    def split(want_outer):
        _lib.check(lib.shg_limb_split_u16(img.data_ptr(), SIZE, SIZE, img.stride(0), circle.ctypes.data, MARGIN, REACH, inner.data_ptr(), SIZE,
                                          outer.data_ptr() if want_outer else None, SIZE, st()), 'shg_limb_split_u16')

    def merge(with_sky):
        _lib.check(lib.shg_limb_merge_u16(img.data_ptr(), img.stride(0), inner.data_ptr(), SIZE, outer.data_ptr() if with_sky else None, SIZE,
                                          SIZE, SIZE, circle.ctypes.data, MARGIN, BLEND, out.data_ptr(), SIZE, st()), 'shg_limb_merge_u16')

    for name, fn, moved in (('shg_limb_split_u16, both planes', lambda: split(True), 6), ('shg_limb_split_u16, the inner plane', lambda: split(False), 4),
                            ('shg_limb_merge_u16, with the sky plane', lambda: merge(True), 8), ('shg_limb_merge_u16, without', lambda: merge(False), 6)):
        with limit():
            t = timeit(fn, iters=TRAIN)
        lines.append('%-40s %8.1f us a call (median, events around one call)  %8.1f us in a train -> %6.1f GB/s of its %d bytes a pixel, '
                     '%5.2f of the copy\'s time' % (name + ':', t[0] * 1e6, t[1] * 1e6, moved * pixels / t[1] / 1e9, moved, t[1] / copies[moved][1]))
    limb = {'circle': CIRCLE, 'margin': MARGIN, 'blend': BLEND, 'reach': REACH}
    sigma = sharpen.estimate_sigma(img, CIRCLE)[0]
    wholes = (('deconvolve_disk sigma 1.2, 10 iterations', lambda how: deconvolve.deconvolve_disk(img, 1.2, 10, limb=how)),
              ('sharpen_disk, default gains, sigma given', lambda how: sharpen.sharpen_disk(img, sharpen.DEFAULT_GAINS, sharpen.DEFAULT_DENOISE, sigma, limb=how)))
    for name, fn in wholes:
        took = {}
        for tag, how in (('plain', None), ('limb', limb), ('disk only', dict(limb, sky=False))):
            with limit():
                took[tag] = timeit(lambda: fn(how), iters=TRAIN, warmup=3)
        lines.append('%-42s plain %8.1f us a call %8.1f us in a train; limb= %8.1f / %8.1f (%.2f of plain); sky False %8.1f / %8.1f (%.2f) '
                     '(the Python call, its allocations included)'
                     % (name + ':', took['plain'][0] * 1e6, took['plain'][1] * 1e6, took['limb'][0] * 1e6, took['limb'][1] * 1e6,
                        took['limb'][1] / took['plain'][1], took['disk only'][0] * 1e6, took['disk only'][1] * 1e6,
                        took['disk only'][1] / took['plain'][1]))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
