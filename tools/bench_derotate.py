"""Time shg_derotate_u16 in one process on a C2-sized disk (2000 x 2000, radius 900): six hours of differential rotation without and
with the limb-darkening table, and thirty minutes with it (the displacement a series really has), beside a device-to-device copy of
the same bytes (2 bytes a pixel read, 2 written).  Every buffer is allocated once; each call is timed two ways, as
tools/bench_dejitter.py does: HIP events around single calls (median; includes the launch) and a train of 50 calls between two events
(the rate the stream sustains).  Each step runs under its own time limit (SIGALRM ends the process: nothing is started after a step
that hangs), and nothing is retried.  Before anything is timed the result is checked once: a time difference of zero returns the
image, and there and back returns close to it.

    python tools/bench_derotate.py [--out profiles/derotate_timings.txt]
"""
import contextlib
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import _lib, derotate, ops  # noqa: E402

STEP_SECONDS = 60
SIZE = 2000
CIRCLE = (1000.3, 999.6, 900.4)
NORTH, B0 = 17.0, -5.2


@contextlib.contextmanager
def limit(seconds=STEP_SECONDS):
    """The step inside runs at most `seconds`: SIGALRM's default action ends the process."""
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


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


def disk_image(n, circle, seed):
    """An n x n limb-darkened disk with granulation-like noise (the bench needs plausible data, not the accuracy scene)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    r2 = ((x - circle[0]) ** 2 + (y - circle[1]) ** 2) / circle[2] ** 2
    img = np.where(r2 < 1.0, 0.6 * (0.4 + 0.6 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))), 0.01) + 0.004 * rng.standard_normal((n, n))
    img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
    return torch.from_numpy(img.view(np.int16)).cuda().view(torch.uint16)


def main(argv):
    lib, st = _lib.lib, ops._stream
    n = SIZE
    lines = ['bench_derotate on %s, a %d x %d disk of radius %.1f, first measurements (one run, no time bar was fixed in advance)'
             % (torch.cuda.get_device_name(0), n, n, CIRCLE[2])]
    img = disk_image(n, CIRCLE, 1)
    with limit():
        same, _ = derotate.derotate_disk(img, CIRCLE, 0.0, NORTH, B0)
        there, rec = derotate.derotate_disk(img, CIRCLE, 0.25, NORTH, B0)
        back, _ = derotate.derotate_disk(there, CIRCLE, -0.25, NORTH, B0)
        torch.cuda.synchronize()
    assert torch.equal(same.view(torch.int16), img.view(torch.int16))
    inner = torch.from_numpy(((np.mgrid[0:n, 0:n][1] - CIRCLE[0]) ** 2 + (np.mgrid[0:n, 0:n][0] - CIRCLE[1]) ** 2) < (0.9 * CIRCLE[2]) ** 2).cuda()
    diff = (back.to(torch.float64) - img.to(torch.float64))[inner]
    lines.append('  6 h: a = %.4f rad at the equator, the largest displacement %.1f px, %d pixels from behind the limb; there and back %.1f counts rms '
                 '(the noise of %.0f counts smoothed twice by the cubic)' % (rec['a_equator'], rec['max_px'], rec['behind_limb'],
                                                                            float(diff.pow(2).mean().sqrt()), 0.004 * 65535.0))
    matrix = np.ascontiguousarray(derotate.orientation(NORTH, B0)).reshape(-1)
    circle = np.array(CIRCLE)
    table = torch.from_numpy(rec['clv']).cuda()
    out = torch.empty_like(img)

    def call(hours, clv):
        rate = np.array(derotate.rates(hours / 24.0))

        def run():
            _lib.check(lib.shg_derotate_u16(img.data_ptr(), n, n, img.stride(0), circle.ctypes.data, matrix.ctypes.data, rate.ctypes.data,
                                            table.data_ptr() if clv else None, rec['rings'], out.data_ptr(), out.stride(0), st()), 'shg_derotate_u16')
        return run

    rows = {}
    copy = 'device-to-device copy'
    for name, fn in ((copy, lambda: out.copy_(img)), ('shg_derotate_u16, 6 h, no clv', call(6.0, False)),
                     ('shg_derotate_u16, 6 h, clv', call(6.0, True)), ('shg_derotate_u16, 30 min, clv', call(0.5, True))):
        with limit():
            rows[name] = timeit(fn)
        moved = 4 * n * n
        lines.append('  %-32s %8.1f us a call (median, events around one call)  %8.1f us in a train  algorithmic %6.1f MB -> %.3f TB/s in the train'
                     % (name, rows[name][0] * 1e6, rows[name][1] * 1e6, moved / 1e6, moved / rows[name][1] / 1e12))
    for name in rows:
        if name != copy:
            lines.append('  %s / %s: %.2f by single calls, %.2f in trains' % (name, copy, rows[name][0] / rows[copy][0], rows[name][1] / rows[copy][1]))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
