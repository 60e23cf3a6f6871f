"""Time the disk flattening's two calls beside their nearest yardsticks, in one process, on a C2-sized product (2000 x 2000) and on
a 500 x 500 one: shg_ring_medians_u16 against shg_select_u16 for two ranks on the same image (the whole-image radix select), and
shg_ring_flatten_u16 against shg_rescale_u16 on the same image (the streaming u16 -> u16 kernel).  Every buffer is allocated once;
each call is timed two ways, as tools/bench_detrend.py does: HIP events around single calls (median; includes the launches) and a
train of calls between two events (the rate the stream sustains).  Each step runs under its own time limit (SIGALRM ends the
process: nothing is started after a step that hangs), and nothing is retried.  Run it under rocprofv3 --kernel-trace --stats for
the kernels alone.  Algorithmic bytes: the medians read 2 B a pixel twice, the select once or twice; flatten and rescale read 2 B
and write 2 B a pixel.

    python tools/bench_flatten.py [--out profiles/flatten_timings.txt]
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


def disk(n, seed):
    """An n x n limb-darkened disk with noise (the synthetic scenes' law), its circle, on the device."""
    rng = np.random.default_rng(seed)
    circle = (n / 2.0 + 0.3, n / 2.0 - 0.4, 0.45 * n)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    r2 = ((x - circle[0]) ** 2 + (y - circle[1]) ** 2) / circle[2] ** 2
    img = np.where(r2 <= 1.0, 0.6 * (0.35 + 0.65 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))), 0.01) + 0.004 * rng.standard_normal((n, n))
    img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
    return torch.from_numpy(img.view(np.int16)).cuda().view(torch.uint16), circle


def bench(n, lines):
    lib, st = _lib.lib, ops._stream
    img, circle = disk(n, n)
    c3 = np.ascontiguousarray(circle, dtype=np.float64)
    k = int(np.floor(circle[2])) + 1
    count = torch.empty(k, dtype=torch.uint32, device='cuda')
    lo, hi = torch.empty(k, dtype=torch.uint16, device='cuda'), torch.empty(k, dtype=torch.uint16, device='cuda')
    ws_bytes = lib.shg_ring_medians_u16_workspace_bytes(k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    sel_bytes = lib.shg_select_u16_workspace_bytes(2)
    sel_ws = torch.empty(sel_bytes, dtype=torch.uint8, device='cuda')
    sel_out = torch.empty(2, dtype=torch.float64, device='cuda')
    ranks = (ctypes.c_int64 * 2)((n * n - 1) // 2, n * n // 2)
    out = torch.empty_like(img)
    pitch = img.stride(0)

    def medians():
        _lib.check(lib.shg_ring_medians_u16(img.data_ptr(), n, n, pitch, c3.ctypes.data, k, count.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                            ws.data_ptr(), ws_bytes, st()), 'shg_ring_medians_u16')

    def select():
        _lib.check(lib.shg_select_u16(img.data_ptr(), n, n, pitch, ranks, 2, sel_out.data_ptr(), sel_ws.data_ptr(), sel_bytes, st()),
                   'shg_select_u16')

    with limit():
        medians()
        torch.cuda.synchronize()
    med = (lo.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.float64) + hi.view(torch.int16).cpu().numpy().view(np.uint16)) / 2.0
    gain = np.minimum(np.median(med[:max(1, k // 10)]) / np.maximum(med, 1.0), 8.0)

    def flatten():
        _lib.check(lib.shg_ring_flatten_u16(img.data_ptr(), n, n, pitch, c3.ctypes.data, gain.ctypes.data, k, out.data_ptr(), out.stride(0),
                                            st()), 'shg_ring_flatten_u16')

    def rescale():
        _lib.check(lib.shg_rescale_u16(img.data_ptr(), n, n, pitch, 1000.0, 40000.0, 1.0, out.data_ptr(), out.stride(0), st()),
                   'shg_rescale_u16')

    rows = {}
    lines.append('%d x %d, K = %d rings (%d flatten launches), workspace %.1f MB' % (n, n, k, -(-k // 448), ws_bytes / 1e6))
    for name, fn, alg in (('shg_ring_medians_u16', medians, 4 * n * n), ('shg_select_u16 (2 ranks)', select, 2 * n * n),
                          ('shg_ring_flatten_u16', flatten, 4 * n * n), ('shg_rescale_u16', rescale, 4 * n * n)):
        with limit():
            rows[name] = timeit(fn)
        lines.append('  %-26s %8.1f us a call (median, events around one call)  %8.1f us in a train  algorithmic %5.1f MB -> %.3f TB/s in the train'
                     % (name, rows[name][0] * 1e6, rows[name][1] * 1e6, alg / 1e6, alg / rows[name][1] / 1e12))
    for a, b in (('shg_ring_medians_u16', 'shg_select_u16 (2 ranks)'), ('shg_ring_flatten_u16', 'shg_rescale_u16')):
        lines.append('  %s / %s: %.2f by single calls, %.2f in trains' % (a, b, rows[a][0] / rows[b][0], rows[a][1] / rows[b][1]))


def main(argv):
    lines = ['bench_flatten on %s' % torch.cuda.get_device_name(0)]
    for n in (2000, 500):
        bench(n, lines)
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
