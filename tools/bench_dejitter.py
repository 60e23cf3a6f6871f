"""Time the two calls of the dejitter stage in one process on a C2-sized raw disk (2000 x 2000): shg_column_limb_u16 (one plane: 2
bytes a pixel read, 24 bytes a column written) and shg_column_shift_u16 for one plane and for 21 planes (2 bytes a pixel read, 2
written), beside a device-to-device copy of the same bytes.  Every buffer is allocated once; each call is timed two ways, as
tools/bench_flatten.py does: HIP events around single calls (median; includes the launches) and a train of calls between two
events (the rate the stream sustains).  Each step runs under its own time limit (SIGALRM ends the process: nothing is started after
a step that hangs), and nothing is retried.  The results are checked against each other once before anything is timed: the shift
with the measured jitter straightens the midpoints.

    python tools/bench_dejitter.py [--out profiles/dejitter_timings.txt]
"""
import contextlib
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import _lib, dejitter, ops  # noqa: E402

STEP_SECONDS = 60
SIZE = 2000
PLANES = 21
WINDOW = 5


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


def raw_disk(n, seed):
    """An n x n raw-disk-like image: a limb-darkened ellipse with noise, every column moved by a whole-row-and-a-fraction jitter
    (linear between rows: the bench needs plausible data, not the accuracy scene) -> (the device image, the jitter)."""
    rng = np.random.default_rng(seed)
    jitter = rng.normal(0.0, 0.8, n)
    y = np.arange(n, dtype=np.float64)[:, None] - jitter[None, :]
    x = np.arange(n, dtype=np.float64)[None, :]
    r2 = ((x - (n / 2.0 + 0.3)) / (0.42 * n)) ** 2 + ((y - (n / 2.0 - 0.4) - 0.02 * (x - n / 2.0)) / (0.45 * n)) ** 2
    edge = np.clip((1.0 - r2) * 0.225 * n / 2.0 + 0.5, 0.0, 1.0)             # about two rows of limb
    img = 0.01 + edge * 0.6 * (0.35 + 0.65 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))) + 0.004 * rng.standard_normal((n, n))
    img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
    return torch.from_numpy(img.view(np.int16)).cuda().view(torch.uint16), jitter


def main(argv):
    lib, st = _lib.lib, ops._stream
    n = SIZE
    lines = ['bench_dejitter on %s, a %d x %d raw disk, window %d, first measurements (one run, no time bar was fixed in advance)'
             % (torch.cuda.get_device_name(0), n, n, WINDOW)]
    img, planted = raw_disk(n, 1)
    with limit():
        rec = dejitter.measure(img, window=WINDOW)
        again = dejitter.measure(dejitter.apply(img, rec['shift']), threshold=rec['threshold'], window=WINDOW)
        torch.cuda.synchronize()
    lines.append('  measured %d of %d columns at T = %d: %.3f px rms about the line (%.3f planted), %.3f after the shift'
                 % (rec['n_measured'], n, rec['threshold'], rec['rms'], float(np.sqrt(np.mean(planted ** 2))), again['rms']))
    offset, weight = dejitter.weights(rec['shift'])
    table = torch.empty((n, 6), dtype=torch.int32, device='cuda')
    stack = img[None].repeat(PLANES, 1, 1).contiguous()
    out = torch.empty_like(stack)
    threshold = rec['threshold']

    def limb():
        _lib.check(lib.shg_column_limb_u16(img.data_ptr(), n, n, img.stride(0), WINDOW, threshold, table.data_ptr(), st()), 'shg_column_limb_u16')

    def shift(planes):
        def call():
            _lib.check(lib.shg_column_shift_u16(stack.data_ptr(), planes, n, n, stack.stride(1), stack.stride(0), offset.ctypes.data,
                                                weight.ctypes.data, out.data_ptr(), out.stride(1), out.stride(0), st()), 'shg_column_shift_u16')
        return call

    def copy(planes):
        return lambda: out[:planes].copy_(stack[:planes])

    rows = {}
    for name, fn, moved in (('device-to-device copy, 1 plane', copy(1), 4 * n * n), ('shg_column_limb_u16', limb, 2 * n * n + 24 * n),
                            ('shg_column_shift_u16, 1 plane', shift(1), 4 * n * n),
                            ('device-to-device copy, %d planes' % PLANES, copy(PLANES), 4 * n * n * PLANES),
                            ('shg_column_shift_u16, %d planes' % PLANES, shift(PLANES), 4 * n * n * PLANES)):
        with limit():
            rows[name] = timeit(fn)
        lines.append('  %-36s %8.1f us a call (median, events around one call)  %8.1f us in a train  algorithmic %6.1f MB -> %.3f TB/s in the train'
                     % (name, rows[name][0] * 1e6, rows[name][1] * 1e6, moved / 1e6, moved / rows[name][1] / 1e12))
    for a, b in (('shg_column_limb_u16', 'device-to-device copy, 1 plane'), ('shg_column_shift_u16, 1 plane', 'device-to-device copy, 1 plane'),
                 ('shg_column_shift_u16, %d planes' % PLANES, 'device-to-device copy, %d planes' % PLANES)):
        lines.append('  %s / %s: %.2f by single calls, %.2f in trains' % (a, b, rows[a][0] / rows[b][0], rows[a][1] / rows[b][1]))
    print('\n'.join(lines))
    if '--out' in argv:
        path = argv[argv.index('--out') + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main(sys.argv[1:])
