"""What does a packet between two passes cost the frame-pass lane?  N back-to-back launches of the real pass A (k_accumulate_vec over
a resident C2 stack) on one stream (shg_lane_packets_probe) with, between consecutive launches,
  (a) three hipEventRecord   -- the lane with the profiler on, before the events were bound to the dispatch
  (b) one hipEventRecord     -- the same lane without the profiler
  (c) nothing                -- the bare kernel-to-kernel period of one queue
  (d) nothing, start / stop events bound to every launch (hipExtLaunchKernel) -- the lane with the profiler on, now
  (e) nothing, a stop event alone bound to every launch -- the lane without the profiler, now
First record to last record over N, in ms per launch; for (d) also the kernel time the bound pairs report.
    python3 tools/lane_packets.py [launches] [rounds] [out.txt]"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solex_ser_recon_en_amd import _lib, ops, synth  # noqa: E402

launches = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None

stack = synth.synth_frames_torch(2000, 2000, 200, 16, seed=0, padded=True)
n, h, w, bpp = ops.stack_geometry(stack)
ws = torch.empty(_lib.lib.shg_accumulate_workspace_bytes(n, h, w, bpp), dtype=torch.uint8, device='cuda')
stream = torch.cuda.Stream()
torch.cuda.synchronize()


def probe(mode, profiler=False):
    _lib.profile_reset()
    _lib.profile_enable(profiler, only=('accumulate',))
    ms = ctypes.c_double(0.0)
    try:
        _lib.check(_lib.lib.shg_lane_packets_probe(stack.data_ptr(), n, h, w, bpp, ops.frame_stride(stack), ws.data_ptr(), ws.numel(), mode,
                                                   launches, stream.cuda_stream, ctypes.byref(ms)), 'shg_lane_packets_probe')
        kernel_ms = None
        if profiler:
            total, count = _lib.profile_get('accumulate')
            assert count == launches, (count, launches)
            kernel_ms = total / count
    finally:
        _lib.profile_enable(False)
        _lib.profile_reset()
    return ms.value, kernel_ms


cases = (('a: three records', 0, False), ('b: one record', 1, False), ('c: nothing', 2, False),
         ('d: bound start + stop', 3, True), ('e: bound stop alone', 3, False))
for _, mode, prof in cases:                                    # warm-up: code objects, the stack's pages
    probe(mode, prof)
got = {name: [] for name, _, _ in cases}
kernel = []
for _ in range(rounds):                                        # the cases alternate, round by round
    for name, mode, prof in cases:
        ms, k = probe(mode, prof)
        got[name].append(ms)
        if k is not None:
            kernel.append(k)
lines = ['lane packets: %d back-to-back k_accumulate_vec over %d x %d x %d u%d on one stream, %d rounds; ms per launch, median (min .. max)'
         % (launches, n, h, w, 8 * bpp, rounds)]
med = {}
for name, _, _ in cases:
    v = sorted(got[name])
    med[name[0]] = v[len(v) // 2]
    lines.append('  %-24s %.4f  (%.4f .. %.4f)' % (name, v[len(v) // 2], v[0], v[-1]))
kernel.sort()
lines.append('  kernel time by the bound pairs of (d): %.4f ms median (%.4f .. %.4f)' % (kernel[len(kernel) // 2], kernel[0], kernel[-1]))
lines.append('  per record: (a - c) / 3 = %.2f us, b - c = %.2f us;  d - c = %.2f us, e - c = %.2f us;  a - d = %.2f us of a - c = %.2f us'
             % ((med['a'] - med['c']) / 3 * 1e3, (med['b'] - med['c']) * 1e3, (med['d'] - med['c']) * 1e3, (med['e'] - med['c']) * 1e3,
                (med['a'] - med['d']) * 1e3, (med['a'] - med['c']) * 1e3))
text = '\n'.join(lines)
print(text)
if out_path:
    with open(out_path, 'w') as f:
        f.write(text + '\n')
