"""The frame passes' events bound to their own dispatch (shg::launch_timed, csrc/shg_error.hip; the lane: csrc/streams.hip).
Nothing is recorded on the lane any more: the event a scan waits for and the profiler's start / stop pair travel with the kernel's
packet, and when both want the stop slot they share one event by a reference count.  What must hold: the profiler's samples are
still real kernel times on a serial lane, the products do not depend on the profiler, a profiler reset in the middle of a batch
costs no scan its event, and a pass nobody came to use gives its event back.
(No CPU-side test: events need the runtime, and a mock of it would test the mock.)"""
import ctypes
import os
import tempfile
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

N_SCANS = 12


@pytest.fixture(scope='module')
def pkg():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import SHG_MAIN, Solex_recon, _lib, ops, outputs, synth
    return SHG_MAIN, Solex_recon, _lib, ops, outputs, synth


@pytest.fixture(scope='module')
def stacks(pkg):
    synth = pkg[5]
    return [synth.synth_frames_torch(1000, 1000, 120, 16, seed=80 + i) for i in range(4)]


def run_batch(pkg, stacks, n, workers):
    """n scans (scan i over stacks[i mod len]) through the native pool -> per scan [(cc, protus), ...] as arrays"""
    SHG_MAIN, Solex_recon, _lib, ops, outputs, synth = pkg
    from solex_ser_recon_en_amd.video_reader import array_reader
    tasks = []
    for i in range(n):
        opts = SHG_MAIN.default_options()
        opts.update(_nolog=True)
        tasks.append((array_reader(stacks[i % len(stacks)]), opts))
    res = Solex_recon.solex_do_work(tasks, True, distribute='none', return_results=True, workers=workers)
    outputs.flush()
    torch.cuda.synchronize()
    return [[(np.asarray(cc), np.asarray(pr)) for cc, pr in per] for per in res]


def accumulate_spans(_lib):
    """(start, stop) in ms of every 'accumulate' sample since the last reset, by start time (shg_profile_dump)"""
    path = os.path.join(tempfile.gettempdir(), 'shg_lane_events_%d.csv' % os.getpid())
    try:
        _lib.check(_lib.lib.shg_profile_dump(path.encode()), 'shg_profile_dump')
        rows = [ln.split(',') for ln in open(path).read().splitlines()[1:]]
    finally:
        if os.path.exists(path):
            os.remove(path)
    return sorted((float(r[2]), float(r[3])) for r in rows if r[0] == 'accumulate')


def profiled(pkg, stacks, n, workers):
    _lib = pkg[2]
    _lib.profile_reset()
    _lib.profile_enable(True, only=('accumulate',))
    try:
        out = run_batch(pkg, stacks, n, workers)
    finally:
        _lib.profile_enable(False)
    spans = accumulate_spans(_lib)
    total_ms, launches = _lib.profile_get('accumulate')
    _lib.profile_reset()
    return out, spans, total_ms, launches


def test_samples_are_kernel_times_on_a_serial_lane_and_products_do_not_depend_on_the_profiler(pkg, stacks):
    """(1) 12 scans through a pool of four with the profiler on for 'accumulate': 12 samples, each as long as a pass of the same
    scans takes one scan at a time (that run's shortest x 0.5 to its longest x 3: kernel times, not zeros and not the batch), no
    two overlapping.  (2) The same batch with the profiler off gives the same products bit for bit."""
    run_batch(pkg, stacks, 4, 4)                                          # (first launches load code objects)
    _, serial_spans, _, serial_n = profiled(pkg, stacks, N_SCANS, 1)
    assert serial_n == N_SCANS and len(serial_spans) == N_SCANS
    serial = [b - a for a, b in serial_spans]
    print('serial pass A (ms):', ' '.join('%.4f' % d for d in serial))
    assert min(serial) > 0.0

    on, spans, total_ms, launches = profiled(pkg, stacks, N_SCANS, 4)
    dur = [b - a for a, b in spans]
    gaps = [spans[i + 1][0] - spans[i][1] for i in range(len(spans) - 1)]
    print('pooled pass A (ms):', ' '.join('%.4f' % d for d in dur))
    print('gaps on the lane (ms):', ' '.join('%.4f' % g for g in gaps))
    assert launches == N_SCANS and len(spans) == N_SCANS
    lo, hi = 0.5 * min(serial), 3.0 * max(serial)
    assert all(lo <= d <= hi for d in dur), (dur, lo, hi)
    assert abs(total_ms - sum(dur)) <= 1e-3 * N_SCANS                     # shg_profile_get and shg_profile_dump read the same events
    # the lane is serial: a pass starts after the one before it ended (the dump prints 0.1 us steps: two roundings of half a step)
    assert all(g >= -1e-4 for g in gaps), gaps

    off = run_batch(pkg, stacks, N_SCANS, 4)
    assert len(on) == len(off) == N_SCANS
    for a, b in zip(on, off):
        assert len(a) == len(b) and len(a) > 0
        for (c1, p1), (c2, p2) in zip(a, b):
            np.testing.assert_array_equal(c1, c2)
            np.testing.assert_array_equal(p1, p2)


def test_a_profiler_reset_in_the_middle_of_a_batch_costs_no_scan_its_event(pkg, stacks):
    """(3) Another thread resets the profiler over and over while a batch runs with it on: a scan's `done` event is the sample's b,
    and the reset lets go of the sample -- every scan must still get its pass (the batch completes, with the products of a quiet run)."""
    _lib = pkg[2]
    quiet = run_batch(pkg, stacks, N_SCANS, 4)
    stop = threading.Event()

    def resetter():
        while not stop.is_set():
            _lib.profile_reset()
            stop.wait(0.0002)
    got, failed = [], []

    def batches():
        try:
            for _ in range(3):
                got.append(run_batch(pkg, stacks, N_SCANS, 4))
        except BaseException as e:      # noqa: BLE001
            failed.append(repr(e))
    _lib.profile_reset()
    _lib.profile_enable(True, only=('accumulate', 'extract'))
    r = threading.Thread(target=resetter, daemon=True)
    w = threading.Thread(target=batches, daemon=True)
    try:
        r.start()
        w.start()
        w.join(120)
        hung = w.is_alive()
    finally:
        stop.set()
        r.join(10)
        _lib.profile_enable(False)
        _lib.profile_reset()
    assert not hung, 'a scan never got its pass'
    assert not failed, failed
    assert len(got) == 3
    for batch in got:
        for a, b in zip(batch, quiet):
            for (c1, p1), (c2, p2) in zip(a, b):
                np.testing.assert_array_equal(c1, c2)
                np.testing.assert_array_equal(p1, p2)


def test_a_pass_nobody_came_to_use_gives_its_event_back(pkg, stacks):
    """(4) 200 rounds of shg_pass_a_prelaunch + shg_pass_a_forget (a scan that failed before its first stage), half of them with the
    profiler on (the event is then shared with a sample) and a reset every tenth round.  The runtime shows no count of live events, so
    what is held is that all 200 complete and that the lane still serves a whole batch afterwards."""
    SHG_MAIN, Solex_recon, _lib, ops, outputs, synth = pkg
    run_batch(pkg, stacks, 2, 2)                                          # (makes the device's lane)
    assert _lib.lib.shg_frame_pass_lane_get()
    stack = stacks[0]
    n, h, w, bpp = ops.stack_geometry(stack)
    ws = torch.empty(_lib.lib.shg_accumulate_workspace_bytes(n, h, w, bpp), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    done = 0
    try:
        for i in range(200):
            if i % 100 == 0:
                _lib.profile_enable(i == 0, only=('accumulate',))
            assert ops.pass_a_prelaunch(stack, ws)
            _lib.check(_lib.lib.shg_pass_a_forget(ctypes.c_void_p(ws.data_ptr())), 'shg_pass_a_forget')
            if i % 10 == 9:
                _lib.profile_reset()
            done += 1
    finally:
        _lib.profile_enable(False)
        _lib.profile_reset()
    torch.cuda.synchronize()
    assert done == 200
    assert len(run_batch(pkg, stacks, N_SCANS, 4)) == N_SCANS
