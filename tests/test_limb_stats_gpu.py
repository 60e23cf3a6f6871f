"""The limb stage's statistics kernels -- the fused path (csrc/limb_fused.hip: shg_limb_prepare) and the one-kernel-per-call chain
(csrc/limb.hip, csrc/post.hip: shg_downscale_mean_u16, shg_box_blur_f64, shg_box_blur_key_f64, shg_select_keys_u32, shg_select_f64,
shg_select_multi_f64, shg_flood_stats_f64, shg_flood_stats_lerp_f64) -- each against the exact NumPy restatement of
tests/limb_stats_ref.py on its adversarial cases, bit for bit: integers as integers, float64 by their 64 bits.  Neither chain is
compared with the other.  tests/test_limb_stats_cpu.py holds the restatement to the oracle and shows the decision classes the cases
reach.

The empty flood.  For a constant disk nothing lies below the 99th percentile: data = blurred[blurred < very_bright] is empty and the
reference fails.  Both chains then give 20 zero counts and leave min / max as the float64 of their untouched accumulators' keys:
min = bits 0x7fffffffffffffff, max = bits 0xffffffffffffffff (two NaNs: EMPTY_MIN_BITS, EMPTY_MAX_BITS), and the host raises
ValueError on them (shg_host_flood_threshold) instead of building a threshold."""
import ctypes

import numpy as np
import pytest

from tests import limb_stats_ref as ref
from tests import pitched_util as pu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

EMPTY_MIN_BITS, EMPTY_MAX_BITS = 0x7fffffffffffffff, 0xffffffffffffffff
GUARD, GUARD_BYTES = 0xA5, 256
PLANTED = 7.25                        # what `packed` holds before a call that must refuse


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def reference():
    """name -> (case, limb_stats_ref.prepare of it): computed once, never changed."""
    out = {}
    for c in ref.cases():
        p = ref.prepare(c['disk'], c['k'])
        for v in p.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[c['name']] = (c, p)
    return out


CASE_NAMES = [c['name'] for c in ref.cases()]


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()              # (a copy: the reference's arrays are read-only)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


class Findings:
    """Every comparison of a test is made; the test fails at its end with the first differing element of each."""

    def __init__(self, tag):
        self.tag, self.failed, self.made = tag, [], 0

    def same(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.dtype == np.float64 or want.dtype == np.float64:
            got, want = bits(got), bits(want)
        self.made += 1
        if got.shape != want.shape:
            self.failed.append('%s %s: shape %r, reference %r' % (self.tag, what, got.shape, want.shape))
        elif not np.array_equal(got, want):
            bad = np.flatnonzero(got.ravel() != want.ravel())
            i = int(bad[0])
            self.failed.append('%s %s: %d of %d differ, first at %d: %r, reference %r' % (self.tag, what, bad.size, got.size, i, got.ravel()[i], want.ravel()[i]))

    def true(self, what, ok):
        self.made += 1
        if not ok:
            self.failed.append('%s %s' % (self.tag, what))

    def close(self):
        assert not self.failed, '%d of %d comparisons failed:\n%s' % (len(self.failed), self.made, '\n'.join(self.failed[:40]))


def placed(case):
    """The case's disk in its store: (store, view), the padding holding pitched_util.POISON (inside the range of a full-range image)."""
    pitch, col0 = ref.layout_args(case['layout'], case['disk'].shape[1])
    store, view = pu.pitched(case['disk'], pitch, pu.POISON, col0)
    vec = view.data_ptr() % 8 == 0 and view.stride(0) % 4 == 0
    assert vec == (case['layout'] == 'vec')
    return store, view


def want_stats(p):
    """(sum, min, max) as 64-bit patterns: the empty flood's sentinels where data is empty."""
    if p['mn'] is None:
        return np.array([bits([p['total']])[0], EMPTY_MIN_BITS, EMPTY_MAX_BITS], np.uint64)
    return bits([p['total'], p['mn'], p['mx']])


def check_packed(f, what, packed, p):
    got = packed.cpu().numpy()
    f.same(what + ' order statistics', got[0:4], p['order_stats'])
    f.same(what + ' sum, min, max', bits(got[4:7]), want_stats(p))
    f.same(what + ' counts', got[8:18].view(np.uint32).astype(np.int64), p['counts'])


def limb_prepare_guarded(view, k, ranks, gamma, short=0, shift=0):
    """shg_limb_prepare on a workspace this test owns: GUARD_BYTES of GUARD behind what shg_limb_prepare_workspace_bytes asks for
    (`short` bytes fewer handed over, the base moved by `shift` bytes), packed planted with PLANTED.
    -> (status, packed, keys pointer or None, workspace tensor, bytes asked for)."""
    from solex_ser_recon_en_amd._lib import lib
    from solex_ser_recon_en_amd import ops as _ops
    ptr, h, w, pitch = _ops._img(view, 'disk', torch.uint16)
    sh, sw = -(-h // 4), -(-w // 4)
    need = lib.shg_limb_prepare_workspace_bytes(sh, sw, int(k))
    room = need if need else 4096
    ws = torch.full((room + GUARD_BYTES + 8,), GUARD, dtype=torch.uint8, device=view.device)
    assert ws.data_ptr() % 8 == 0
    packed = torch.full((32,), PLANTED, dtype=torch.float64, device=view.device)
    rk = (ctypes.c_int64 * 4)(*[int(r) for r in ranks])
    keys_ptr = ctypes.c_void_p()
    torch.cuda.synchronize()
    status = lib.shg_limb_prepare(ptr, h, w, pitch, int(k), rk, float(gamma), packed.data_ptr(), ctypes.byref(keys_ptr), ws.data_ptr() + shift,
                                  room - short, _ops._stream())
    torch.cuda.synchronize()
    return status, packed, keys_ptr.value, ws, room


def run_fused(ops, f, what, case, p):
    store, view = placed(case)
    k = case['k']
    packed, keys, ws = ops.limb_prepare(view, k, p['ranks'], p['gamma'])
    torch.cuda.synchronize()
    f.same(what + ' keys', keys.cpu().numpy().view(np.uint32).astype(np.int64), p['Wk'])
    check_packed(f, what, packed, p)
    f.true(what + ' wrote into the disk\'s padding', pu.padding_untouched(store, view, pu.POISON))
    f.same(what + ' changed the disk', pu.view_to_host(view), case['disk'])
    # the same call on a workspace with a guard behind it
    status, packed2, keys_ptr, ws2, room = limb_prepare_guarded(view, k, p['ranks'], p['gamma'])
    f.same(what + ' status (guarded workspace)', status, 0)
    if status == 0:
        check_packed(f, what + ' (guarded workspace)', packed2, p)
        f.true(what + ' keys outside the workspace', ws2.data_ptr() <= keys_ptr and keys_ptr + 4 * p['Wk'].size <= ws2.data_ptr() + room)
        f.true(what + ' wrote behind its workspace', bool((ws2[room:] == GUARD).all().item()))


@pytest.mark.parametrize('name', CASE_NAMES)
def test_fused_path_equals_the_reference(ops, reference, name, monkeypatch):
    """ops.limb_prepare(disk, k, ranks, gamma) on every case: keys == Wk as integers, packed[0:4] == the four order statistics,
    packed[4:7] == sum, min, max (the empty flood's sentinels, above, where data is empty), the 20 counts; the disk's padding and
    a guard behind the workspace untouched.  The cases marked `fence` run again under SHG_LIMB_FENCE=1."""
    case, p = reference[name]
    f = Findings(name)
    monkeypatch.delenv('SHG_LIMB_FENCE', raising=False)
    run_fused(ops, f, 'fused', case, p)
    if case['fence']:
        monkeypatch.setenv('SHG_LIMB_FENCE', '1')
        run_fused(ops, f, 'fused, fence', case, p)
    f.close()


def run_separate(ops, f, disk, layout, k, p):
    """Each kernel of the one-kernel-per-call chain on the reference's own arrays (so that a failure names its kernel)."""
    store, view = placed(dict(disk=disk, layout=layout))
    small_ref = p['B'].astype(np.float64) * ref.UNIT
    f.same('downscale_mean_u16', ops.downscale_mean_u16(view, 4).cpu().numpy(), small_ref)
    f.true('downscale_mean_u16 wrote into the disk\'s padding', pu.padding_untouched(store, view, pu.POISON))
    small = dev(small_ref)
    planes = {}
    for kw, W, blur in ((k, p['Wk'], p['blur_k']), (5, p['W5'], p['blur_5'])):
        f.same('box_blur_f64 k=%d' % kw, ops.box_blur_f64(small, kw).cpu().numpy(), blur)
        if kw <= 63:
            got, keys = ops.box_blur_key_f64(small, kw)
            f.same('box_blur_key_f64 k=%d blurred' % kw, got.cpu().numpy(), blur)
            f.same('box_blur_key_f64 k=%d keys' % kw, keys.cpu().numpy().view(np.uint32).astype(np.int64), W)
        planes[kw] = dev(blur), dev(W.astype(np.uint32).view(np.int32))
    (blur_k, keys_k), (blur_5, keys_5) = planes[k], planes[5]
    ranks = p['ranks']
    f.same('select_keys_u32', ops.select_keys_u32([keys_5, keys_5, keys_k, keys_k], ranks, [5, 5, k, k]).cpu().numpy(), p['order_stats'])
    f.same('select_f64 blur 5', ops.select_f64(blur_5, ranks[0:2]).cpu().numpy(), p['order_stats'][0:2])
    f.same('select_f64 blur k', ops.select_f64(blur_k, ranks[2:4]).cpu().numpy(), p['order_stats'][2:4])
    f.same('select_multi_f64', ops.select_multi_f64([blur_5, blur_5, blur_k, blur_k], ranks).cpu().numpy(), p['order_stats'])
    for what, (stats, counts) in (('flood_stats', ops.flood_stats(small, blur_k, p['very_bright'])),
                                  ('flood_stats_lerp', ops.flood_stats_lerp(small, blur_k, dev(p['order_stats'][2:4]), p['gamma']))):
        f.same(what + ' sum, min, max', bits(stats.cpu().numpy()), want_stats(p))
        f.same(what + ' counts', counts.cpu().numpy().view(np.uint32).astype(np.int64), p['counts'])


@pytest.mark.parametrize('name', CASE_NAMES)
def test_separate_chain_equals_the_reference(ops, reference, name):
    """downscale_mean_u16 (in the case's layout, padding verified), box_blur_f64 and box_blur_key_f64 (windows k and 5),
    select_keys_u32, select_f64 and select_multi_f64 on the blurred planes, flood_stats and flood_stats_lerp: each against the
    restatement, none against the fused path.  The empty flood: the same sentinels as the fused path's (above)."""
    case, p = reference[name]
    f = Findings(name)
    run_separate(ops, f, case['disk'], case['layout'], case['k'], p)
    f.close()


@pytest.mark.parametrize('k', [17, 31, 63])
def test_windows_beyond_the_fused_path_go_through_the_separate_chain(ops, k):
    """k = 17 ... 63: refused by shg_limb_prepare (its tile holds a 16 x 16 window), served by the separate chain with 32-bit keys.
    A 19 x 23 quarter-size image: k = 63 folds its halo more than once."""
    from solex_ser_recon_en_amd._lib import lib
    rng = np.random.default_rng(k)
    disk = rng.integers(0, 65536, (75, 90)).astype(np.uint16)
    p = ref.prepare(disk, k)
    assert lib.shg_limb_fused_fits(19, 23, k) == 0 and lib.shg_limb_prepare_workspace_bytes(19, 23, k) == 0
    with pytest.raises(ValueError):
        ops.limb_prepare(dev(disk), k, p['ranks'], p['gamma'])
    f = Findings('k=%d' % k)
    run_separate(ops, f, disk, 'odd', k, p)
    f.close()


@pytest.mark.parametrize('n', [1, 777, 2048, 2049, 600001])
def test_select_multi_f64_against_a_sort(ops, n):
    """shg_select_multi_f64 itself: two arrays of different content (one with heavy ties, negative values, infinities and
    denormals; one continuous), eight (array, rank) pairs with different ranks each -- first, last, middle, inside and at both ends
    of a run of equal values -- against np.sort.  n = 2048 / 2049: one and two workgroups; 600001: the grid capped at 256."""
    rng = np.random.default_rng(n)
    a = np.round(rng.normal(0, 3, n)) + 0.0                       # (no -0.0: np.sort leaves the order of the two zeros open)
    a[rng.random(n) < 0.02] = np.inf
    a[rng.random(n) < 0.02] = -np.inf
    a[rng.random(n) < 0.05] = 5e-324
    a[rng.random(n) < 0.05] = -2.5e-310
    b = rng.normal(0, 1e-3, n) + np.where(rng.random(n) < 0.5, 1.0, -1e300)
    sa, sb = np.sort(a), np.sort(b)
    run = np.flatnonzero(sa == 1.0)                                # a run of ties in a (round(N(0, 3)) == 1), when n is not tiny
    first, last = (int(run[0]), int(run[-1])) if run.size else (0, n - 1)
    pairs = [(a, 0), (b, n - 1), (a, n // 2), (b, n // 3), (a, first), (a, last), (b, 0), (a, (first + last) // 2)]
    da, db = dev(a), dev(b)
    got = ops.select_multi_f64([da if arr is a else db for arr, _ in pairs], [r for _, r in pairs]).cpu().numpy()
    want = np.array([(sa if arr is a else sb)[r] for arr, r in pairs])
    f = Findings('n=%d' % n)
    f.same('select_multi_f64', got, want)
    f.same('select_multi_f64 changed its input', da.cpu().numpy(), a)
    f.close()


def test_refusals_launch_nothing(ops):
    """shg_limb_prepare refuses with the documented status -- SHG_E_UNSUPPORTED (-3) outside the fused path (k = 17, k = 0, sh <= 2),
    SHG_E_ARG (-1) for a rank equal to n, gamma outside [0, 1] and a workspace off 8 bytes, SHG_E_WORKSPACE (-2) for one a byte short
    -- and launches nothing: packed, the workspace (its head is zeroed by the first launch) and the guard are as planted."""
    rng = np.random.default_rng(7)
    disk = dev(rng.integers(0, 65536, (80, 90)).astype(np.uint16))           # 20 x 23
    n = 20 * 23
    ranks, gamma = ref.stage_ranks(n)
    flat = dev(rng.integers(0, 65536, (8, 90)).astype(np.uint16))            # sh = 2
    f = Findings('refusal')
    for what, want, view, k, rk, g, short, shift in (
            ('k = 17', -3, disk, 17, ranks, gamma, 0, 0),
            ('k = 0', -3, disk, 0, ranks, gamma, 0, 0),
            ('sh = 2', -3, flat, 1, [0, 0, 0, 0], 0.5, 0, 0),
            ('rank == n', -1, disk, 3, ranks[:3] + [n], gamma, 0, 0),
            ('median rank == n', -1, disk, 3, [n] + ranks[1:], gamma, 0, 0),
            ('gamma < 0', -1, disk, 3, ranks, -1e-9, 0, 0),
            ('gamma > 1', -1, disk, 3, ranks, 1.0000001, 0, 0),
            ('gamma nan', -1, disk, 3, ranks, float('nan'), 0, 0),
            ('workspace one byte short', -2, disk, 3, ranks, gamma, 1, 0),
            ('workspace off 8 bytes', -1, disk, 3, ranks, gamma, 0, 4)):
        status, packed, keys_ptr, ws, room = limb_prepare_guarded(view, k, rk, g, short, shift)
        f.same(what + ' status', status, want)
        f.true(what + ' wrote packed', bool((packed == PLANTED).all().item()))
        f.true(what + ' wrote the workspace', bool((ws == GUARD).all().item()))
        f.true(what + ' set keys_out', keys_ptr is None)
    # (and the same arguments without the fault are taken)
    status, packed, keys_ptr, ws, room = limb_prepare_guarded(disk, 3, ranks, gamma)
    f.same('accepted status', status, 0)
    f.true('accepted: packed written', bool((packed[:7] != PLANTED).all().item()))
    f.close()


@pytest.mark.parametrize('fused', ['1', '0'])
@pytest.mark.parametrize('value', [0, 12345, 65535])
def test_constant_disk_raises(ops, value, fused, monkeypatch):
    """A constant 400 x 40 disk (quarter size 100 x 10, k = 1) through the whole stage, both chains: data is empty, and the limb fit
    raises ValueError -- as the reference fails on such a disk -- instead of returning a circle built on a threshold computed from
    the empty flood's sentinels."""
    from solex_ser_recon_en_amd import stages
    monkeypatch.setenv('SHG_LIMB_FUSED', fused)
    monkeypatch.delenv('SHG_LIMB_FENCE', raising=False)
    disk = dev(np.full((400, 40), value, np.uint16))
    with pytest.raises(ValueError, match='99th percentile'):
        stages.limb_fit(disk)
    torch.cuda.synchronize()
