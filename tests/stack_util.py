"""What the GPU tests of the stacking family (test_stack_gpu, test_align_gpu, test_quality_gpu) share: planted device buffers with odd
pitches and skewed base pointers, random sources, fields and weight lattices, the one driver of the three combine entry points and
the comparison against a restatement."""
import ctypes

import numpy as np
import pytest

from tests import align_ref as ar
from tests import stack_ref as sr

torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
PAD, OUT_FILL, COUNT_FILL, SSD_FILL = 0xBEEF, 0x5A5A, 0xA5, 0x7EADBEEF7EADBEEF
GUARD = 3                                   # planted words behind a table
MODES = ('mean', 'median', 'sigma')
MAX_SOURCES = 32

# the patch kernels' image and its special centres
H, W = 70, 90
SPECIAL = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),                       # the corners
           (0, 45), (35, 0), (H - 1, 44), (34, W - 1),                           # the edges
           (-1, -1), (-33, 45), (35, W + 32), (H, W), (1000, 1000), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31),    # outside
           (35, 45), (35, 45), (20, 30), (41, 52)]                               # inside, two of them equal
# the lattice combines' grids
GRIDS = [((1, 1), 'odd'), ((1, 7), 'odd'), ((9, 8), 'aligned'), ((37, 263), 'odd'), ((64, 256), 'aligned'), ((64, 256), 'skewed')]
LAYOUTS = {'aligned': dict(out_extra=0, count_extra=0), 'odd': dict(out_extra=1, count_extra=3), 'skewed': dict(out_extra=0, count_extra=0, skew=1)}


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops, stack
    from solex_ser_recon_en_amd._lib import lib
    return stack, ops, lib


def up16(a):
    return torch.from_numpy(np.array(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.uint16)


def down16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def skewed(img, extra, skew=1, fill=PAD):
    """img in a device buffer of pitch w + extra that starts `skew` elements into its allocation, everything else `fill` ->
    (the allocation, the image's address)."""
    h, w = img.shape
    buf = np.full(skew + h * (w + extra), fill, np.uint16)
    buf[skew:].reshape(h, w + extra)[:, :w] = img
    dev = up16(buf)
    return dev, dev.data_ptr() + 2 * skew


def padded(img, extra, fill=PAD):
    """img in a device buffer whose pitch is w + extra, the rest `fill` -> the buffer [h, w + extra]."""
    return skewed(img, extra, 0, fill)[0].reshape(img.shape[0], img.shape[1] + extra)


def void_array(values):
    return (ctypes.c_void_p * len(values))(*values)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def planted_table(words):
    """`words` 64-bit words and GUARD more behind them on the device, all SSD_FILL."""
    return torch.from_numpy(np.full(words + GUARD, SSD_FILL, np.uint64).view(np.int64)).cuda()


def circle3(circle):
    """The circle argument: a host float64 [3] array, or None for 'none'."""
    return None if circle == 'none' else np.ascontiguousarray([float(v) for v in circle], dtype=np.float64)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, '%d %s differ, first at %s: %d vs %d' % (len(bad), what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def random_sources(n, shapes, seed, spread=3.0, scale=0.03, gains=(0.8, 1.2)):
    """n sources, their shapes cycling through `shapes`: a common ramp plus noise and here and there an outlier, so that the clipping
    has something to clip, with transforms a few pixels and per cent apart."""
    rng = np.random.default_rng(seed)
    srcs, xforms = [], []
    for j in range(n):
        h, w = shapes[j % len(shapes)]
        img = 20000.0 + 150.0 * np.arange(w)[None, :] + 90.0 * np.arange(h)[:, None] + rng.normal(0.0, 300.0, (h, w))
        srcs.append(np.clip(img + (rng.random((h, w)) < 0.03) * 20000.0, 0, 65535).astype(np.uint16))
        xforms.append((1.0 + rng.uniform(-scale, scale), rng.uniform(-spread, spread), rng.uniform(-spread, spread), rng.uniform(*gains)))
    return srcs, xforms


def random_fields(n, shape, step, seed, size=3.0, none=()):
    rng = np.random.default_rng(seed)
    gh, gw = ar.lattice_shape(shape, step)
    return [None if j in none else rng.uniform(-size, size, (gh, gw, 2)) for j in range(n)]


def random_weights(n, shape, step, seed, none=(), top=2.0):
    rng = np.random.default_rng(seed)
    gh, gw = ar.lattice_shape(shape, step)
    return [None if j in none else rng.uniform(0.0, top, (gh, gw)) * (rng.random((gh, gw)) > 0.15) for j in range(n)]


def combine(lib, srcs, xforms, shape, fields=None, weights=None, step=None, mode='mean', kappa=2.5, iterations=2, out_extra=1, count_extra=3,
            skew=0, want_count=True, plain=False, **over):
    """The combine entry point that takes what is given -- weights: shg_stack_combine_weighted_u16 (fields may be None as a whole);
    else a step: shg_stack_combine_field_u16; else, or with plain, shg_stack_combine_u16 -- on the sources in padded buffers (pitch
    w + 1 + j % 3) into planted outputs that start `skew` elements into their buffers -> (status, out [oh, ow], count [oh, ow] or
    None, everything else intact).  The sources, the fields and the lattices are verified untouched.  over: arguments to pass
    instead (n, dims {j: row}, null_src, srcs_ptr, dims_ptr, xf_ptr, out, oh, ow, out_pitch, count, count_pitch, gh, gw,
    field_ptr {j: address}, weight_ptr {j: address}, no_fields, no_weights)."""
    oh, ow = shape
    n = over.pop('n', len(srcs))
    bufs = [padded(np.asarray(s, np.uint16), 1 + j % 3) for j, s in enumerate(srcs)]
    ptrs = void_array([b.data_ptr() for b in bufs] + [None] * (MAX_SOURCES - len(bufs)))
    dims = np.zeros((MAX_SOURCES, 3), np.int64)
    xf = np.zeros((MAX_SOURCES, 4), np.float64)
    for j, s in enumerate(srcs):
        dims[j] = (s.shape[0], s.shape[1], s.shape[1] + 1 + j % 3)
        xf[j] = xforms[j]
    for j, row in over.pop('dims', {}).items():
        dims[j] = row
    if 'null_src' in over:
        ptrs[over.pop('null_src')] = None
    lattice, planted = (), []                                                    # the lattice's arguments; (host, device) nodes to verify

    def node_ptrs(nodes, key):
        dev = [None if f is None else torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).cuda() for f in nodes]
        planted.extend(zip(nodes, dev))
        return void_array([over.get(key, {}).get(j, None if d is None else d.data_ptr()) for j, d in enumerate(dev)])

    fn = lib.shg_stack_combine_u16
    if step is not None and not plain:
        fn = lib.shg_stack_combine_field_u16 if weights is None else lib.shg_stack_combine_weighted_u16
        fptrs = None if fields is None else node_ptrs(fields, 'field_ptr')
        lattice = (None if over.get('no_fields') else fptrs,)
        if weights is not None:
            wptrs = node_ptrs(weights, 'weight_ptr')
            lattice += (None if over.get('no_weights') else wptrs,)
        gh, gw = ar.lattice_shape(shape, step) if 1 <= step else (1, 1)
        lattice += (over.get('gh', gh), over.get('gw', gw), step)
    out_pitch, count_pitch = ow + out_extra, ow + count_extra
    out = up16(np.full(oh * out_pitch + skew + 8, OUT_FILL))
    cnt = torch.full((oh * count_pitch + skew + 8,), COUNT_FILL, dtype=torch.uint8, device='cuda')
    st = fn(over.get('srcs_ptr', ptrs), over.get('dims_ptr', dims.ctypes.data), over.get('xf_ptr', xf.ctypes.data), *lattice, n,
            sr.MODES.get(mode, mode), kappa, iterations, over.get('out', out.data_ptr() + 2 * skew), over.get('oh', oh), over.get('ow', ow),
            over.get('out_pitch', out_pitch), over.get('count', cnt.data_ptr() + skew if want_count else None),
            over.get('count_pitch', count_pitch), None)
    torch.cuda.synchronize()
    got, got_c = down16(out), cnt.cpu().numpy()
    planes = got[skew:skew + oh * out_pitch].reshape(oh, out_pitch), got_c[skew:skew + oh * count_pitch].reshape(oh, count_pitch)
    intact = (got[:skew] == OUT_FILL).all() and (got_c[:skew] == COUNT_FILL).all()
    intact = intact and (got[skew + (oh - 1) * out_pitch + ow:] == OUT_FILL).all() and (got_c[skew + (oh - 1) * count_pitch + ow:] == COUNT_FILL).all()
    intact = intact and (planes[0][:, ow:][:-1] == OUT_FILL).all() and (planes[1][:, ow:][:-1] == COUNT_FILL).all()
    if st != 0 or not want_count:
        intact = intact and (got_c == COUNT_FILL).all()
    if st != 0:
        intact = intact and (got == OUT_FILL).all()
    for f, d in planted:
        assert f is None or np.array_equal(bits(d.cpu().numpy()), bits(f)), 'a field or a lattice changed'
    for j, (b, s) in enumerate(zip(bufs, srcs)):
        back = down16(b)
        assert np.array_equal(back[:, :s.shape[1]], s) and (back[:, s.shape[1]:] == PAD).all(), 'source %d changed' % j
    return st, planes[0][:, :ow].copy(), planes[1][:, :ow].copy() if want_count else None, bool(intact)


def check(ref, lib, srcs, xforms, shape, mode, kappa=2.5, iterations=2, **how):
    """combine against the restatement `ref` -- sr.stack_combine, ar.stack_combine_field or qr.stack_combine_weighted, called with
    the fields, weights and step among `how` that it takes -- bit for bit -> (the restatement's out, count)."""
    lattice = [how[key] for key in ('fields', 'weights', 'step') if key in how]
    want, want_count = ref(srcs, xforms, *lattice, shape, mode, kappa, iterations)
    st, got, got_count, intact = combine(lib, srcs, xforms, shape, mode=mode, kappa=kappa, iterations=iterations, **how)
    assert st == 0 and intact
    same(got, want, 'pixels')
    if got_count is not None:
        same(got_count, want_count, 'counts')
    return want, want_count


def same_records(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in ('s', 'tx', 'ty', 'gain', 'ssd_per_pixel'):
            assert np.float64(g[key]).view(np.uint64) == np.float64(w[key]).view(np.uint64), (key, g[key], w[key])
        assert tuple(g['offset']) == tuple(w['offset']) and g['pixels'] == w['pixels'] and g['rejected'] == w['rejected']


def same_fields(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is not None:
            assert g.dtype == torch.float64 and g.is_cuda and np.array_equal(bits(g.cpu().numpy()), bits(w))
