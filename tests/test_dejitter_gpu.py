"""Dejittering on the GPU: shg_column_limb_u16 and shg_column_shift_u16 bit for bit against the restatement written from the header
(tests/dejitter_ref.py) -- images in buffers whose pitch exceeds the width, on and off 16 bytes, with the padding planted and
checked; one column, several workgroups, every window; columns of pure sky, of pure disk, with a disk that touches the first or the
last row, with window sums that equal K T exactly, with crossings on every boundary between the row segments of a workgroup;
thresholds 0 and 65535; shifts of every kind for 1, 3 and 21 planes --, then the Python layer and a scan end to end: planted
whole-row jitter recovered, the untouched path bit for bit what it was, the command line's files."""
import os
import shutil

import numpy as np
import pytest

from solex_ser_recon_en_amd import dejitter as _dejitter  # noqa: F401  (no feature: no tests)
from tests import dejitter_ref as jr
from tests import flatten_ref as fr
from tests.linemaps_util import run_json, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
PAD, FILL = 0xBEEF, 0x5A5A
SHAPES = [(7, 1), (9, 8), (40, 67), (64, 130), (200, 260)]
WINDOWS = (1, 5, 15)


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import dejitter, disk, ops
    from solex_ser_recon_en_amd._lib import lib
    return {'dejitter': dejitter, 'disk': disk, 'ops': ops, 'lib': lib}


def up16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.uint16)


def down16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class Planes:
    """[n, h, w] images inside a flat device buffer: `skew` elements in, rows `pitch` and planes `stride` apart (more than h pitch),
    everything else planted with `fill`.  aligned: every row starts on 16 bytes (the kernels' 16-byte path); else the pitch is odd
    and the start two bytes off (the element path)."""
    def __init__(self, n, h, w, aligned, fill, imgs=None):
        self.n, self.h, self.w, self.fill = n, h, w, fill
        self.pitch = w + (-w) % 8 + 8 if aligned else w + 3 + w % 2
        self.stride = h * self.pitch + (16 if aligned else 5)
        self.skew = 0 if aligned else 1
        host = np.full(self.skew + n * self.stride + 8, fill, np.uint16)
        self.mask = np.zeros(host.shape, bool)
        for p in range(n):
            at = self.skew + p * self.stride
            self.mask[at:at + h * self.pitch].reshape(h, self.pitch)[:, :w] = True
        if imgs is not None:
            host[self.mask] = np.asarray(imgs, dtype=np.uint16).reshape(-1)
        self.buf = up16(host)
        self.ptr = self.buf.data_ptr() + 2 * self.skew
        assert (self.ptr % 16 == 0 and self.pitch % 8 == 0 and self.stride % 8 == 0) == bool(aligned)

    def read(self):
        """(the images [n, h, w], whether everything around them still holds the fill)."""
        got = down16(self.buf)
        return got[self.mask].reshape(self.n, self.h, self.w), bool((got[~self.mask] == self.fill).all())

    def untouched(self):
        return bool((down16(self.buf) == self.fill).all())


def run_limb(lib, img, window, threshold, aligned, **over):
    """shg_column_limb_u16 on the image in a padded buffer -> (status, the table or None, whether the image, its padding and the
    table's guards are as they were -- and, after a refusal, the table too)."""
    h, w = img.shape
    src = Planes(1, h, w, aligned, PAD, img)
    table = torch.full((w * 6 + 16,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    st = lib.shg_column_limb_u16(over.get('img_ptr', src.ptr), over.get('h', h), over.get('w', w), over.get('pitch', src.pitch), window, threshold,
                                 over.get('table', table.data_ptr() + 32), None)
    torch.cuda.synchronize()
    back, intact = src.read()
    intact = intact and np.array_equal(back[0], img)
    got = table.cpu().numpy()
    guards = (got[:8] == 0x5A5A5A5A).all() and (got[8 + w * 6:] == 0x5A5A5A5A).all()
    if st != 0:
        return st, None, bool(intact and guards and (got == 0x5A5A5A5A).all())
    return st, got[8:8 + w * 6].reshape(w, 6), bool(intact and guards)


def same_table(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, '%s: %d words differ, first at column %d: %s vs %s' % (what, len(bad), bad[0][0], got[bad[0][0]], ref[bad[0][0]])


def limb_image(h, w, window, threshold, seed):
    """Columns of every kind, in turn: a disk in the sky with noise on both; pure sky; pure disk; a disk that touches row 0; one that
    touches row h - 1; a disk of exactly T on a sky of 0 (the window's sum equals K T where it lies in the disk, and nowhere else);
    noise about T (many crossings); two disks; the whole range at random."""
    rng = np.random.default_rng([h, w, window, seed])
    t = max(1, min(int(threshold), 65534))
    lo, hi = (0, t), (t, 65536)
    img = np.empty((h, w), np.uint16)
    for c in range(w):
        kind = c % 9
        a, b = sorted(rng.integers(0, h, 2))
        col = rng.integers(*lo, h)
        if kind == 0:
            col[a:b + 1] = rng.integers(*hi, b + 1 - a)
        elif kind == 2:
            col = rng.integers(*hi, h)
        elif kind == 3:
            col[:b + 1] = rng.integers(*hi, b + 1)
        elif kind == 4:
            col[a:] = rng.integers(*hi, h - a)
        elif kind == 5:
            col[:] = 0
            col[a:b + 1] = threshold
        elif kind == 6:
            col = rng.integers(max(0, t - 3), min(65536, t + 4), h)
        elif kind == 7:
            col[a // 2:a // 2 + 2] = rng.integers(*hi, 2)
            col[b:b + 3] = rng.integers(*hi, h - b if b + 3 > h else 3)
        elif kind == 8:
            col = rng.integers(0, 65536, h)
        img[:, c] = col
    return img


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_column_limb_matches_the_restatement(mods, shape):
    lib = mods['lib']
    h, w = shape
    measured = 0
    for window in WINDOWS:
        for turn, threshold in enumerate((300, 0, 65535, 20000)):
            img = limb_image(h, w, window, threshold, turn)
            ref = jr.column_limb(img, window, threshold)
            measured += int((ref[:, 0] >= 0).sum())
            if h < window + 2 or threshold == 0:
                assert (ref == -1).all()
            for aligned in (False, True):
                what = '%d x %d, K %d, T %d, aligned %s' % (h, w, window, threshold, aligned)
                st, got, intact = run_limb(lib, img, window, threshold, aligned)
                assert st == 0 and intact, what
                same_table(got, ref, what)
    assert measured > 0 or h < 9


def test_column_limb_on_every_segment_boundary(mods):
    """A disk of 1000 on a sky of 0 with T = 1000 // K: the window's sum passes K T with the first disk row it holds, so a disk on rows
    a .. b has i_top = a - K + 1 and i_bot = b.  Segment g of a workgroup owns the sums [g L, (g + 1) L): both crossings are put on
    g L - 1, g L and g L + 1 for every g the image has."""
    lib, ops = mods['lib'], mods['ops']
    for h, window in ((200, 5), (200, 15), (700, 5), (1500, 1)):
        seg = ops.column_limb_segment(h, window)
        ni = h - window + 1
        assert seg == -(-ni // ops.COLUMN_LIMB_SEGMENTS) and seg >= 2
        edges = [g * seg + d for g in range(1, ops.COLUMN_LIMB_SEGMENTS) for d in (-1, 0, 1) if 1 <= g * seg + d <= ni - 2]
        columns = []                                                 # (first disk row, last disk row)
        for j, i in enumerate(edges):
            if i <= h - 2 * window:                                  # the top crossing on the boundary, the bottom one wherever
                columns.append((i + window - 1, max(i + window - 1, h - window - 1 - j % 3)))
            if i >= window:                                          # the bottom crossing on it
                columns.append((min(window + j % 3, i), i))
        w = len(columns)
        assert w > ops.COLUMN_LIMB_COLUMNS and h >= 3 * window - 1
        img = np.zeros((h, w), np.uint16)
        for c, (a, b) in enumerate(columns):
            img[a:b + 1, c] = 1000
        want = np.array([(a - window + 1, b) for a, b in columns])
        assert set(edges) <= set(want[:, 0]) | set(want[:, 1])
        ref = jr.column_limb(img, window, 1000 // window)
        assert np.array_equal(ref[:, [0, 3]], want)
        for aligned in (False, True):
            st, got, intact = run_limb(lib, img, window, 1000 // window, aligned)
            assert st == 0 and intact
            same_table(got, ref, 'h %d, K %d, aligned %s' % (h, window, aligned))


def test_column_limb_refusals_leave_everything_untouched(mods):
    lib, ops = mods['lib'], mods['ops']
    img = limb_image(20, 22, 5, 300, 0)

    def refused(code, window=5, threshold=300, **over):
        st, _, intact = run_limb(lib, img, window, threshold, False, **over)
        assert st == code and intact, (window, threshold, over)

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        refused(E_UNSUPPORTED, **over)
    for over in (dict(img_ptr=None), dict(table=None), dict(pitch=21), dict(window=0), dict(window=4), dict(window=17), dict(threshold=-1),
                 dict(threshold=65536)):
        refused(E_ARG, **over)
    src = Planes(1, 20, 22, False, FILL)
    for table in (src.ptr, src.ptr + 2 * (19 * src.pitch + 21) - 2, src.ptr - 22 * 24 + 2):
        assert lib.shg_column_limb_u16(src.ptr, 20, 22, src.pitch, 5, 300, table, None) == E_ARG
    torch.cuda.synchronize()
    assert src.untouched()
    dev = up16(img)
    for bad in (dict(window=4), dict(window=17), dict(window=5.0), dict(threshold=-1), dict(threshold=65536), dict(threshold=0.5),
                dict(out=torch.empty((22, 5), dtype=torch.int32, device='cuda')), dict(out=torch.empty((22, 6), dtype=torch.int64, device='cuda'))):
        with pytest.raises(ValueError):
            ops.column_limb_u16(dev, bad.pop('window', 5), bad.pop('threshold', 300), **bad)
    with pytest.raises(RuntimeError):
        ops.column_limb_u16(torch.zeros((4, 4), dtype=torch.uint16), 1, 3)
    mine = torch.empty((22, 6), dtype=torch.int32, device='cuda')
    got = ops.column_limb_u16(dev, 5, 300, out=mine)
    assert got is mine and np.array_equal(got.cpu().numpy(), jr.column_limb(img, 5, 300))


# ---- the shifts ----
def run_shift(lib, imgs, offset, weight, in_aligned, out_aligned, **over):
    """shg_column_shift_u16 on the planes in a padded buffer into a planted one -> (status, the planes or None, intact)."""
    n, h, w = imgs.shape
    src, dst = Planes(n, h, w, in_aligned, PAD, imgs), Planes(n, h, w, out_aligned, FILL)
    offset, weight = np.ascontiguousarray(offset, dtype=np.int32), np.ascontiguousarray(weight, dtype=np.int32)
    st = lib.shg_column_shift_u16(over.get('img_ptr', src.ptr), over.get('n', n), over.get('h', h), over.get('w', w), over.get('pitch', src.pitch),
                                  over.get('stride', src.stride), over.get('offset_ptr', offset.ctypes.data), over.get('weight_ptr', weight.ctypes.data),
                                  over.get('out', dst.ptr), over.get('out_pitch', dst.pitch), over.get('out_stride', dst.stride), None)
    torch.cuda.synchronize()
    back, intact = src.read()
    intact = intact and np.array_equal(back, imgs)
    if st != 0:
        return st, None, bool(intact and dst.untouched())
    got, around = dst.read()
    return st, got, bool(intact and around)


def same_planes(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, '%s: %d pixels differ, first at %s: %d vs %d' % (what, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def shifts_of(h, w, seed):
    """A shift a column, in turn: 0, +-0.5, whole rows, -3.25, +7.9, +-(h + 2) (every tap clamps), and fractions at random."""
    rng = np.random.default_rng([h, w, seed])
    fixed = [0.0, 0.5, -0.5, 1.0, -2.0, -3.25, 7.9, float(h + 2), -float(h + 2), 3.0]
    s = rng.uniform(-6.0, 6.0, w)
    at = rng.permutation(w)[:len(fixed)] if w >= len(fixed) else np.arange(w)
    s[at] = np.roll(fixed, seed)[:at.size]
    return s


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_column_shift_matches_the_restatement(mods, shape):
    lib = mods['lib']
    h, w = shape
    rng = np.random.default_rng([h, w, 24])
    for turn, n in enumerate((1, 3, 21)):
        imgs = rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
        imgs[n // 2, :, w // 2:] = np.where(np.arange(h)[:, None] % 2 == 0, 65535, 0)       # full scale beside zero: the cubic leaves the range
        for k in range(3 if w == 1 else 1):
            shift = shifts_of(h, w, turn + 3 * k)
            offset, weight = jr.weights(shift)
            ref = jr.column_shift(imgs, offset, weight)
            for in_aligned, out_aligned in ((False, False), (True, True), (False, True), (True, False))[turn % 2::2] if n == 21 else \
                    ((False, False), (True, True), (False, True), (True, False)):
                what = '%d x %d, %d planes, input aligned %s, output aligned %s' % (h, w, n, in_aligned, out_aligned)
                st, got, intact = run_shift(lib, imgs, offset, weight, in_aligned, out_aligned)
                assert st == 0 and intact, what
                same_planes(got, ref, what)


def test_column_shift_identity_clip_and_flat_planes(mods):
    lib = mods['lib']
    h, w = 40, 67
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 65536, (3, h, w)).astype(np.uint16)
    ident = (np.zeros(w, np.int32), np.tile(np.array([0, 16384, 0, 0], np.int32), (w, 1)))
    # weights at the limits of the range, which no Keys fraction reaches: they overshoot by a quarter both ways
    wild = (rng.integers(-2, 3, w).astype(np.int32), np.tile(np.array([-4096, 20480, 4096, -4096], np.int32), (w, 1)))
    wild[1][::2] = (4096, -4096, 20480, -4096)
    stripes = np.broadcast_to(np.where(np.arange(h)[:, None] % 2 == 0, 65535, 0).astype(np.uint16), (1, h, w)).copy()
    for aligned in (False, True):
        st, got, intact = run_shift(lib, imgs, *ident, aligned, aligned)
        assert st == 0 and intact
        same_planes(got, imgs, 'the identity')
        for plane, value in ((np.full((1, h, w), 65535, np.uint16), 65535), (np.zeros((1, h, w), np.uint16), 0)):
            for offset, weight in (wild, jr.weights(shifts_of(h, w, 1))):
                st, got, intact = run_shift(lib, plane, offset, weight, aligned, not aligned)
                assert st == 0 and intact and (got == value).all()
                same_planes(got, jr.column_shift(plane, offset, weight), 'a flat plane')
        ref = jr.column_shift(stripes, *wild)
        # (1.5 x - 0.5 y with x, y the two stripes: beyond the range both ways, so both ends of the clip are taken)
        assert (ref[0, 2:-2, ::2] == 0).any() and (ref[0, 2:-2, ::2] == 65535).any()
        st, got, intact = run_shift(lib, stripes, *wild, aligned, aligned)
        assert st == 0 and intact
        same_planes(got, ref, 'the clip')


def test_column_shift_refusals_leave_everything_untouched(mods):
    lib, ops = mods['lib'], mods['ops']
    h, w = 20, 22
    imgs = np.random.default_rng(4).integers(0, 65536, (2, h, w)).astype(np.uint16)
    offset, weight = jr.weights(shifts_of(h, w, 0))

    def refused(code, **over):
        for key in ('offset', 'weight'):
            if key in over:
                over['keep_' + key] = over.pop(key)                     # (alive during the call)
                over[key + '_ptr'] = None if over['keep_' + key] is None else over['keep_' + key].ctypes.data
        st, _, intact = run_shift(lib, imgs, offset, weight, False, False, **over)
        assert st == code and intact, over

    def changed(a, at, value):
        b = a.copy()
        b[at] = value
        return b

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        refused(E_UNSUPPORTED, **over)
    for over in (dict(img_ptr=None), dict(out=None), dict(offset=None), dict(weight=None), dict(pitch=21), dict(out_pitch=21), dict(n=0), dict(n=65),
                 dict(stride=19 * 25 + 21), dict(out_stride=100), dict(offset=changed(offset, 5, 16385)), dict(offset=changed(offset, 21, -16385)),
                 dict(weight=changed(weight, (3, 1), weight[3, 1] + 1)), dict(weight=changed(weight, (0, 2), weight[0, 2] - 1)),
                 dict(weight=changed(changed(weight, (7, 0), -4097), (7, 1), weight[7, 1] + weight[7, 0] + 4097)),
                 dict(weight=changed(changed(weight, (9, 1), 20481), (9, 2), weight[9, 2] + weight[9, 1] - 20481))):
        refused(E_ARG, **over)
    a, b = Planes(2, h, w, False, FILL), Planes(2, h, w, False, FILL)
    last = 2 * (a.stride + 19 * a.pitch + 21)
    for out in (a.ptr, a.ptr + last, a.ptr - last):
        assert lib.shg_column_shift_u16(a.ptr, 2, h, w, a.pitch, a.stride, offset.ctypes.data, weight.ctypes.data, out, a.pitch, a.stride, None) == E_ARG
    torch.cuda.synchronize()
    assert a.untouched() and b.untouched()
    dev = up16(imgs)
    for bad in (dict(offset=offset[:-1]), dict(weight=weight[:, :3]), dict(offset=changed(offset, 0, 16385)), dict(weight=changed(weight, (0, 1), 0)),
                dict(out=dev[:1]), dict(out=torch.empty((2, h, w), dtype=torch.int16, device='cuda'))):
        with pytest.raises(ValueError):
            ops.column_shift_u16(dev, bad.pop('offset', offset), bad.pop('weight', weight), **bad)
    with pytest.raises(ValueError):
        ops.column_shift_u16(torch.zeros((65, 2, 2), dtype=torch.uint16, device='cuda'), [0, 0], [[0, 16384, 0, 0]] * 2)
    with pytest.raises(RuntimeError, match='overlaps'):
        ops.column_shift_u16(dev, offset, weight, out=dev)
    with pytest.raises(RuntimeError):
        ops.column_shift_u16(torch.zeros((4, 4), dtype=torch.uint16), np.zeros(4), [[0, 16384, 0, 0]] * 4)
    assert np.array_equal(down16(dev), imgs)


# ---- the Python layer ----
def test_measure_and_apply_are_the_restatement(mods):
    dejitter, ops = mods['dejitter'], mods['ops']
    jitter = jr.planted()
    img = jr.scene(jitter=jitter)
    dev = up16(img)
    assert dejitter.threshold(dev) == jr.threshold(img) and dejitter.threshold(dev, 0.3) == jr.threshold(img, 0.3)
    for args in ({}, {'window': 9, 'level': 0.3}, {'threshold': 5000, 'min_chord': 0.6, 'max_shift': 1.0}):
        got = dejitter.measure(dev, **args)
        ref_args = dict(args)
        want = jr.measure(img, ref_args.pop('threshold', None), **ref_args)
        assert got['threshold'] == want['threshold'] and got['window'] == want['window'] and got['n_measured'] == want['n_measured']
        assert np.array_equal(got['measured'], want['measured']) and np.allclose(got['shift'], want['shift'], rtol=0, atol=1e-12)
        assert np.array_equal(got['top'], want['top'], equal_nan=True) and np.array_equal(got['bottom'], want['bottom'], equal_nan=True)
    rec = dejitter.measure(dev)
    planes = np.stack([img, img[::-1], np.roll(img, 3, axis=1)])
    out = dejitter.apply(up16(planes), rec['shift'])
    assert out.shape == (3,) + img.shape and np.array_equal(down16(out), jr.apply(planes, rec['shift']))
    one = dejitter.apply(dev, rec['shift'])
    assert one.shape == img.shape and np.array_equal(down16(one), jr.apply(img, rec['shift']))
    mine = ops.pitched_u16(img.shape[0], img.shape[1], 'cuda', 8)
    assert ops.column_shift_u16(dev, *dejitter.weights(rec['shift']), out=mine) is mine and np.array_equal(down16(mine), down16(one))
    # the accuracy the restatement measures is the GPU's
    got = jr.accuracy(lambda im: dejitter.measure(up16(im)), lambda im, shift: down16(dejitter.apply(up16(im), shift)))
    assert got == jr.accuracy()
    for key, bound in jr.TOLERANCE.items():
        assert got[key] <= bound, key
    with pytest.raises(ValueError):
        dejitter.measure(up16(np.zeros((50, 50), np.uint16)), threshold=100)


# ---- end to end: a scan ----
@pytest.fixture(scope='module')
def scans(mods, tmp_path_factory):
    """The small synthetic scan of the flatten and stack tests, and the same with every frame rolled along the slit by a whole number
    of rows in -2 .. 2 (the wrap falls in the sky).  The file holds the frames turned by a quarter: the slit is a frame's second
    axis there, and it runs the other way, so a roll by d rows moves that frame's column of the raw disk by -d."""
    frames = fr.pipeline_scan()
    rows = np.random.default_rng(7).integers(-2, 3, frames.shape[0])
    rolled = np.stack([np.roll(f, int(d), axis=1) for f, d in zip(frames, rows)])
    return {'still': write_scan(tmp_path_factory, 'dejitter_still', frames), 'moved': write_scan(tmp_path_factory, 'dejitter_moved', rolled),
            'planted': -rows.astype(np.float64)}


def test_scan_recovers_planted_rows(mods, scans):
    dejitter = mods['dejitter']
    res = dejitter.dejitter_scan(scans['moved'])
    jitter = res['jitter']
    m = jitter['measured']
    assert jitter['rejected_by_max_shift'] == 0 and jitter['n_measured'] >= 0.6 * jitter['crossing']
    err = jr.detrended(jitter['shift'] - scans['planted'], m)[m]
    rms, worst = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    print('planted whole rows recovered to %.6f px rms, worst %.6f, over %d columns' % (rms, worst, int(m.sum())))
    assert rms <= jr.TOLERANCE['shift_rms'] and worst <= jr.TOLERANCE['shift_max']
    assert res['image'].dtype == torch.uint16 and len(res['circle']) == 3
    # the corrected scan's disk is round where the jittered one's limb is jagged: its circle is the still scan's within a pixel
    still = mods['disk'].scan_disk(scans['still'])
    assert np.abs(np.array(res['circle']) - np.array(still['circle'])).max() < 1.0


def test_still_scan_stays_within_the_floor(mods, scans):
    jitter = mods['dejitter'].dejitter_scan(scans['still'])['jitter']
    print('a scan without jitter: %.6f px rms found, worst %.6f, over %d columns' % (jitter['rms'], jitter['max'], jitter['n_measured']))
    assert jitter['rejected_by_max_shift'] == 0 and jitter['n_measured'] >= 0.6 * jitter['crossing']
    assert jitter['rms'] <= jr.TOLERANCE['floor']


def test_scan_disk_without_dejitter_is_what_it_was(mods, scans):
    disk = mods['disk']
    plain, none = disk.scan_disk(scans['moved']), disk.scan_disk(scans['moved'], dejitter=None)
    assert sorted(plain) == sorted(none) == ['circle', 'crop', 'image', 'phi', 'ratio', 'shift']
    assert np.array_equal(down16(plain['image']), down16(none['image']))
    assert all(plain[k] == none[k] for k in ('circle', 'crop', 'phi', 'ratio', 'shift'))
    fixed = disk.scan_disk(scans['moved'], dejitter={})
    assert sorted(set(fixed) - set(plain)) == ['jitter'] and not np.array_equal(down16(fixed['image']), down16(plain['image']))


def test_command_lines(mods, scans, tmp_path, capsys):
    from solex_ser_recon_en_amd import SHG_MAIN, flatten
    from solex_ser_recon_en_amd.fits_io import read_fits_u16
    from solex_ser_recon_en_amd.png_io import read_png_gray
    dejitter = mods['dejitter']
    work = str(tmp_path / 'scan.ser')
    shutil.copy(scans['moved'], work)
    base = work[:-4]
    k = SHG_MAIN.default_options()['img_rotate'] // 90
    out = run_json(dejitter.main, capsys, [work, '-f'])
    assert out['png'] == base + '_shift=0_dejitter.png' and out['fits'] == base + '_shift=0_dejitter.fits' and out['txt'] == base + '_jitter.txt'
    want = dejitter.dejitter_scan(work)
    image = np.rot90(down16(want['image']), k)
    assert np.array_equal(read_png_gray(out['png']), image) and np.array_equal(read_fits_u16(out['fits'])[0], image)
    jitter = want['jitter']
    assert out['threshold'] == jitter['threshold'] and out['n_measured'] == jitter['n_measured'] and out['rms'] == jitter['rms']
    assert out['max'] == jitter['max'] and out['line'] == [jitter['slope'], jitter['intercept']]
    assert out['circle'] == list(want['circle']) and out['ratio'] == want['ratio'] and out['phi'] == want['phi']
    rows = np.loadtxt(out['txt'])
    assert rows.shape == (jitter['shift'].shape[0], 7) and np.array_equal(rows[:, 0], np.arange(rows.shape[0]))
    assert np.allclose(rows[:, 5], jitter['shift'], rtol=0, atol=5.1e-5) and np.array_equal(rows[:, 6] != 0, jitter['measured'])
    out = run_json(dejitter.main, capsys, [work, '--threshold', '2500', '--window', '7', '--min-chord', '0.5', '--max-shift', '4', '--contrast'])
    assert out['threshold'] == 2500 and out['window'] == 7 and out['fits'] is None
    for suffix in ('_clahe.png', '_protus.png'):
        assert os.path.exists(base + '_shift=0_dejitter' + suffix), suffix
    # --dejitter on a product: the flat of the corrected disk, and a jitter key
    plain = run_json(flatten.main, capsys, [work])
    fixed = run_json(flatten.main, capsys, [work, '--dejitter'])
    assert sorted(set(fixed) - set(plain)) == ['jitter'] and fixed['jitter']['n_measured'] == jitter['n_measured']
    assert fixed['jitter'] == {key: out_ for key, out_ in run_json(dejitter.main, capsys, [work]).items() if key in fixed['jitter']}
