"""Stacking on the GPU: shg_stack_combine_u16 and shg_shift_ssd_u16 bit for bit against the restatement written from the header
(tests/stack_ref.py) -- every shape in buffers whose pitch exceeds the width with the padding planted and checked: sources of one
pixel, one column and one row, several sizes at once, every capacity of the kernel (N = 1 .. 32), output rows on and off 16 bytes,
samples exactly on and a rounding step beyond the last column, pixels no source covers; values whose sum depends on its order, ties,
saturation, every mode and pass count; the refused arguments; the SSD's window sizes, its empty and one-pixel sets, circles, the
largest term; register_disks against its restatement; and three scans through stack_scans and the command line."""
import functools
import math
import os
import shutil

import numpy as np
import pytest

from tests import stack_ref as sr
from tests import stack_util as su
from tests.linemaps_util import run_json, write_scan
from tests.stack_util import (COUNT_FILL, E_ARG, E_UNSUPPORTED, MODES, OUT_FILL, PAD, SSD_FILL, combine, down16, mods, padded,  # noqa: F401
                              planted_table, random_sources, same_records, up16, void_array)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

check = functools.partial(su.check, sr.stack_combine)


# ---- combine: shapes and transforms ----
@pytest.mark.parametrize('mode', MODES)
def test_one_pixel_one_column_one_row(mods, mode):
    _, _, lib = mods
    one = np.array([[40000]], np.uint16)
    assert check(lib, [one], [(1.0, 0.0, 0.0, 1.0)], (1, 1), mode)[0].tolist() == [[40000]]
    rng = np.random.default_rng(3)
    column, row = rng.integers(0, 65536, (9, 1)).astype(np.uint16), rng.integers(0, 65536, (1, 11)).astype(np.uint16)
    # a source one pixel wide is present at sx = 0 only (x1 clamps to 0), one a pixel high at sy = 0 only; s = 0.25 puts four output
    # columns (rows) on fractions of it, ty (tx) lies between two of its pixels
    xforms = [(0.25, 0.0, 1.5, 1.0), (0.25, 2.25, 0.0, 0.9)]
    want, count = check(lib, [column, row], xforms, (5, 7), mode, 1.0, 2)
    assert count[0, 0] == 2 and count[4, 0] == 1 and count[0, 6] == 1 and count[4, 6] == 0 and want[4, 6] == 0
    assert count[:, 1:].max() == 1 and count[1:, :].max() == 1                   # (only the first column sees the column, the first row the row)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('layout', ['aligned', 'odd_pitch', 'skewed'])
def test_three_sizes_partial_coverage_and_both_store_paths(mods, mode, layout):
    """70 x 67 from sources of three sizes that each cover a part of it; 67 is no multiple of the eight columns a thread owns.
    aligned: rows on 16 bytes (pitch 72: the 16-byte stores, the last three columns by element); odd_pitch, skewed: by element."""
    _, _, lib = mods
    srcs, xforms = random_sources(3, [(60, 80), (75, 50), (40, 64)], 7, spread=6.0)
    how = {'aligned': dict(out_extra=5, count_extra=5), 'odd_pitch': dict(out_extra=2, count_extra=1),
           'skewed': dict(out_extra=5, count_extra=5, skew=1)}[layout]
    want, count = check(lib, srcs, xforms, (70, 67), mode, 1.1, 2, **how)
    # (of three samples the clipping at kappa 1.1 nearly always drops the farthest)
    assert sorted(set(count.ravel().tolist())) == ([0, 1, 2] if mode == 'sigma' else [0, 1, 2, 3]) and (want[count == 0] == 0).all()
    check(lib, srcs, xforms, (5, 7), mode, 1.1, 2, **how)
    check(lib, srcs, xforms, (70, 67), mode, 1.1, 2, want_count=False, **how)     # the count plane is optional


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 8, 9, 16, 17, 32])
def test_every_capacity(mods, n):
    """N on either side of every capacity the kernel is built for (4, 8, 16, 32), every mode, one to three passes."""
    _, _, lib = mods
    srcs, xforms = random_sources(n, [(23, 21), (19, 26)], 100 + n)
    for mode in MODES:
        for iterations in (1, 2, 3) if mode == 'sigma' else (2,):
            want, count = check(lib, srcs, xforms, (20, 19), mode, 1.3, iterations)
            assert count.max() <= n
    if n >= 9:
        passes = [sr.stack_combine(srcs, xforms, (20, 19), 'sigma', 1.3, it)[1] for it in (1, 2, 3)]
        assert (passes[0] != passes[1]).any() and (passes[0] < n).any()           # the passes clip, and a second clips more


def test_identity_and_the_edges_of_presence(mods):
    _, _, lib = mods
    img = np.random.default_rng(9).integers(0, 65536, (12, 17)).astype(np.uint16)
    for mode in MODES:
        want, count = check(lib, [img, img], [(1.0, 0.0, 0.0, 1.0)] * 2, img.shape, mode)
        assert np.array_equal(want, img) and (count == 2).all()
    # column 16 of the output sits exactly on the last column of the source, row 11 on its last row: present, neighbour clamped
    want, count = check(lib, [img], [(1.0, 0.0, 0.0, 1.0)], (12, 17), 'mean')
    assert count[11, 16] == 1 and want[11, 16] == img[11, 16]
    up, down = math.inf, -math.inf
    want, count = check(lib, [img], [(1.0, 16.0, 11.0, 1.0)], (2, 2), 'mean')     # (0, 0) -> (16, 11) = (w - 1, h - 1); the rest beyond
    assert count.tolist() == [[1, 0], [0, 0]] and want[0, 0] == img[11, 16]
    for xform in ((1.0, math.nextafter(0.0, down), 0.0, 1.0), (1.0, 0.0, math.nextafter(0.0, down), 1.0),
                  (1.0, math.nextafter(16.0, up), 0.0, 1.0), (1.0, 0.0, math.nextafter(11.0, up), 1.0)):
        want, count = check(lib, [img], [xform], (1, 1), 'mean')
        assert count.tolist() == [[0]] and want.tolist() == [[0]]
    want, count = check(lib, [img], [(1.0, math.nextafter(16.0, down), math.nextafter(11.0, down), 1.0)], (1, 1), 'mean')
    assert count.tolist() == [[1]]


# ---- combine: values and modes ----
@pytest.mark.parametrize('value', [0, 65535])
def test_constant_images(mods, value):
    _, _, lib = mods
    srcs = [np.full((9, 10), value, np.uint16)] * 3
    xforms = [(1.0, 0.3, 0.6, 1.0), (1.01, 0.0, 0.2, 1.0), (0.99, 0.5, 0.0, 1.0)]
    for mode in MODES:
        want, count = check(lib, srcs, xforms, (8, 9), mode, 1.0, 3)                 # q = 0: a pass that rejects nothing
        assert (want[count > 0] == value).all() and (count == 3).any()
    want, _ = check(lib, srcs, [(s, tx, ty, 3.7) for s, tx, ty, _ in xforms], (8, 9), 'mean')
    assert (want[want > 0] == (65535 if value else 0)).all()                         # a gain that saturates


def order_images():
    """Three images whose weighted sum a / 3 + 3.7 b + c / 3 is, exactly, 3 k + 1.5 -- a mean of k + 0.5 --: 10 (a + c) + 111 b =
    90 k + 45 needs b = 5 (mod 10) and a + c = 9 k + (45 - 111 b) / 10.  Where the rounded sum falls, and with it the side of the tie,
    depends on the order of the additions."""
    a, b, c = [], [], []
    for bb in range(5, 400, 10):
        for k in range(bb * 2, bb * 2 + 40):
            total = 9 * k + (45 - 111 * bb) // 10
            for split in (total // 7, total // 3, total // 2):
                a.append(split), b.append(bb), c.append(total - split)
    shape = (40, len(a) // 40)
    return [np.array(t[:shape[0] * shape[1]], np.uint16).reshape(shape) for t in (a, b, c)]


def test_the_sum_follows_the_source_order(mods):
    _, _, lib = mods
    a, b, c = order_images()
    gains = (1.0 / 3.0, 3.7, 1.0 / 3.0)
    xf = [(1.0, 0.0, 0.0, g) for g in gains]
    for mode in ('mean', 'sigma'):
        want, _ = check(lib, [a, b, c], xf, a.shape, mode, 1e9, 1)                    # (kappa 1e9: a pass that rejects nothing)
        other = sr.stack_combine([c, b, a], xf[::-1], a.shape, mode, 1e9, 1)[0]
        assert (want != other).any(), 'the permuted sum rounds alike everywhere: the case shows nothing'
        check(lib, [c, b, a], xf[::-1], a.shape, mode, 1e9, 1)


def test_ties_round_to_even_and_gains_saturate(mods):
    _, _, lib = mods
    rng = np.random.default_rng(4)
    a = rng.integers(0, 65535, (16, 24)).astype(np.uint16)
    xf = [(1.0, 0.0, 0.0, 1.0)] * 2
    for mode in MODES:
        want, _ = check(lib, [a, a + np.uint16(1)], xf, a.shape, mode)                # every mean and median is a tie
        assert np.array_equal(want, np.where(a % 2 == 0, a, a + 1))
    want, _ = check(lib, [a], [(1.0, 0.5, 0.0, 1.0)], (16, 23), 'mean')               # and half-pixel shifts give the ties of a resample
    big = (a | np.uint16(0x8000))
    want, _ = check(lib, [big, big], [(1.0, 0.0, 0.0, 3.7), (1.0, 0.0, 0.0, 1e300)], a.shape, 'mean')
    assert (want == 65535).all()
    want, count = check(lib, [big] * 3, [(1.0, 0.0, 0.0, g) for g in (1.0, 1e305, 1.0)], a.shape, 'sigma', 1.0, 3)
    assert (want == 65535).all() and (count == 3).all()                               # infinite: no sample kept, the set stays
    want, _ = check(lib, [a], [(1.0, 0.0, 0.0, 0.0)], a.shape, 'median')
    assert (want == 0).all()


# ---- combine: refused arguments ----
def test_refused_arguments_leave_the_outputs_untouched(mods):
    _, _, lib = mods
    srcs, xforms = random_sources(2, [(20, 22)], 1)
    nan, inf = float('nan'), float('inf')

    def refused(code, xform=None, **over):
        xf = list(xforms)
        if xform is not None:
            xf[1] = xform
        st, _, _, intact = combine(lib, srcs, xf, (18, 20), mode='sigma', kappa=over.pop('kappa', 2.5), iterations=over.pop('iterations', 2), **over)
        assert st == code and intact, (over, xform)

    for over in (dict(oh=0), dict(ow=16385), dict(dims={1: (16385, 22, 23)}), dict(dims={0: (20, 0, 23)})):
        refused(E_UNSUPPORTED, **over)
    for over in (dict(n=0), dict(n=33), dict(srcs_ptr=None), dict(dims_ptr=None), dict(xf_ptr=None), dict(out=None), dict(null_src=1),
                 dict(out_pitch=19), dict(count_pitch=19), dict(dims={1: (20, 22, 21)}), dict(kappa=nan), dict(kappa=0.999),
                 dict(iterations=0), dict(iterations=4)):
        refused(E_ARG, **over)
    for mode in (3, -1):
        st, _, _, intact = combine(lib, srcs, xforms, (18, 20), mode=mode)
        assert st == E_ARG and intact
    for xform in ((0.0, 0.0, 0.0, 1.0), (-1.0, 0.0, 0.0, 1.0), (nan, 0.0, 0.0, 1.0), (inf, 0.0, 0.0, 1.0), (1.0, nan, 0.0, 1.0),
                  (1.0, 0.0, -inf, 1.0), (1.0, 0.0, 0.0, -1e-300), (1.0, 0.0, 0.0, nan), (1.0, 0.0, 0.0, inf)):
        refused(E_ARG, xform)
    # an output that aliases a source: the source's own buffer, its last element, and the count plane on the source
    buf = padded(srcs[0], 1)
    ptrs = void_array([buf.data_ptr(), buf.data_ptr()])
    dims = np.array([[20, 22, 23], [20, 22, 23]], np.int64)
    xf = np.array(xforms, np.float64)
    other = up16(np.full(20 * 23, OUT_FILL))
    cnt = torch.full((20 * 23,), COUNT_FILL, dtype=torch.uint8, device='cuda')
    last = buf.data_ptr() + 2 * (19 * 23 + 21)
    for out, count in ((buf.data_ptr(), cnt.data_ptr()), (last, cnt.data_ptr()), (other.data_ptr(), last), (other.data_ptr(), other.data_ptr())):
        assert lib.shg_stack_combine_u16(ptrs, dims.ctypes.data, xf.ctypes.data, 2, 0, 2.5, 2, out, 20, 22, 23, count, 23, None) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(down16(buf)[:, :22], srcs[0]) and (down16(other) == OUT_FILL).all() and (cnt.cpu().numpy() == COUNT_FILL).all()


# ---- SSD ----
def ssd(lib, ref, img, search, circle='none', extra=(1, 3), **over):
    """shg_shift_ssd_u16 on padded buffers into a planted table -> (status, table uint64, guards and padding intact)."""
    h, w = ref.shape
    a, b = padded(ref, extra[0]), padded(img, extra[1])
    words = (2 * search + 1) ** 2 + 1 if 0 <= search <= 8 else 1
    table, c3 = planted_table(words), su.circle3(circle)
    st = lib.shg_shift_ssd_u16(over.get('ref_ptr', a.data_ptr()), over.get('ref_pitch', w + extra[0]), over.get('img_ptr', b.data_ptr()),
                               over.get('img_pitch', w + extra[1]), over.get('h', h), over.get('w', w), search,
                               None if c3 is None else c3.ctypes.data, over.get('table', table.data_ptr()), None)
    torch.cuda.synchronize()
    got = table.cpu().numpy().view(np.uint64)
    intact = (got[words if st == 0 else 0:] == SSD_FILL).all()
    assert (down16(a)[:, w:] == PAD).all() and (down16(b)[:, w:] == PAD).all()
    return st, got[:words], bool(intact)


def check_ssd(lib, ref, img, search, circle='none'):
    want = sr.shift_ssd(ref, img, search, None if circle == 'none' else circle)
    st, got, intact = ssd(lib, ref, img, search, circle)
    assert st == 0 and intact
    su.same(got, want, 'sums')
    return want


SSD_CASES = [  # (name, h, w, S, circle)
    ('s0', 40, 37, 0, 'none'), ('s1', 40, 37, 1, 'none'), ('s8', 40, 37, 8, 'none'),
    ('one_pixel', 17, 17, 8, 'none'), ('one_row', 17, 30, 8, 'none'), ('narrow', 10, 30, 8, 'none'), ('narrow_w', 30, 16, 8, 'none'),
    ('1x1_s0', 1, 1, 0, 'none'), ('off_image', 40, 37, 3, (200.0, 200.0, 20.0)),
    ('tiles', 130, 70, 8, 'none'), ('tiles_disk', 130, 70, 8, (33.4, 61.7, 40.2)), ('tiles_s3', 130, 70, 3, (33.4, 61.7, 25.0)),
    ('no_circle', 64, 64, 2, (-1, -1, -1)), ('limb', 64, 64, 2, (32.0, 32.0, 5.0)),
    ('limb_in', 64, 64, 2, (32.0, 32.0, math.nextafter(5.0, 0.0))), ('wide', 20, 300, 4, (150.5, 9.5, 120.0)),
]


@pytest.mark.parametrize('case', SSD_CASES, ids=[c[0] for c in SSD_CASES])
def test_ssd_matches_the_restatement(mods, case):
    _, _, lib = mods
    name, h, w, search, circle = case
    rng = np.random.default_rng([h, w, search])
    ref, img = rng.integers(0, 65536, (h, w)).astype(np.uint16), rng.integers(0, 65536, (h, w)).astype(np.uint16)
    want = check_ssd(lib, ref, img, search, circle)
    pixels = int(want[-1])
    if name == 'one_pixel':
        assert pixels == 1
    if name in ('narrow', 'narrow_w', 'off_image'):
        assert pixels == 0 and (want == 0).all()
    if name == 'no_circle':
        assert pixels == 60 * 60
    if name == 'limb':                                                           # (3, 4) lies exactly on the limb: 81 pixels, 69 just inside
        assert pixels == 81
    if name == 'limb_in':
        assert pixels == 69
    if name == 'tiles':
        assert pixels == (130 - 16) * (70 - 16)


def test_ssd_of_the_largest_term_and_of_equal_images(mods):
    _, _, lib = mods
    zero, full = np.zeros((64, 64), np.uint16), np.full((64, 64), 65535, np.uint16)
    for search in (0, 1):
        want = check_ssd(lib, zero, full, search)
        assert (want[:-1] == 65535 ** 2 * int(want[-1])).all() and want[-1] == (64 - 2 * search) ** 2
        check_ssd(lib, full, zero, search)
    img = np.random.default_rng(2).integers(0, 65536, (50, 45)).astype(np.uint16)
    want = check_ssd(lib, img, img, 4, (22.0, 25.0, 18.0))
    assert want[4 * 9 + 4] == 0 and (np.delete(want[:-1], 40) > 0).all()
    shifted = np.roll(img, (2, -3), axis=(0, 1))                                  # shifted[r + 2][c - 3] = img[r][c]: the minimum at (-3, 2)
    want = check_ssd(lib, img, shifted, 4, (22.0, 25.0, 15.0))
    assert int(np.argmin(want[:-1])) == (2 + 4) * 9 + (-3 + 4) and want[(2 + 4) * 9 + 1] == 0


def test_ssd_refusals_leave_the_table_untouched(mods):
    _, _, lib = mods
    img = np.random.default_rng(6).integers(0, 65536, (20, 22)).astype(np.uint16)
    for over, code in ((dict(h=0), E_UNSUPPORTED), (dict(w=16385), E_UNSUPPORTED), (dict(ref_ptr=None), E_ARG), (dict(img_ptr=None), E_ARG),
                       (dict(table=None), E_ARG), (dict(ref_pitch=21), E_ARG), (dict(img_pitch=21), E_ARG)):
        st, _, intact = ssd(lib, img, img, 2, **over)
        assert st == code and intact, over
    for search in (-1, 9):
        st, _, intact = ssd(lib, img, img, search)
        assert st == E_ARG and intact
    for circle in ((float('nan'), 1.0, 5.0), (1.0, float('inf'), 5.0), (1.0, 1.0, float('nan'))):
        st, _, intact = ssd(lib, img, img, 2, circle)
        assert st == E_ARG and intact


# ---- the wrappers, and the registration against its restatement ----
def test_ops_wrappers(mods):
    _, ops, _ = mods
    srcs, xforms = random_sources(3, [(30, 33), (28, 36)], 21)
    views = [padded(s, 2)[:, :s.shape[1]] for s in srcs]
    want, want_count = sr.stack_combine(srcs, xforms, (29, 31), 'sigma', 1.2, 2)
    out, count = ops.stack_combine_u16(views, xforms, (29, 31), 'sigma', 1.2, 2)
    assert out.dtype == torch.uint16 and count.dtype == torch.uint8
    assert np.array_equal(down16(out), want) and np.array_equal(count.cpu().numpy(), want_count)
    again, none = ops.stack_combine_u16(views, xforms, (29, 31), 'sigma', 1.2, 2, out=out, want_count=False)
    assert again is out and none is None and np.array_equal(down16(out), want)
    with pytest.raises(ValueError):
        ops.stack_combine_u16(views, xforms, (29, 31), out=out[:-1])
    with pytest.raises(RuntimeError, match='kappa'):
        ops.stack_combine_u16(views, xforms, (29, 31), kappa=0.5)
    ref, img = views[0], ops.stack_combine_u16(views[:1], [(1.0, 1.0, -2.0, 1.0)], srcs[0].shape, 'mean')[0]
    table = ops.shift_ssd_u16(ref, img, 3, (15.0, 15.0, 9.0))
    assert table.dtype == torch.int64 and np.array_equal(table.cpu().numpy().view(np.uint64), sr.shift_ssd(srcs[0], down16(img), 3, (15.0, 15.0, 9.0)))
    with pytest.raises(ValueError):
        ops.shift_ssd_u16(ref, views[1], 3)
    with pytest.raises(ValueError):
        ops.shift_ssd_u16(ref, img, 9)


@pytest.fixture(scope='module')
def series():
    images, true, given = sr.synthetic_series()
    for img in images:
        img.setflags(write=False)
    return images, given, sr.register_disks(images, given)


def test_register_and_stack_disks_match_the_restatement(mods, series):
    stack, _, _ = mods
    images, given, want_records = series
    dev = [up16(img) for img in images]
    records = stack.register_disks(dev, given)
    same_records(records, want_records)
    assert not any(rec['rejected'] for rec in records)
    rows = [(r['s'], r['tx'], r['ty'], r['gain']) for r in want_records]
    for mode, kappa in (('sigma', sr.SERIES_KAPPA), ('mean', 2.5), ('median', 2.5)):
        out, count = stack.stack_disks(dev, records, mode, kappa, 2)
        want, want_count = sr.stack_combine(images, rows, images[0].shape, mode, kappa, 2)
        assert np.array_equal(down16(out), want) and np.array_equal(count.cpu().numpy(), want_count)
    # another reference, a smaller window: the same against the restatement; a window the offset does not fit rejects the frame
    same_records(stack.register_disks(dev[:3], given[:3], reference=2, search=4), sr.register_disks(images[:3], given[:3], 2, 4))
    narrow = stack.register_disks(dev[:2], given[:2], search=1)
    same_records(narrow, sr.register_disks(images[:2], given[:2], 0, 1))
    assert narrow[1]['rejected']
    with pytest.raises(ValueError, match='level'):
        stack.register_disks([dev[0], up16(np.zeros_like(images[0]))], given[:2])


# ---- end to end: three scans ----
@pytest.fixture(scope='module')
def scans(mods, tmp_path_factory):
    """sr.pipeline_series() on disk, stack_scans' result, and the pipeline's own product of the reference scan."""
    from solex_ser_recon_en_amd import SHG_MAIN, outputs
    from solex_ser_recon_en_amd.png_io import read_png_gray
    stack = mods[0]
    paths = [write_scan(tmp_path_factory, 'stack%d' % i, frames) for i, frames in enumerate(sr.pipeline_series())]
    products = tmp_path_factory.mktemp('stack_products') / 'scan.ser'
    shutil.copy(paths[0], products)
    assert SHG_MAIN.main([str(products)]) == 0
    outputs.flush()
    return {'paths': paths, 'uncontrasted': read_png_gray(str(products)[:-4] + '_shift=0_uncontrasted.png'), 'res': stack.stack_scans(paths)}


def test_stack_scans_is_the_restatement_of_its_disks(mods, scans):
    stack = mods[0]
    res = scans['res']
    images, circles = [down16(t) for t in res['images']], res['circles']
    assert np.array_equal(images[0], scans['uncontrasted']) and images[0].dtype == np.uint16
    one = stack.scan_disk(scans['paths'][1])
    assert np.array_equal(down16(one['image']), images[1]) and one['circle'] == circles[1]
    want, want_count, want_records = sr.stack_series(images, circles)
    same_records(res['records'], want_records)
    assert res['used'] == [0, 1, 2] and res['rejected'] == [] and res['circle'] == circles[0]
    assert np.array_equal(down16(res['stack']), want) and np.array_equal(res['count'].cpu().numpy(), want_count)
    assert tuple(res['stack'].shape) == images[0].shape and int(want_count.max()) == 3
    noise = sr.pipeline_noise(down16(res['stack']), images[0], circles[0])
    print('noise of the stack against the reference frame\'s: %.6f' % noise)
    assert noise <= sr.TOLERANCE['pipeline']['noise']


def test_command_line(mods, scans, tmp_path, capsys):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.fits_io import read_fits_u16
    from solex_ser_recon_en_amd.png_io import read_png_gray
    stack = mods[0]
    work = []
    for i, path in enumerate(scans['paths']):
        work.append(str(tmp_path / ('scan%d.ser' % i)))
        shutil.copy(path, work[-1])
    res = scans['res']
    k = SHG_MAIN.default_options()['img_rotate'] // 90
    want = np.rot90(down16(res['stack']), k)
    out = run_json(stack.main, capsys, work + ['--coverage', '--contrast', '-f'])
    base = work[0][:-4] + '_shift=0_stack'
    assert out['png'] == base + '.png' and out['fits'] == base + '.fits' and out['count_png'] == base + '_count.png'
    assert np.array_equal(read_png_gray(out['png']), want) and np.array_equal(read_fits_u16(out['fits'])[0], want)
    assert np.array_equal(read_png_gray(out['count_png']), np.rot90(res['count'].cpu().numpy(), k))
    for suffix in ('_clahe.png', '_protus.png', '_uncontrasted.png', '_clahe.fits'):
        assert os.path.exists(base + suffix), suffix
    assert np.array_equal(read_png_gray(base + '_uncontrasted.png'), want)
    assert out['shape'] == list(want.shape) and out['mode'] == 'sigma' and out['kappa'] == 2.5 and out['iterations'] == 2
    assert out['files'] == work and out['rejected'] == [] and out['shift'] == 0 and out['reference'] == 0
    assert out['circle'] == list(res['circle']) and out['ratio'] == res['ratio']
    for frame, rec, path in zip(out['frames'], res['records'], work):
        assert frame['file'] == path and frame['scale'] == rec['s'] and frame['offset'] == list(rec['offset'])
        assert frame['gain'] == rec['gain'] and frame['rms'] == math.sqrt(rec['ssd_per_pixel']) and frame['rejected'] is False
    # another reference, another mode: the stack sits on that scan's grid and carries its name
    out = run_json(stack.main, capsys, work + ['--reference', '2', '--mode', 'median', '--search', '6'])
    assert out['png'] == work[2][:-4] + '_shift=0_stack.png' and out['fits'] is None and out['count_png'] is None and out['mode'] == 'median'
    other = stack.stack_scans(work, reference=2, mode='median', search=6)
    assert np.array_equal(read_png_gray(out['png']), np.rot90(down16(other['stack']), k))
    assert stack.main(work + ['-x']) == 1                                         # no limb fit, no circle
    assert 'circle' in capsys.readouterr().err
