"""Flattening the disk on the GPU: shg_ring_medians_u16 and shg_ring_flatten_u16 bit for bit against the restatement written from
the header (tests/flatten_ref.py) -- every shape in a buffer whose pitch exceeds its width with the padding checked, circles with
pixels exactly on a ring boundary and on the limb, centres outside the image and on tile corners, empty rings, constant images and
rings whose middle pair straddles a high byte; rounding ties, saturation and the clamps of the flatten; the refused arguments;
flatten_disk end to end; and one scan through flatten_scan and the command line against the pipeline's own product."""
import math
import os
import shutil

import numpy as np
import pytest

from tests import flatten_ref as fr
from tests.linemaps_util import run_json, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
PAD, OUT_FILL, COUNT_FILL, STAT_FILL = 0xBEEF, 0x5A5A, 0x7EADBEEF, 0x7E57
GUARD = 3                                   # planted elements behind count, lo and hi


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import flatten, ops
    from solex_ser_recon_en_amd._lib import lib
    return flatten, ops, lib


def up16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.uint16)


def down16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def c3(circle):
    return np.ascontiguousarray([float(v) for v in circle], dtype=np.float64)


def padded(img, extra, fill=PAD):
    """img in a device buffer whose pitch is w + extra, the rest `fill` -> the buffer [h, w + extra]."""
    h, w = img.shape
    buf = np.full((h, w + extra), fill, np.uint16)
    buf[:, :w] = img
    return up16(buf)


def medians(lib, img, circle, extra=1, **over):
    """shg_ring_medians_u16 on img in a padded buffer, outputs and workspace planted -> (status, count, lo, hi, guards intact)."""
    h, w = img.shape
    kk = over.pop('k', fr.n_rings(circle))
    src = padded(img, extra)
    count = torch.full((max(kk, 0) + GUARD,), COUNT_FILL, dtype=torch.int32, device='cuda')
    lo, hi = up16(np.full(max(kk, 0) + GUARD, STAT_FILL)), up16(np.full(max(kk, 0) + GUARD, STAT_FILL))
    need = lib.shg_ring_medians_u16_workspace_bytes(max(kk, 1))
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device='cuda')          # (garbage: the call clears what it counts into)
    circ = c3(circle)
    st = lib.shg_ring_medians_u16(over.get('img_ptr', src.data_ptr()), over.get('h', h), over.get('w', w), over.get('pitch', w + extra),
                                  over.get('c3', circ.ctypes.data), kk, over.get('count', count.data_ptr()), over.get('lo', lo.data_ptr()),
                                  over.get('hi', hi.data_ptr()), over.get('ws', ws.data_ptr() + over.get('ws_skew', 0)),
                                  over.get('ws_bytes', need), None)
    torch.cuda.synchronize()
    count, lo, hi = count.cpu().numpy().view(np.uint32), down16(lo), down16(hi)
    n = max(kk, 0) if st == 0 else 0
    intact = (count[n:] == COUNT_FILL).all() and (lo[n:] == STAT_FILL).all() and (hi[n:] == STAT_FILL).all()
    assert np.array_equal(down16(src)[:, w:], np.full((h, extra), PAD, np.uint16))
    return st, count[:kk], lo[:kk], hi[:kk], bool(intact)


def flattened(lib, img, circle, gain, extra=1, out_extra=2, in_place=False, **over):
    """shg_ring_flatten_u16 on img in a padded buffer into a planted one (or in place) -> (status, out [h, w], padding intact)."""
    h, w = img.shape
    kk = over.pop('k', fr.n_rings(circle))
    src = padded(img, extra)
    dst = src if in_place else up16(np.full((h, w + out_extra), OUT_FILL))
    out_pitch = w + extra if in_place else w + out_extra
    circ, g = c3(circle), np.ascontiguousarray(gain, dtype=np.float64)
    st = lib.shg_ring_flatten_u16(over.get('img_ptr', src.data_ptr()), over.get('h', h), over.get('w', w), over.get('pitch', w + extra),
                                  over.get('c3', circ.ctypes.data), over.get('gain_ptr', g.ctypes.data), kk, over.get('out', dst.data_ptr()),
                                  over.get('out_pitch', out_pitch), None)
    torch.cuda.synchronize()
    got = down16(dst)
    pad = got[:, w:]
    intact = (pad == (PAD if in_place else OUT_FILL)).all()
    if not in_place:
        assert np.array_equal(down16(src)[:, :w], img), 'the input changed'
    return st, got[:, :w], bool(intact)


# ---- geometries: (name, h, w, pitch extra, circle) ----
UP, DOWN = math.inf, -math.inf
GEOMETRIES = [
    ('1x1_k1', 1, 1, 1, (0.0, 0.0, 0.0)),
    ('1x1_r09', 1, 1, 3, (0.0, 0.0, 0.9)),
    ('1x1_off', 1, 1, 1, (5.0, 5.0, 3.0)),                               # the only pixel lies off the disk: every ring empty
    ('5x7', 5, 7, 1, (3.0, 2.0, 2.0)),
    ('5x7_big', 5, 7, 2, (3.4, 1.7, 6.3)),                               # the radius exceeds the image: rings cut, rings empty
    ('5x7_outside', 5, 7, 1, (-4.0, 2.0, 7.5)),
    ('64_r5', 64, 64, 1, (32.0, 32.0, 5.0)),                             # (3, 4) exactly on the limb and on ring 5's inner edge
    ('64_r5_in', 64, 64, 1, (32.0, 32.0, math.nextafter(5.0, DOWN))),
    ('64_r10_out', 64, 64, 1, (32.0, 32.0, math.nextafter(10.0, UP))),   # (6, 8)
    ('64_r13', 64, 64, 1, (32.0, 32.0, 13.0)),                           # (5, 12)
    ('64_r13_in', 64, 64, 1, (32.0, 32.0, math.nextafter(13.0, DOWN))),
    ('64_r13_9', 64, 64, 1, (32.0, 32.0, 13.9)),                         # (4, 13): u = 13.1 >= K - 1, the flatten's last clamp
    ('64_k1', 64, 64, 1, (20.0, 41.0, 0.5)),
    ('64_two_px', 64, 64, 1, (32.5, 32.0, 13.0)),                        # ring 0 holds exactly two pixels; with 32.0 exactly one
    ('130_frac_0', 130, 257, 0, (128.3, 64.6, 60.2)),
    ('130_frac_1', 130, 257, 1, (128.3, 64.6, 60.2)),
    ('130_frac_7', 130, 257, 7, (128.3, 64.6, 60.2)),
    ('130_corner64', 130, 257, 1, (64.0, 64.0, 50.0)),                   # the centre on a corner of the 64 x 64 and 32 x 32 tiles
    ('130_corner32', 130, 257, 7, (96.0, 32.0, 40.5)),                   # and on one of the 32 x 32 tiles only
    ('130_outside', 130, 257, 1, (-20.5, 140.0, 150.0)),
    ('130_far', 130, 257, 0, (-3000.5, 9000.25, 9500.0)),                # a centre far outside: the tile bound holds for any centre
    ('130_big', 130, 257, 7, (128.0, 65.0, 400.0)),                      # K = 401, rings beyond 145 empty
    ('1030', 1030, 1030, 2, (515.2, 514.9, 700.7)),                      # many workgroups, 701 rings, the corners cut them
]
SMALL = [g for g in GEOMETRIES if g[1] < 1000]
_reference = {}


def image_of(kind, h, w, circle):
    rng = np.random.default_rng([h, w, len(kind)])
    if kind == 'random':
        return rng.integers(0, 65536, (h, w)).astype(np.uint16)
    if kind == 'narrow':                                                 # a smooth disk: a ring's values share a high byte or two
        return (30000 + rng.integers(0, 300, (h, w))).astype(np.uint16)
    if kind == 'straddle':                                               # 0x00FF and 0x0100 alternating along every ring
        on, k, _ = fr.rings(h, w, circle)
        img = np.full((h, w), 0x0100, np.uint16)
        order = np.argsort(k[on], kind='stable')
        rank = np.empty(order.size, np.int64)
        ring_sorted = k[on][order]
        rank[order] = np.arange(order.size) - np.searchsorted(ring_sorted, ring_sorted)
        img[on] = np.where(rank % 2 == 0, 0x00FF, 0x0100)
        return img
    return np.full((h, w), int(kind), np.uint16)


def reference(kind, name, h, w, circle):
    key = (kind, name)
    if key not in _reference:
        img = image_of(kind, h, w, circle)
        img.setflags(write=False)
        _reference[key] = (img,) + fr.ring_medians(img, circle)
    return _reference[key]


@pytest.mark.parametrize('kind', ['random', 'narrow', 'straddle', '0', '65535', '4660'])
@pytest.mark.parametrize('geometry', SMALL, ids=[g[0] for g in SMALL])
def test_ring_medians_match_the_restatement(mods, geometry, kind):
    _, _, lib = mods
    name, h, w, extra, circle = geometry
    img, count, lo, hi = reference(kind, name, h, w, circle)
    st, g_count, g_lo, g_hi, intact = medians(lib, img, circle, extra)
    assert st == 0 and intact
    assert np.array_equal(g_count, count), np.flatnonzero(g_count != count)[:5]
    assert np.array_equal(g_lo, lo), (np.flatnonzero(g_lo != lo)[:5], g_lo[g_lo != lo][:5], lo[g_lo != lo][:5])
    assert np.array_equal(g_hi, hi), (np.flatnonzero(g_hi != hi)[:5], g_hi[g_hi != hi][:5], hi[g_hi != hi][:5])


@pytest.mark.parametrize('kind', ['random', 'narrow', '65535'])
def test_ring_medians_on_many_workgroups_and_rings(mods, kind):
    """1030 x 1030 around a circle of radius 700.7; all 65535: a 64 x 64 tile that holds one value counts 4096 in one 16-bit
    counter, and the select must leave bin 255 twice."""
    _, _, lib = mods
    name, h, w, extra, circle = GEOMETRIES[-1]
    img, count, lo, hi = reference(kind, name, h, w, circle)
    st, g_count, g_lo, g_hi, intact = medians(lib, img, circle, extra)
    assert st == 0 and intact and (count[-20:] > 0).any() and (count == 0).sum() == 0
    assert np.array_equal(g_count, count) and np.array_equal(g_lo, lo) and np.array_equal(g_hi, hi)


def test_the_planted_rings_are_what_they_claim(mods):
    """The cases the list above names, checked on the reference: a ring of one pixel, of two, of odd and of even count, an even ring
    whose middle pair straddles a high byte, empty rings."""
    by_name = {g[0]: g for g in GEOMETRIES}
    _, count, lo, hi = reference('straddle', '64_r13', *by_name['64_r13'][1:3], by_name['64_r13'][4])
    assert count[0] == 1 and (count % 2 == 1).any()
    even = (count % 2 == 0) & (count > 0)
    assert even.sum() > 3 and (lo[even] == 0x00FF).all() and (hi[even] == 0x0100).all()
    assert fr.ring_medians(np.zeros((64, 64), np.uint16), by_name['64_two_px'][4])[0][0] == 2
    assert (reference('random', '130_big', 130, 257, by_name['130_big'][4])[1][146:] == 0).all()
    assert reference('random', '1x1_off', 1, 1, by_name['1x1_off'][4])[1].sum() == 0


def test_ring_medians_do_not_depend_on_the_workspace_alignment(mods):
    _, _, lib = mods
    name, h, w, extra, circle = GEOMETRIES[14]
    img, count, lo, hi = reference('random', name, h, w, circle)
    for skew in (1, 16, 63):
        st, g_count, g_lo, g_hi, intact = medians(lib, img, circle, extra, ws_skew=skew)
        assert st == 0 and intact and np.array_equal(g_count, count) and np.array_equal(g_lo, lo) and np.array_equal(g_hi, hi)


def test_ops_ring_medians(mods):
    _, ops, _ = mods
    name, h, w, extra, circle = GEOMETRIES[15]
    img, count, lo, hi = reference('random', name, h, w, circle)
    view = padded(img, extra)[:, :w]
    got = ops.ring_medians_u16(view, circle)
    assert got[0].dtype == torch.uint32 and got[1].dtype == got[2].dtype == torch.uint16
    assert np.array_equal(got[0].view(torch.int32).cpu().numpy().view(np.uint32), count)
    assert np.array_equal(down16(got[1]), lo) and np.array_equal(down16(got[2]), hi)
    again = ops.ring_medians_u16(view, circle, out=got)
    assert again[0] is got[0] and np.array_equal(down16(again[2]), hi)
    with pytest.raises(ValueError):
        ops.ring_medians_u16(view, circle, out=(got[0][:-1], got[1], got[2]))
    with pytest.raises(ValueError):
        ops.ring_medians_u16(view, (1.0, 1.0, float('nan')))


# ---- flatten ----
def gains_of(kind, kk, seed):
    rng = np.random.default_rng([seed, kk])
    if kind == 'random':
        g = rng.uniform(0.0, 8.0, kk)
        for i in list(np.flatnonzero(rng.random(kk - 1) < 0.05)) + [kk // 3]:    # pairs of rings with gain 0: exact zeros in between
            g[i] = g[min(i + 1, kk - 1)] = 0.0
        return g
    if kind == 'half':                                                   # odd values times 0.5, 1.5, 2.5: ties of both parities
        return rng.choice([0.5, 1.5, 2.5], kk)
    return np.full(kk, float(kind))


def check_flatten(lib, img, circle, gain, extra, **how):
    want = fr.ring_flatten(img, circle, gain)
    st, got, intact = flattened(lib, img, circle, gain, extra, **how)
    assert st == 0 and intact
    bad = np.argwhere(got != want)
    assert bad.size == 0, '%d pixels differ, first at %s: %d vs %d' % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    return want


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('geometry', SMALL, ids=[g[0] for g in SMALL])
def test_ring_flatten_matches_the_restatement(mods, geometry, in_place):
    _, _, lib = mods
    name, h, w, extra, circle = geometry
    img, count = reference('random', name, h, w, circle)[:2]
    kk = fr.n_rings(circle)
    want = check_flatten(lib, img, circle, gains_of('random', kk, 1), extra, in_place=in_place, out_extra=(extra + 5) % 8)
    on = fr.rings(h, w, circle)[0]
    assert np.array_equal(want[~on], img[~on])
    if kk >= 40 and count[kk // 3] > 40:                                  # (pixels between the mid-radii of two rings of gain 0)
        assert (want[on] == 65535).any() and (want[on] == 0).any()        # saturation and gain 0 both occur


@pytest.mark.parametrize('kind', ['half', '1.0', '0.0', '8.0', '1e300'])
@pytest.mark.parametrize('name', ['64_r13_9', '130_frac_7', '130_corner64', '130_far'])
def test_ring_flatten_ties_saturation_and_zero(mods, name, kind):
    _, _, lib = mods
    _, h, w, extra, circle = {g[0]: g for g in GEOMETRIES}[name]
    img = reference('random', name, h, w, circle)[0] | np.uint16(1)       # odd values: v / 2 is a tie
    gain = gains_of(kind, fr.n_rings(circle), 2)
    want = check_flatten(lib, img, circle, gain, extra)
    on = fr.rings(h, w, circle)[0]
    if kind == 'half' and on.sum() > 50:
        prod = img[on].astype(np.float64) * 0.5
        assert (np.rint(prod) % 2 == 0).all() and (np.floor(prod) % 2 == 0).any() and (np.floor(prod) % 2 == 1).any()
    if kind == '1.0':
        assert np.array_equal(want, img)
    if kind == '1e300':
        assert (want[on] == 65535).all()


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
def test_ring_flatten_over_several_gain_windows(mods, in_place):
    """701 rings: three launches, each with its own 448 table intervals; aligned and unaligned rows."""
    _, _, lib = mods
    name, h, w, _, circle = GEOMETRIES[-1]
    img = reference('random', name, h, w, circle)[0]
    gain = gains_of('random', fr.n_rings(circle), 3)
    for extra, out_extra in ((2, 2), (6, 14), (1, 3)):                    # 1032 and 1036: 16-byte rows; 1031: element accesses
        check_flatten(lib, img, circle, gain, extra, in_place=in_place, out_extra=out_extra)


def test_ops_ring_flatten_and_flatten_disk(mods):
    flatten, ops, _ = mods
    img, circle = fr.synthetic_disk(0.004)
    want_flat, want_profile, want_gain = fr.flatten_disk(img, circle)
    dev = up16(img)
    flat, profile, gain = flatten.flatten_disk(dev, circle)
    for key in ('count', 'lo', 'hi', 'median', 'radius'):
        assert profile[key].dtype == want_profile[key].dtype and np.array_equal(profile[key], want_profile[key]), key
    assert np.array_equal(gain.view(np.uint64), want_gain.view(np.uint64))
    assert np.array_equal(down16(flat), want_flat) and np.array_equal(down16(dev), img)
    for smooth, level, max_gain in ((5, None, 8.0), (1, 20000.0, 1.5)):
        flat, _, gain = flatten.flatten_disk(dev, circle, smooth, level, max_gain)
        want_flat, _, want_gain = fr.flatten_disk(img, circle, smooth, level, max_gain)
        assert np.array_equal(gain.view(np.uint64), want_gain.view(np.uint64)) and np.array_equal(down16(flat), want_flat)
    same = ops.ring_flatten_u16(dev, circle, want_gain, out=dev)          # in place through the wrapper
    assert same is dev and np.array_equal(down16(dev), want_flat)
    with pytest.raises(ValueError, match='gain'):
        ops.ring_flatten_u16(dev, circle, want_gain[:-1])
    with pytest.raises(ValueError):
        ops.ring_flatten_u16(dev, circle, want_gain, out=dev[:-1])


# ---- refusals: the planted outputs stay as they are ----
def test_refused_arguments_leave_the_outputs_untouched(mods):
    _, _, lib = mods
    name, h, w, extra, circle = GEOMETRIES[15]
    img = reference('random', name, h, w, circle)[0]
    kk = fr.n_rings(circle)
    nan_c, far_c, neg_c, big_c = c3((float('nan'), 1.0, 5.0)), c3((65536.0, 1.0, 60.2)), c3((1.0, 1.0, -1.0)), c3((1.0, 1.0, 16384.0))
    bad_circles = [(nan_c.ctypes.data, kk), (far_c.ctypes.data, kk), (neg_c.ctypes.data, 0), (big_c.ctypes.data, 16385), (None, kk)]
    for over, code in ([(dict(h=0), E_UNSUPPORTED), (dict(w=16385), E_UNSUPPORTED), (dict(img_ptr=None), E_ARG), (dict(pitch=w - 1), E_ARG),
                        (dict(k=kk - 1), E_ARG), (dict(k=kk + 1), E_ARG), (dict(count=None), E_ARG), (dict(lo=None), E_ARG),
                        (dict(hi=None), E_ARG), (dict(ws=None), E_ARG),
                        (dict(ws_bytes=lib.shg_ring_medians_u16_workspace_bytes(kk) - 1), E_ARG)]
                       + [(dict(c3=p, k=k), E_ARG) for p, k in bad_circles]):
        st, _, _, _, intact = medians(lib, img, circle, extra, **dict(over))
        assert st == code and intact, over
    gain = np.ones(kk)
    for over, code in ([(dict(h=16385), E_UNSUPPORTED), (dict(w=0), E_UNSUPPORTED), (dict(img_ptr=None), E_ARG), (dict(pitch=w - 1), E_ARG),
                        (dict(out_pitch=w - 1), E_ARG), (dict(out=None), E_ARG), (dict(gain_ptr=None), E_ARG), (dict(k=kk - 1), E_ARG)]
                       + [(dict(c3=p, k=k), E_ARG) for p, k in bad_circles]):
        st, got, intact = flattened(lib, img, circle, gain, extra, **dict(over))
        assert st == code and intact and (got == OUT_FILL).all(), over
    for bad in (-0.5, float('nan'), float('inf')):
        g = gain.copy()
        g[kk // 2] = bad
        st, got, intact = flattened(lib, img, circle, g, extra)
        assert st == E_ARG and intact and (got == OUT_FILL).all(), bad
    # in place with another pitch: out is the image's own buffer
    src = padded(img, extra)
    circ = c3(circle)
    assert lib.shg_ring_flatten_u16(src.data_ptr(), h, w, w + extra, circ.ctypes.data, gain.ctypes.data, kk, src.data_ptr(), w, None) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(down16(src)[:, :w], img)


# ---- one scan ----
@pytest.fixture(scope='module')
def scan(mods, tmp_path_factory):
    """fr.pipeline_scan() on disk, the pipeline's own products of it, and flatten_scan's result."""
    from solex_ser_recon_en_amd import SHG_MAIN, outputs
    from solex_ser_recon_en_amd.png_io import read_png_gray
    flatten = mods[0]
    frames = fr.pipeline_scan()
    path = write_scan(tmp_path_factory, 'flatten', frames)
    products = tmp_path_factory.mktemp('flatten_products') / 'scan.ser'
    shutil.copy(path, products)
    assert SHG_MAIN.main([str(products)]) == 0
    outputs.flush()
    uncontrasted = read_png_gray(str(products)[:-4] + '_shift=0_uncontrasted.png')
    return {'frames': frames, 'path': path, 'uncontrasted': uncontrasted, 'res': flatten.flatten_scan(path)}


def test_flatten_scan_composes_the_stages_as_the_pipeline_does(mods, scan):
    res = scan['res']
    image = down16(res['image'])
    assert image.dtype == scan['uncontrasted'].dtype == np.uint16 and np.array_equal(image, scan['uncontrasted'])
    want_flat, want_profile, want_gain = fr.flatten_disk(image, res['circle'])
    assert np.array_equal(down16(res['flat']), want_flat)
    assert np.array_equal(res['gain'].view(np.uint64), want_gain.view(np.uint64))
    assert np.array_equal(res['profile']['median'], want_profile['median'])
    assert res['shift'] == 0 and res['level'] == float(np.median(want_profile['median'][:len(want_gain) // 10]))


def test_flatten_scan_at_another_shift_is_that_shifts_product(mods, scan, tmp_path):
    from solex_ser_recon_en_amd import SHG_MAIN, outputs
    from solex_ser_recon_en_amd.png_io import read_png_gray
    flatten = mods[0]
    work = tmp_path / 'scan.ser'
    shutil.copy(scan['path'], work)
    assert SHG_MAIN.main(['-w', '3', str(work)]) == 0
    outputs.flush()
    res = flatten.flatten_scan(str(work), shift=3)
    assert np.array_equal(down16(res['image']), read_png_gray(str(work)[:-4] + '_shift=3_uncontrasted.png'))
    assert np.array_equal(down16(res['flat']), fr.flatten_disk(down16(res['image']), res['circle'])[0])


def test_accuracy_on_the_pipelines_image(mods, scan):
    """The 'pipeline' bounds: measured here on the CPU, on the image and circle the pipeline oracle makes of the scan, printed, and
    held; then the same measures on what flatten_scan returned."""
    from oracle import pipeline_oracle as po
    r = po.run(scan['frames'], {})['results'][0]
    image, circle = r['cropped'], tuple(float(v) for v in r['cercle'])
    flat, profile, _ = fr.flatten_disk(image, circle)
    measured = (fr.profile_error(profile, circle[2]), fr.flatness(fr.profile_of(*fr.ring_medians(flat, circle))))
    res = scan['res']
    ours = (fr.profile_error(res['profile'], res['circle'][2]),
            fr.flatness(fr.profile_of(*fr.ring_medians(down16(res['flat']), res['circle']))))
    for who, (prof, flatness) in (('oracle', measured), ('flatten_scan', ours)):
        print('%s: profile core %.6f inner %.6f outer %.6f; flatness core %.6f inner %.6f outer %.6f' % ((who,) + prof + flatness))
        for got, bound in zip(prof, fr.TOLERANCE['pipeline']['profile']):
            assert got <= bound, (who, prof)
        for got, bound in zip(flatness, fr.TOLERANCE['pipeline']['flatness']):
            assert got <= bound, (who, flatness)
    assert np.allclose(res['circle'], circle, rtol=0, atol=1e-6)


def test_command_line(mods, scan, tmp_path, capsys):
    from solex_ser_recon_en_amd.fits_io import read_fits_u16
    from solex_ser_recon_en_amd.png_io import read_png_gray
    flatten = mods[0]
    work = tmp_path / 'scan.ser'
    shutil.copy(scan['path'], work)
    out = run_json(flatten.main, capsys, [str(work), '--contrast', '-f'])
    base = str(work)[:-4] + '_shift=0'
    assert out['png'] == base + '_flat.png' and out['fits'] == base + '_flat.fits' and out['clv'] == base + '_clv.txt'
    flat = down16(scan['res']['flat'])
    assert np.array_equal(read_png_gray(out['png']), flat) and np.array_equal(read_fits_u16(out['fits'])[0], flat)
    for suffix in ('_flat_clahe.png', '_flat_protus.png', '_flat_uncontrasted.png', '_flat_high_contrast.png', '_flat_clahe.fits'):
        assert os.path.exists(base + suffix), suffix
    assert np.array_equal(read_png_gray(base + '_flat_uncontrasted.png'), flat)
    res = scan['res']
    kk = len(res['gain'])
    assert out['rings'] == kk and out['shift'] == 0 and out['smooth'] == 1 and out['max_gain'] == 8.0 and out['shape'] == list(flat.shape)
    assert out['circle'] == list(res['circle']) and out['level'] == res['level'] and out['ratio'] == res['ratio']
    have = np.flatnonzero(res['profile']['count'])
    assert out['centre_median'] == res['profile']['median'][have[0]] and out['limb_median'] == res['profile']['median'][have[-1]]
    assert out['saturated'] == int(((flat == 65535) & (down16(res['image']) != 65535)).sum())
    rows = [line.split() for line in open(out['clv']) if not line.startswith('#')]
    assert len(rows) == kk and [int(r[0]) for r in rows] == list(range(kk))
    assert np.array_equal([int(r[2]) for r in rows], res['profile']['count'])
    assert np.array_equal([float(r[3]) for r in rows], res['profile']['median'])
    assert np.allclose([float(r[4]) for r in rows], res['gain'], rtol=1e-8) and np.allclose([float(r[1]) for r in rows], res['profile']['radius'] / res['circle'][2], atol=1e-6)
    # the SHG_MAIN flags reach the stages: mirrored and cropped square, five rings smoothed, the gain capped
    out = run_json(flatten.main, capsys, [str(work), '--smooth', '5', '--max-gain', '3', '-ms'])
    assert out['smooth'] == 5 and out['max_gain'] == 3.0 and out['fits'] is None and out['shape'] == [flat.shape[0]] * 2
    gains = [float(line.split()[4]) for line in open(out['clv']) if not line.startswith('#')]
    assert max(gains) == 3.0
    assert flatten.main([str(work), '-x']) == 1                           # no limb fit, no circle
    assert 'circle' in capsys.readouterr().err
