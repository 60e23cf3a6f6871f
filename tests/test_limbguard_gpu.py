"""Limb protection on the GPU: shg_limb_split_u16 and shg_limb_merge_u16 bit for bit against the restatement written from the header
(tests/limbguard_ref.py): images in buffers whose pitch exceeds the width with the padding planted and checked, outputs on and off
16 bytes with guard fills, one row, one column, several workgroups on both axes; circles inside the image, centred exactly on a
pixel, centred off the image, containing the whole image, of radius 2.5 with margin 1; margin 0, a reach of 1 and of rad - margin, a
blend of 2^-10 and of 100; random, zero, full-scale images and a disk on a sky of exactly 0; either plane left out; every refused
argument; protect with the identity; deconvolve_disk and sharpen_disk with limb= against the restatements composed; and a scan and a
PNG through deconvolve_scan, sharpen_scan and the two command lines."""
import os
import shutil

import numpy as np
import pytest

from solex_ser_recon_en_amd import limbguard as _limbguard  # noqa: F401  (no feature: no tests)
from tests import deconvolve_ref as dr
from tests import flatten_ref as fr
from tests import limbguard_ref as lr
from tests import sharpen_ref as sr
from tests.linemaps_util import run_json, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
PAD, FILL = 0xBEEF, 0x5A5A
SHAPES = [(1, 9), (9, 1), (7, 5), (33, 257), (70, 130), (300, 520)]


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import deconvolve, limbguard, ops, sharpen
    from solex_ser_recon_en_amd._lib import lib
    return {'deconvolve': deconvolve, 'sharpen': sharpen, 'limbguard': limbguard, 'ops': ops, 'lib': lib}


def up16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.uint16)


def down16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def scramble(plane):
    """A stand-in for a filter: every value changed, deterministically."""
    return (plane.astype(np.uint32) * 40503 + 12345 & 0xFFFF).astype(np.uint16)


class Plane:
    """An [h, w] image inside a flat device buffer: `skew` elements in, rows `pitch` apart, everything else planted with `fill`.
    aligned: every row starts on 16 bytes (the kernels' 16-byte path); else the pitch is odd and the start two bytes off."""
    def __init__(self, h, w, aligned, fill, img=None, extra=3):
        self.h, self.w, self.fill = h, w, fill
        self.pitch = w + (-w) % 8 + 8 if aligned else w + extra + (w + extra + 1) % 2
        self.skew = 0 if aligned else 1
        host = np.full(h * self.pitch + self.skew + 8, fill, np.uint16)
        if img is not None:
            host[self.skew:self.skew + h * self.pitch].reshape(h, self.pitch)[:, :w] = img
        self.buf = up16(host)
        self.ptr = self.buf.data_ptr() + 2 * self.skew
        assert (self.ptr % 16 == 0 and self.pitch % 8 == 0) == bool(aligned)

    def read(self):
        """(the image, whether everything around it still holds the fill)."""
        got = down16(self.buf)
        rows = got[self.skew:self.skew + self.h * self.pitch].reshape(self.h, self.pitch)
        around = (got[:self.skew] == self.fill).all() and (got[self.skew + (self.h - 1) * self.pitch + self.w:] == self.fill).all()
        return rows[:, :self.w].copy(), bool(around and (rows[:-1, self.w:] == self.fill).all())

    def untouched(self):
        return bool((down16(self.buf) == self.fill).all())


def c3(circle):
    return np.ascontiguousarray(circle, dtype=np.float64)


def run_split(lib, img, circle, margin, reach, aligned=False, want=(True, True), **over):
    """shg_limb_split_u16 on the image in a padded buffer into planted planes -> (status, inner or None, outer or None, whether the
    image, the padding and the guards are as they were -- and, after a refusal, the planes too)."""
    h, w = img.shape
    src = Plane(h, w, aligned, PAD, img)
    inner, outer = Plane(h, w, aligned, FILL, extra=1), Plane(h, w, aligned, FILL, extra=5)
    circle = c3(circle)
    st = lib.shg_limb_split_u16(over.get('img_ptr', src.ptr), over.get('h', h), over.get('w', w), over.get('pitch', src.pitch),
                                over.get('circle_ptr', circle.ctypes.data), margin, reach, over.get('inner', inner.ptr if want[0] else None),
                                over.get('inner_pitch', inner.pitch), over.get('outer', outer.ptr if want[1] else None),
                                over.get('outer_pitch', outer.pitch), None)
    torch.cuda.synchronize()
    back, intact = src.read()
    intact = intact and np.array_equal(back, img)
    got = []
    for plane, wanted in ((inner, want[0]), (outer, want[1])):
        if st != 0 or not wanted:
            intact = intact and plane.untouched()
            got.append(None)
        else:
            values, around = plane.read()
            intact = intact and around
            got.append(values)
    return st, got[0], got[1], bool(intact)


def run_merge(lib, img, disk, sky, circle, margin, blend, aligned=False, **over):
    """shg_limb_merge_u16 likewise -> (status, out or None, intact)."""
    h, w = img.shape
    src, dsk = Plane(h, w, aligned, PAD, img), Plane(h, w, aligned, PAD, disk, extra=1)
    sk = None if sky is None else Plane(h, w, aligned, PAD, sky, extra=5)
    out = Plane(h, w, aligned, FILL, extra=7)
    circle = c3(circle)
    st = lib.shg_limb_merge_u16(over.get('img_ptr', src.ptr), over.get('pitch', src.pitch), over.get('disk_ptr', dsk.ptr), over.get('disk_pitch', dsk.pitch),
                                over.get('sky_ptr', None if sk is None else sk.ptr), over.get('sky_pitch', 0 if sk is None else sk.pitch),
                                over.get('h', h), over.get('w', w), over.get('circle_ptr', circle.ctypes.data), margin, blend,
                                over.get('out', out.ptr), over.get('out_pitch', out.pitch), None)
    torch.cuda.synchronize()
    intact = True
    for plane, values in ((src, img), (dsk, disk), (sk, sky)):
        if plane is not None:
            back, around = plane.read()
            intact = intact and around and np.array_equal(back, values)
    if st != 0:
        return st, None, bool(intact and out.untouched())
    got, around = out.read()
    return st, got, bool(intact and around)


def same(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, '%s: %d pixels differ, first at %s: %d vs %d' % (what, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def circles(h, w):
    """name -> (circle, the margins to try)."""
    m = min(h, w)
    rad = max(2.6, 0.31 * m + 0.4)
    far = (-0.3 * w - 3.5, 1.2 * h + 2.25)
    return {'inside': ((0.47 * w + 0.3, 0.52 * h + 0.1, rad), (0.0, min(2.75, rad - 1.0))),
            'on a pixel': ((float(w // 2), float(h // 2), max(3.5, 0.25 * m + 0.5)), (0.0, 1.5)),
            'off the image': ((far[0], far[1], float(np.hypot(w / 2 - far[0], h / 2 - far[1])) + 0.3), (0.0, 3.25)),
            'contains the image': ((0.5 * w + 0.3, 0.5 * h - 0.2, 2.0 * (h + w) + 0.5), (0.0, 6.0)),
            'small': ((min(w - 1, 3) + 0.25, min(h - 1, 2) + 0.5, 2.5), (1.0,))}


def images(h, w):
    rng = np.random.default_rng([h, w, 22])
    return {'random': rng.integers(0, 65536, (h, w)).astype(np.uint16), 'zeros': np.zeros((h, w), np.uint16),
            'full': np.full((h, w), 65535, np.uint16), 'disk': dr.zero_sky_disk(h, w),
            'halves': np.where(np.add.outer(np.arange(h), np.arange(w)) % 7 < 3, 65535, 0).astype(np.uint16)}


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_split_and_merge_match_the_restatement(mods, shape):
    """Every circle with every margin; the reach (1, rad - margin, in between), the blend (2^-10, 100, 3.3), the image, the layout and
    the plane left out take turns.  The merge takes scrambled planes, so that nothing it blends equals the image."""
    lib = mods['lib']
    h, w = shape
    pictures = images(h, w)
    turn = SHAPES.index(shape)
    for name, (circle, margins) in circles(h, w).items():
        for margin in margins:
            edge = circle[2] - margin
            for k, (reach, blend) in enumerate(((1.0, 2.0 ** -10), (edge, 100.0), (min(edge, 1.0 + 0.37 * edge), 3.3))):
                turn += 1
                picture = list(pictures)[turn % len(pictures)]
                img = pictures[picture]
                aligned = turn % 2 == 0
                want = ((True, True), (True, False), (False, True), (True, True))[turn % 4]
                what = '%s, %s, margin %g, reach %g, blend %g, aligned %s' % (name, picture, margin, reach, blend, aligned)
                ref_inner, ref_outer = lr.split(img, circle, margin, reach)
                st, inner, outer, intact = run_split(lib, img, circle, margin, reach, aligned, want)
                assert st == 0 and intact, what
                if want[0]:
                    same(inner, ref_inner, what + ' (inner)')
                if want[1]:
                    same(outer, ref_outer, what + ' (outer)')
                if name == 'contains the image':
                    assert np.array_equal(ref_inner, img)
                disk, sky = scramble(ref_inner), (scramble(ref_outer) if want[1] else None)
                st, out, intact = run_merge(lib, img, disk, sky, circle, margin, blend, aligned)
                assert st == 0 and intact, what
                same(out, lr.merge(img, disk, sky, circle, margin, blend), what + ' (merge)')
                band, disk_full, sky_full = lr.regions(img.shape, circle, margin, blend)
                assert np.array_equal(out[band], img[band]) and np.array_equal(out[disk_full], disk[disk_full]), what
                if sky is not None:
                    assert np.array_equal(out[sky_full], sky[sky_full]), what


def test_the_clamp_at_both_ends_and_the_zero_ray(mods):
    """Full scale beside zero: 2 s - m leaves [0, 65535] both ways and is clipped; the pixel the circle is centred on takes the ray
    (1, 0)."""
    lib = mods['lib']
    h, w = 70, 130
    step = np.where(np.arange(w)[None, :] < 66, 65535, 0).astype(np.uint16) + np.zeros((h, 1), np.uint16)
    circle = (65.0, 35.0, 20.0)
    ref_inner, ref_outer = lr.split(step, circle, 0.0, 10.0)
    rho = lr.rays(h, w, circle)[0]
    assert rho[35, 65] == 0.0 and ref_outer[35, 65] != step[35, 65]
    for plane in (ref_inner, ref_outer):
        assert plane.max() == 65535 and plane.min() == 0
    for aligned in (False, True):
        st, inner, outer, intact = run_split(lib, step, circle, 0.0, 10.0, aligned)
        assert st == 0 and intact
        same(inner, ref_inner, 'inner')
        same(outer, ref_outer, 'outer')


def test_refusals_leave_everything_untouched(mods):
    lib, ops = mods['lib'], mods['ops']
    img = images(20, 22)['random']
    circle = (10.5, 9.25, 7.0)
    nan, inf = float('nan'), float('inf')
    bad_circles = [c3(v) for v in ((nan, 9.0, 7.0), (10.0, inf, 7.0), (10.0, 9.0, nan), (10.0, 9.0, 0.0), (10.0, 9.0, -7.0), (10.0, 9.0, 16384.0),
                                   (65536.0, 9.0, 7.0), (10.0, 9.0, 2.9))]

    def split_refused(code, margin=2.0, reach=3.0, **over):
        st, _, _, intact = run_split(lib, img, circle, margin, reach, **over)
        assert st == code and intact, (margin, reach, over)

    def merge_refused(code, margin=2.0, blend=3.0, sky=img, **over):
        st, _, intact = run_merge(lib, img, img, sky, circle, margin, blend, **over)
        assert st == code and intact, (margin, blend, over)

    for refused in (split_refused, merge_refused):
        for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
            refused(E_UNSUPPORTED, **over)
        for over in [dict(img_ptr=None), dict(circle_ptr=None), dict(pitch=21), dict(margin=-1.0), dict(margin=nan), dict(margin=inf), dict(margin=6.5)] + \
                [dict(circle_ptr=c.ctypes.data) for c in bad_circles]:
            refused(E_ARG, **over)
    for over in (dict(want=(False, False)), dict(inner_pitch=21), dict(outer_pitch=21), dict(reach=0.5), dict(reach=5.5), dict(reach=nan),
                 dict(reach=inf), dict(reach=-1.0)):
        split_refused(E_ARG, **over)
    for over in (dict(disk_ptr=None), dict(out=None), dict(disk_pitch=21), dict(sky_pitch=21), dict(out_pitch=21), dict(blend=0.0), dict(blend=-2.0),
                 dict(blend=nan), dict(blend=inf)):
        merge_refused(E_ARG, **over)
    # an output on an input, on its last element, and on the other output
    a, b, c, d = (Plane(20, 22, False, FILL) for _ in range(4))
    last = 2 * (19 * a.pitch + 21)
    ring = c3(circle)
    for inner, outer in ((a.ptr, c.ptr), (a.ptr + last, c.ptr), (b.ptr, a.ptr - last), (b.ptr, b.ptr), (b.ptr, b.ptr + last), (b.ptr - last, b.ptr),
                         (None, a.ptr), (a.ptr + last, None)):
        assert lib.shg_limb_split_u16(a.ptr, 20, 22, a.pitch, ring.ctypes.data, 2.0, 3.0, inner, a.pitch, outer, a.pitch, None) == E_ARG
    for out in (a.ptr, a.ptr + last, b.ptr - last, b.ptr, c.ptr + last, c.ptr - last):
        assert lib.shg_limb_merge_u16(a.ptr, a.pitch, b.ptr, a.pitch, c.ptr, a.pitch, 20, 22, ring.ctypes.data, 2.0, 3.0, out, a.pitch, None) == E_ARG
    assert lib.shg_limb_merge_u16(a.ptr, a.pitch, b.ptr, a.pitch, None, 0, 20, 22, ring.ctypes.data, 2.0, 3.0, b.ptr + last, a.pitch, None) == E_ARG
    torch.cuda.synchronize()
    assert all(p.untouched() for p in (a, b, c, d))
    # the wrappers: a ValueError before the call, the overlap a RuntimeError
    dev = up16(img)
    for bad in (dict(circle=(1.0, 2.0)), dict(circle=(1.0, nan, 7.0)), dict(margin=-1.0), dict(margin=6.5), dict(margin='wide'), dict(reach=0.5),
                dict(reach=5.5), dict(want_inner=False, want_outer=False), dict(inner=dev[:-1]), dict(outer=dev[:, :-1])):
        with pytest.raises(ValueError):
            ops.limb_split_u16(dev, bad.pop('circle', circle), bad.pop('margin', 2.0), bad.pop('reach', 3.0), **bad)
    for bad in (dict(circle=(1.0, 2.0, 0.0)), dict(margin=6.5), dict(blend=0.0), dict(blend=nan), dict(disk=dev[:-1]), dict(sky=dev[:, :-1]),
                dict(out=dev[:-1])):
        with pytest.raises(ValueError):
            ops.limb_merge_u16(dev, bad.pop('disk', dev), bad.pop('sky', dev), bad.pop('circle', circle), bad.pop('margin', 2.0),
                               bad.pop('blend', 3.0), **bad)
    with pytest.raises(RuntimeError, match='overlaps'):
        ops.limb_split_u16(dev, circle, 2.0, 3.0, inner=dev)
    with pytest.raises(RuntimeError, match='overlaps'):
        ops.limb_merge_u16(dev, dev.clone(), None, circle, 2.0, 3.0, out=dev)
    with pytest.raises(RuntimeError):
        ops.limb_split_u16(torch.zeros((4, 4), dtype=torch.uint16), circle, 2.0, 3.0)
    assert np.array_equal(down16(dev), img)


# ---- the Python layer ----
def test_wrappers_and_protect(mods):
    ops, limbguard = mods['ops'], mods['limbguard']
    img = images(70, 130)['random']
    circle = (61.4, 36.3, 22.1)
    dev = up16(img)
    inner, outer = ops.limb_split_u16(dev, circle, 2.5, 9.0)
    ref_inner, ref_outer = lr.split(img, circle, 2.5, 9.0)
    assert np.array_equal(down16(inner), ref_inner) and np.array_equal(down16(outer), ref_outer)
    mine = ops.pitched_u16(70, 130, 'cuda', 8)
    got = ops.limb_split_u16(dev, circle, 2.5, 9.0, outer=mine, want_inner=False)
    assert got[0] is None and got[1] is mine and np.array_equal(down16(mine), ref_outer)
    out = ops.limb_merge_u16(dev, up16(scramble(ref_inner)), None, circle, 2.5, 3.0, out=mine)
    assert out is mine and np.array_equal(down16(out), lr.merge(img, scramble(ref_inner), None, circle, 2.5, 3.0))
    # a process that returns its input gives the image back, bit for bit
    seen = []
    for sky in (True, False):
        out, rec = limbguard.protect(dev, circle, lambda p: (seen.append(down16(p)), p)[1], 2.5, 3.0, 9.0, sky)
        assert np.array_equal(down16(out), img)
        assert rec == {'circle': list(circle), 'margin': 2.5, 'blend': 3.0, 'reach': 9.0, 'sky': sky}
    assert len(seen) == 3 and np.array_equal(seen[0], ref_inner) and np.array_equal(seen[1], ref_outer) and np.array_equal(seen[2], ref_inner)
    # reach is clipped to rad - margin; a host image is taken as well
    out, rec = limbguard.protect(img, circle, lambda p: up16(scramble(down16(p))), 2.5, 3.0, 64.0)
    assert rec['reach'] == 22.1 - 2.5
    assert np.array_equal(down16(out), lr.protect(img, circle, scramble, 2.5, 3.0, 64.0))


def test_the_disk_calls_with_limb_are_the_restatements_composed(mods):
    deconvolve, sharpen = mods['deconvolve'], mods['sharpen']
    circle = sr.scene()[2]
    img, _, _ = dr.scene()
    dev = up16(img)
    taps = dr.gaussian(1.5, 6)

    def rl(iterations):
        return lambda plane: dr.deconvolve(plane, taps, iterations)[0]

    out, rec = deconvolve.deconvolve_disk(dev, 1.5, 5, radius=6, limb={'circle': circle})
    assert rec['limb'] == {'circle': list(circle), 'margin': 6.0, 'blend': 4.0, 'reach': 32.0, 'sky': True} and rec['iterations'] == 5
    assert np.array_equal(down16(out), lr.protect(img, circle, rl(5), 6.0, 4.0, 32.0))
    out, rec = deconvolve.deconvolve_disk(dev, taps=taps, iterations=3, limb={'circle': circle, 'margin': 4.5, 'blend': 2.0, 'reach': 500, 'sky': False})
    assert rec['limb'] == {'circle': list(circle), 'margin': 4.5, 'blend': 2.0, 'reach': circle[2] - 4.5, 'sky': False}
    assert np.array_equal(down16(out), lr.protect(img, circle, rl(3), 4.5, 2.0, 500.0, sky=False))
    plain, rec = deconvolve.deconvolve_disk(dev, 1.5, 5, radius=6)
    assert 'limb' not in rec and np.array_equal(down16(plain), dr.deconvolve(img, taps, 5)[0])
    # sharpen: the noise measured once, on the image itself
    gain_q8, thr = lr.sharpen_arguments(img, circle)
    out, rec = sharpen.sharpen_disk(dev, sharpen.DEFAULT_GAINS, sharpen.DEFAULT_DENOISE, circle=circle, limb={})
    assert rec['limb'] == {'circle': list(circle), 'margin': 6.0, 'blend': 4.0, 'reach': 32.0, 'sky': True} and rec['threshold_q6'] == thr.tolist()
    assert np.array_equal(down16(out), lr.protect(img, circle, lambda p: sr.sharpen(p, gain_q8, thr)[0], 6.0, 4.0, 32.0))
    noisy, _, _ = dr.scene(dr.NOISE)
    gain_q8, thr = lr.sharpen_arguments(noisy, circle)
    assert thr[0] > 0
    out, rec = sharpen.sharpen_disk(up16(noisy), sharpen.DEFAULT_GAINS, sharpen.DEFAULT_DENOISE, circle=circle, limb={'margin': 8, 'sky': False})
    assert rec['threshold_q6'] == thr.tolist() and rec['limb']['margin'] == 8.0 and rec['limb']['sky'] is False
    assert np.array_equal(down16(out), lr.protect(noisy, circle, lambda p: sr.sharpen(p, gain_q8, thr)[0], 8.0, 4.0, 32.0, sky=False))
    plain, rec = sharpen.sharpen_disk(dev, sharpen.DEFAULT_GAINS, sharpen.DEFAULT_DENOISE, circle=circle)
    assert 'limb' not in rec
    for bad in ({}, {'circle': (-1, -1, -1)}, {'circle': circle, 'margin': -1}, {'circle': circle, 'edge': 1}):
        with pytest.raises(ValueError):
            deconvolve.deconvolve_disk(dev, 1.5, 5, radius=6, limb=bad)
    with pytest.raises(ValueError):
        sharpen.sharpen_disk(dev, sharpen.DEFAULT_GAINS, limb={})
    # the gain the restatement measures is the GPU's
    got = lr.scene_measures(
        lambda im, k, n, limb: down16(deconvolve.deconvolve_disk(up16(im), taps=k, iterations=n, limb=limb)[0]),
        lambda im, ring, limb: down16(sharpen.sharpen_disk(up16(im), sharpen.DEFAULT_GAINS, sharpen.DEFAULT_DENOISE, circle=ring, limb=limb)[0]))
    print('inner %.6f, sky %.6f, noisy inner %.6f, noisy sky %.6f, sharpen %.6f' % tuple(got[k] for k in ('inner', 'sky', 'noisy_inner', 'noisy_sky', 'sharpen')))
    for key in lr.TOLERANCE:
        assert got[key] <= lr.TOLERANCE[key], key
    for key in lr.HARD:
        assert got[key] < lr.HARD[key], key


# ---- end to end: a scan, and a PNG ----
@pytest.fixture(scope='module')
def scan(mods, tmp_path_factory):
    from solex_ser_recon_en_amd import disk
    path = write_scan(tmp_path_factory, 'limbguard', fr.pipeline_scan())
    own = disk.scan_disk(path)
    return {'path': path, 'image': down16(own['image']), 'circle': own['circle']}


def band_of(scan, margin):
    return lr.regions(scan['image'].shape, scan['circle'], margin, 4.0)[0]


def test_scans_with_limb_and_without(mods, scan):
    deconvolve, sharpen = mods['deconvolve'], mods['sharpen']
    image, circle = scan['image'], scan['circle']
    taps = deconvolve.gaussian_taps(1.2)
    res = deconvolve.deconvolve_scan(scan['path'], iterations=3, limb={})
    assert np.array_equal(down16(res['image']), image) and res['circle'] == circle
    assert res['record']['limb'] == {'circle': list(circle), 'margin': 5.0, 'blend': 4.0, 'reach': min(32.0, circle[2] - 5.0), 'sky': True}
    want = lr.protect(image, circle, lambda p: dr.deconvolve(p, taps, 3)[0], 5.0, 4.0, 32.0)
    band = band_of(scan, 5.0)
    assert np.array_equal(down16(res['deconv']), want) and band.sum() > 100 and np.array_equal(want[band], image[band])
    plain = deconvolve.deconvolve_scan(scan['path'], iterations=3)
    assert 'limb' not in plain['record'] and np.array_equal(down16(plain['deconv']), dr.deconvolve(image, taps, 3)[0])
    assert (down16(plain['deconv'])[band] != image[band]).any()
    res = sharpen.sharpen_scan(scan['path'], limb={'margin': 7.5, 'sky': False})
    rec = res['record']
    assert rec['limb'] == {'circle': list(circle), 'margin': 7.5, 'blend': 4.0, 'reach': min(32.0, circle[2] - 7.5), 'sky': False}
    plain = sharpen.sharpen_scan(scan['path'])
    assert 'limb' not in plain['record'] and plain['record']['threshold_q6'] == rec['threshold_q6']
    process = lambda p: sr.sharpen(p, rec['gain_q8'], rec['threshold_q6'])[0]                 # noqa: E731
    assert np.array_equal(down16(plain['sharp']), process(image))
    want = lr.protect(image, circle, process, 7.5, 4.0, 32.0, sky=False)
    band = band_of(scan, 7.5)
    assert np.array_equal(down16(res['sharp']), want) and np.array_equal(want[band], image[band])
    rho = lr.rays(image.shape[0], image.shape[1], circle)[0]
    assert np.array_equal(want[rho >= circle[2] - 7.5], image[rho >= circle[2] - 7.5])
    for call in (deconvolve.deconvolve_scan, sharpen.sharpen_scan):
        with pytest.raises(ValueError, match='its own limb fit'):
            call(scan['path'], limb={'circle': circle})


def test_command_lines(mods, scan, tmp_path, capsys):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.png_io import read_png_gray, write_png
    deconvolve, sharpen = mods['deconvolve'], mods['sharpen']
    image, circle = scan['image'], scan['circle']
    work = str(tmp_path / 'scan.ser')
    shutil.copy(scan['path'], work)
    k = SHG_MAIN.default_options()['img_rotate'] // 90
    taps = deconvolve.gaussian_taps(1.2)
    # a scan: the limb fit is the circle
    out = run_json(deconvolve.main, capsys, [work, '--iterations', '3', '--limb-protect'])
    assert out['png'] == work[:-4] + '_shift=0_deconv.png' and out['fits'] is None and out['circle'] == list(circle)
    assert out['limb'] == {'circle': list(circle), 'margin': 5.0, 'blend': 4.0, 'reach': min(32.0, circle[2] - 5.0), 'sky': True}
    want = lr.protect(image, circle, lambda p: dr.deconvolve(p, taps, 3)[0], 5.0, 4.0, 32.0)
    got = read_png_gray(out['png'])
    band = np.rot90(band_of(scan, 5.0), k)
    assert np.array_equal(got, np.rot90(want, k)) and np.array_equal(got[band], np.rot90(image, k)[band])
    plain = run_json(deconvolve.main, capsys, [work, '--iterations', '3'])
    assert 'limb' not in plain and plain['png'] == out['png'] and sorted(set(out) - set(plain)) == ['limb']
    assert np.array_equal(read_png_gray(plain['png']), np.rot90(dr.deconvolve(image, taps, 3)[0], k))
    out = run_json(sharpen.main, capsys, [work, '--limb-protect', '7.5', '--limb-blend', '2', '--limb-reach', '12', '--limb-disk-only'])
    assert out['png'] == work[:-4] + '_shift=0_sharp.png'
    assert out['limb'] == {'circle': list(circle), 'margin': 7.5, 'blend': 2.0, 'reach': 12.0, 'sky': False}
    got = read_png_gray(out['png'])
    band = np.rot90(lr.rays(image.shape[0], image.shape[1], circle)[0] >= circle[2] - 7.5, k)
    assert np.array_equal(got[band], np.rot90(image, k)[band]) and (got != np.rot90(image, k)).any()
    plain = run_json(sharpen.main, capsys, [work])
    assert 'limb' not in plain and sorted(set(out) - set(plain)) == ['limb']
    assert np.array_equal(read_png_gray(plain['png']), np.rot90(down16(sharpen.sharpen_scan(work)['sharp']), k))
    # a PNG with --circle
    png = str(tmp_path / 'disk_stack.png')
    write_png(png, image, 0)
    out = run_json(deconvolve.main, capsys, [png, '--iterations', '2', '--circle', ','.join(repr(v) for v in circle), '--limb-protect=4.5'])
    assert out['png'] == png[:-4] + '_deconv.png' and out['circle'] == list(circle) and out['limb']['margin'] == 4.5
    got = read_png_gray(out['png'])
    band = lr.regions(image.shape, circle, 4.5, 4.0)[0]
    assert np.array_equal(got, lr.protect(image, circle, lambda p: dr.deconvolve(p, taps, 2)[0], 4.5, 4.0, 32.0))
    assert np.array_equal(got[band], image[band])
    plain = run_json(deconvolve.main, capsys, [png, '--iterations', '2'])
    assert 'limb' not in plain and plain['circle'] == [-1, -1, -1] and np.array_equal(read_png_gray(plain['png']), dr.deconvolve(image, taps, 2)[0])
    out = run_json(sharpen.main, capsys, [png, '--circle', ','.join(repr(v) for v in circle), '--sigma', '100', '--limb-protect'])
    assert out['png'] == png[:-4] + '_sharp.png' and out['limb'] == {'circle': list(circle), 'margin': 6.0, 'blend': 4.0, 'reach': min(32.0, circle[2] - 6.0), 'sky': True}
    got = read_png_gray(out['png'])
    band = lr.regions(image.shape, circle, 6.0, 4.0)[0]
    assert np.array_equal(got[band], image[band]) and (got != image).any()
    assert os.path.exists(out['png'])
    # --circle with a scan stays an error
    for main in (deconvolve.main, sharpen.main):
        assert main([work, '--circle', '50,50,40', '--limb-protect']) == 1
        assert '--circle goes with a PNG' in capsys.readouterr().err
