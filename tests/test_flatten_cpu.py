"""Flattening the disk, without a GPU: the restatement's own invariants (tests/flatten_ref.py), the accuracy it reaches on a
synthetic disk of the scenes' law -- re-measured here, printed, and held to flatten_ref.TOLERANCE --, flatten.gain_from_profile
against its restatement bit for bit, the workspace query, the argument refusals that need no device, and flatten_scan's refusals."""
import ctypes

import numpy as np
import pytest

from tests import flatten_ref as fr

E_ARG, E_UNSUPPORTED = -1, -3


# ---- the restatement's invariants ----
CIRCLES = [(20.0, 15.0, 13.0), (20.3, 15.7, 12.2), (-5.5, 40.25, 30.9), (3.0, 3.0, 0.4), (20.0, 15.0, 60.5)]


@pytest.mark.parametrize('circle', CIRCLES)
def test_counts_sum_to_the_disk_and_lo_is_below_hi(circle):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 65536, (31, 43)).astype(np.uint16)
    on, k, d2 = fr.rings(*img.shape, circle)
    count, lo, hi = fr.ring_medians(img, circle)
    assert count.shape == lo.shape == hi.shape == (fr.n_rings(circle),)
    assert int(count.sum()) == int(on.sum())
    assert (lo <= hi).all()
    assert (lo[count == 0] == 0).all() and (hi[count == 0] == 0).all()
    for i in np.flatnonzero(count):                       # against np.median, which averages the middle pair of an even count
        assert (float(lo[i]) + float(hi[i])) / 2.0 == np.median(img[on & (k == i)])


def test_the_ring_needs_no_square_root():
    """Pythagorean pixels sit exactly on a ring boundary: (3, 4) is in ring 5, and on the disk of radius 5 but not just inside it."""
    on, k, _ = fr.rings(40, 40, (20.0, 20.0, 13.0))
    for dx, dy, ring in ((3, 4, 5), (6, 8, 10), (5, 12, 13), (0, 0, 0), (1, 0, 1), (1, 1, 1), (2, 2, 2), (3, 3, 4)):
        assert k[20 + dy, 20 + dx] == ring and k[20 - dx, 20 + dy] == ring
    assert on[20 + 12, 20 + 5] and not on[20 + 12, 20 + 6]
    inside = fr.rings(40, 40, (20.0, 20.0, np.nextafter(13.0, 0.0)))[0]
    assert not inside[20 + 12, 20 + 5] and inside[20 + 12, 20 + 4]


@pytest.mark.parametrize('value', [0, 1, 255, 256, 40000, 65535])
def test_a_constant_image_has_that_median_in_every_ring(value):
    circle = (20.3, 15.7, 12.2)
    count, lo, hi = fr.ring_medians(np.full((31, 43), value, np.uint16), circle)
    assert (count > 0).all() and (lo == value).all() and (hi == value).all()


@pytest.mark.parametrize('circle', CIRCLES)
def test_a_gain_of_ones_is_the_identity(circle):
    img = np.random.default_rng(2).integers(0, 65536, (31, 43)).astype(np.uint16)
    assert np.array_equal(fr.ring_flatten(img, circle, np.ones(fr.n_rings(circle))), img)


def test_flatten_interpolates_between_the_rings_mid_radii():
    """gain[k] stands for the radius k + 1/2: a pixel at distance 2 reads halfway between gain[1] and gain[2]; the centre pixel and
    everything from K - 1/2 outwards read the end values; off the disk nothing changes."""
    circle = (10.0, 10.0, 4.0)                              # K = 5
    gain = np.array([2.0, 1.0, 3.0, 0.5, 0.25])
    img = np.full((21, 21), 1000, np.uint16)
    out = fr.ring_flatten(img, circle, gain)
    assert out[10, 10] == 2000 and out[10, 12] == 2000 and out[10, 11] == 1500      # u = -0.5, 1.5, 0.5
    assert out[10, 14] == 375 and out[10, 15] == 1000                                # u = 3.5 = K - 1.5: between 0.5 and 0.25; off
    out = fr.ring_flatten(img, (10.0, 10.0, 4.9), gain)
    u = np.sqrt(18.0) - 0.5                                                          # (3, 3): u = 3.74, below K - 1 = 4
    assert out[14, 10] == 375 and out[13, 13] == np.rint(1000 * (0.5 + (0.25 - 0.5) * (u - 3.0))) == 314
    out = fr.ring_flatten(img, (10.0, 10.0, 2.9), [1.0, 2.0, 4.0])                   # K = 3; (2, 2): u = 2.33 >= K - 1: the last gain
    assert out[12, 12] == 4000 and out[10, 12] == 3000 and out[13, 12] == 1000


def test_flatten_rounds_ties_to_even_and_saturates():
    circle = (1.0, 1.0, 0.5)                               # K = 1: one gain for the centre pixel
    img = np.array([[7, 7, 7], [7, 5, 7], [7, 7, 7]], np.uint16)
    assert fr.ring_flatten(img, circle, [0.5])[1, 1] == 2 and fr.ring_flatten(img + 2, circle, [0.5])[1, 1] == 4       # 2.5, 3.5
    assert fr.ring_flatten(img, circle, [20000.0])[1, 1] == 65535 and fr.ring_flatten(img, circle, [0.0])[1, 1] == 0
    assert (fr.ring_flatten(img, circle, [3.0])[[0, 0, 2], [0, 1, 2]] == 7).all()


# ---- the accuracy, re-measured ----
@pytest.mark.parametrize('noise', [0.0, 0.004])
def test_accuracy_on_the_synthetic_disk(noise):
    """Profile against the law and flatness of the flat image's ring medians over rings 4 .. K - 3; the innermost four and the last
    two rings apart (printed and bounded too): 6 of 121 rings are outside the core."""
    img, circle = fr.synthetic_disk(noise)
    flat, profile, gain = fr.flatten_disk(img, circle)
    kk = gain.shape[0]
    assert kk == 121 and fr.INNER + fr.OUTER <= 6
    assert (profile['count'][:fr.INNER] >= 4).all() and (profile['count'][:fr.INNER] <= 22).all()
    prof = fr.profile_error(profile, circle[2], fr.SCENE['scale'])
    flatness = fr.flatness(fr.profile_of(*fr.ring_medians(flat, circle)))
    print('noise %g: profile core %.6f inner %.6f outer %.6f; flatness core %.6f inner %.6f outer %.6f'
          % ((noise,) + prof + flatness))
    for got, bound in zip(prof, fr.TOLERANCE['profile'][noise]):
        assert got <= bound, (prof, fr.TOLERANCE['profile'][noise])
    for got, bound in zip(flatness, fr.TOLERANCE['flatness'][noise]):
        assert got <= bound, (flatness, fr.TOLERANCE['flatness'][noise])
    # the spot is still there: the median ignores it, the flat image keeps it
    on, k, _ = fr.rings(*img.shape, circle)
    cx, cy, rad = circle
    assert flat[int(round(cy - rad / 5.0)), int(round(cx + rad / 3.0))] < 0.7 * np.median(flat[on & (k < 100)])


def test_smoothing_smears_the_limb():
    """Why smooth = 1 is the default: a running mean over five rings is four times less flat."""
    img, circle = fr.synthetic_disk(0.0)
    flat5 = fr.flatten_disk(img, circle, smooth=5)[0]
    core5 = fr.flatness(fr.profile_of(*fr.ring_medians(flat5, circle)))[0]
    print('smooth 5: flatness core %.6f' % core5)
    assert 0.012 < core5 < 0.021 and core5 > 4 * fr.TOLERANCE['flatness'][0.0][0]


# ---- gain_from_profile against its restatement ----
def _profile(count, lo, hi):
    return fr.profile_of(np.array(count), np.array(lo), np.array(hi))


@pytest.mark.parametrize('smooth', [1, 3, 5, 11])
@pytest.mark.parametrize('level', [None, 1234.5])
def test_gain_from_profile_matches_the_restatement_bit_for_bit(smooth, level):
    from solex_ser_recon_en_amd import flatten
    rng = np.random.default_rng(smooth)
    kk = 57
    lo = np.sort(rng.integers(100, 60000, kk))[::-1].astype(np.uint16)
    hi = (lo + rng.integers(0, 3, kk)).astype(np.uint16)
    count = rng.integers(1, 500, kk)
    count[[0, 5, 6, 7, 30, 56]] = 0                         # ring 6 is as far from 4 as from 8 (5 .. 7 are empty): the lower index wins
    lo[40], hi[40] = 0, 0                                   # a ring whose median is 0: gain 0
    lo[41], hi[41] = 1, 1                                   # and one that the gain would blow up: max_gain
    profile = _profile(count, lo, hi)
    got = flatten.gain_from_profile(profile, smooth, level, 8.0)
    want = fr.gain_from_profile(profile, smooth, level, 8.0)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if smooth == 1:
        assert got[40] == 0.0 and got[41] == 8.0 and got[5] == got[4] and got[6] == got[4] and got[7] == got[8] and got[0] == got[1]
        assert got[56] == got[55] and (got <= 8.0).all() and (got >= 0.0).all()


def test_gain_from_profile_refusals():
    from solex_ser_recon_en_amd import flatten
    empty = _profile([0, 0, 0], [0, 0, 0], [0, 0, 0])
    with pytest.raises(ValueError, match='no ring'):
        flatten.gain_from_profile(empty)
    with pytest.raises(ValueError, match='no ring'):
        fr.gain_from_profile(empty)
    some = _profile([1, 2, 3], [5, 5, 5], [5, 5, 5])
    for smooth in (0, 2, -1, 1.5):
        with pytest.raises(ValueError, match='smooth'):
            flatten.gain_from_profile(some, smooth)
    for max_gain in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='max_gain'):
            flatten.gain_from_profile(some, 1, None, max_gain)
    with pytest.raises(ValueError, match='level'):
        flatten.gain_from_profile(some, 1, -3.0)
    assert np.array_equal(flatten.gain_from_profile(some), [1.0, 1.0, 1.0])


# ---- the C ABI without a device ----
def test_ring_workspace_query_needs_no_gpu():
    from solex_ser_recon_en_amd._lib import lib
    for k in (1, 2, 121, 1000, 16384):
        # three [K][256] tables of 32-bit counts, 16 bytes of select state a ring, room to align the tables to 256 bytes
        assert lib.shg_ring_medians_u16_workspace_bytes(k) == k * (3 * 1024 + 16) + 256
    for k in (0, -1, 16385, 1 << 40):
        assert lib.shg_ring_medians_u16_workspace_bytes(k) == 0


def _c3(*v):
    return (ctypes.c_double * 3)(*v)


def test_ring_calls_refuse_bad_arguments_before_any_device_work():
    """Every refusal comes before the first HIP call: made-up addresses are never touched."""
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(4096)
    big = 1 << 30
    ok = _c3(10.0, 10.0, 4.5)

    def medians(img=p, h=20, w=20, pitch=20, c3=ok, k=5, count=p, lo=p, hi=p, ws=p, ws_bytes=big):
        return lib.shg_ring_medians_u16(img, h, w, pitch, c3, k, count, lo, hi, ws, ws_bytes, None)

    gains = (ctypes.c_double * 5)(1.0, 1.0, 1.0, 1.0, 1.0)

    def flatten(img=p, h=20, w=20, pitch=20, c3=ok, gain=gains, k=5, out=ctypes.c_void_p(8192), out_pitch=20):
        return lib.shg_ring_flatten_u16(img, h, w, pitch, c3, gain, k, out, out_pitch, None)

    for call in (medians, flatten):
        for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385, pitch=16385)):
            assert call(**over) == E_UNSUPPORTED, over
        assert 'image of' in _lib.last_error()
        for over in (dict(img=None), dict(pitch=19), dict(c3=None), dict(c3=_c3(float('nan'), 10.0, 4.5)), dict(c3=_c3(10.0, float('inf'), 4.5)),
                     dict(c3=_c3(10.0, 10.0, float('nan'))), dict(c3=_c3(10.0, 10.0, -0.5), k=0), dict(c3=_c3(10.0, 10.0, 16384.0), k=16385),
                     dict(c3=_c3(65536.0, 10.0, 4.5)), dict(c3=_c3(10.0, -65536.0, 4.5)), dict(k=4), dict(k=6),
                     dict(c3=_c3(10.0, 10.0, 5.0), k=5)):
            assert call(**over) == E_ARG, over
    for over in (dict(count=None), dict(lo=None), dict(hi=None), dict(ws=None), dict(ws_bytes=lib.shg_ring_medians_u16_workspace_bytes(5) - 1),
                 dict(ws_bytes=0)):
        assert medians(**over) == E_ARG, over
    assert 'workspace' in _lib.last_error()
    for bad in (-1.0, -1e-300, float('nan'), float('inf')):
        g = (ctypes.c_double * 5)(1.0, 1.0, 1.0, bad, 1.0)
        assert flatten(gain=g) == E_ARG, bad
    assert 'gain[3]' in _lib.last_error()
    for over in (dict(gain=None), dict(out=None), dict(out_pitch=19), dict(out=p, pitch=24, out_pitch=20), dict(out=p, pitch=20, out_pitch=24)):
        assert flatten(**over) == E_ARG, over
    assert 'in place' in _lib.last_error()


def test_ops_refuse_cpu_tensors_and_bad_circles():
    import torch
    from solex_ser_recon_en_amd import ops
    img = torch.zeros((8, 8), dtype=torch.uint16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ring_medians_u16(img, (4.0, 4.0, 3.0))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ring_flatten_u16(img, (4.0, 4.0, 3.0), np.ones(4))


# ---- flatten_scan's refusals ----
def test_flatten_scan_needs_the_limb_fits_circle():
    from solex_ser_recon_en_amd import SHG_MAIN, flatten
    for over in (dict(ratio_fixe=1.1), dict(slant_fix=0.5), dict(ratio_fixe=1.0, slant_fix=0.0)):
        with pytest.raises(ValueError, match='circle'):
            flatten.flatten_scan('no-such-file.ser', dict(SHG_MAIN.default_options(), **over))
    with pytest.raises(ValueError, match='de-vignette'):
        flatten.flatten_scan('no-such-file.ser', dict(SHG_MAIN.default_options(), **{'de-vignette': True}))


def test_flatten_scan_refuses_a_frame_shard(monkeypatch):
    from solex_ser_recon_en_amd import dist, flatten

    class Shard:
        FrameCount, frame_range, ih, iw = 300, (0, 150), 400, 48

        def device_stack(self):
            raise AssertionError('the shard must be refused before its frames are asked for')

    monkeypatch.setattr(dist, 'active', lambda: True)
    with pytest.raises(ValueError, match='shard'):
        flatten.flatten_scan(Shard())
