"""Limb protection without a GPU: the restatement of its arithmetic (tests/limbguard_ref.py) held to what the header states of it --
the band of the limb is the image bit for bit, where the weight is 1 the output is the processed plane bit for bit, a circle that
contains the image leaves the inner plane the image, a plane is continuous in value and slope across its edge (a ramp continues as
the same ramp), margin 0 --, its gain against planted truth (re-measured against TOLERANCE), the settings of the Python layer, and
the argument checks of the two command lines and of the C entry points."""
import ctypes

import numpy as np
import pytest

from solex_ser_recon_en_amd import deconvolve, limbguard, sharpen
from tests import limbguard_ref as lr

CIRCLES = {'inside': (31.3, 27.6, 17.4), 'on a pixel': (30.0, 26.0, 15.5), 'off the image': (-20.5, 70.25, 60.3),
           'small': (12.25, 9.75, 2.5)}


def random_image(h, w, seed=0):
    return np.random.default_rng([h, w, seed]).integers(0, 65536, (h, w)).astype(np.uint16)


def scramble(plane):
    """A stand-in for a filter: every value changed, deterministically."""
    return (plane.astype(np.uint32) * 40503 + 12345 & 0xFFFF).astype(np.uint16)


def test_the_band_is_the_image_and_full_weight_is_the_processed_plane():
    img = random_image(57, 63)
    for name, circle in CIRCLES.items():
        for margin, blend in ((1.0, 2.0 ** -10), (0.0, 3.0), (1.5, 100.0)):
            reach = min(5.0, circle[2] - margin)
            inner, outer = lr.split(img, circle, margin, reach)
            disk, sky = scramble(inner), scramble(outer)
            band, disk_full, sky_full = lr.regions(img.shape, circle, margin, blend)
            for with_sky in (True, False):
                out = lr.merge(img, disk, sky if with_sky else None, circle, margin, blend)
                assert np.array_equal(out[band], img[band]), (name, margin, blend)
                assert np.array_equal(out[disk_full], disk[disk_full]), (name, margin, blend)
                if with_sky:
                    assert np.array_equal(out[sky_full], sky[sky_full]), (name, margin, blend)
                else:
                    rho = lr.rays(img.shape[0], img.shape[1], circle)[0]
                    assert np.array_equal(out[rho >= circle[2] - margin], img[rho >= circle[2] - margin])
            if blend == 2.0 ** -10 and name != 'small':
                assert disk_full.any() and sky_full.any() and (band.any() or margin == 0.0)
            # the planes are the image where they keep it
            rho = lr.rays(img.shape[0], img.shape[1], circle)[0]
            assert np.array_equal(inner[rho <= circle[2] - margin], img[rho <= circle[2] - margin])
            assert np.array_equal(outer[rho >= circle[2] + margin], img[rho >= circle[2] + margin])
            assert (inner != img)[rho > circle[2] - margin].any() and (outer != img)[rho < circle[2] + margin].any()
    # a process that returns its input gives the image back
    for name, circle in CIRCLES.items():
        assert np.array_equal(lr.protect(img, circle, lambda p: p, 1.0, 2.5, 4.0), img)
        assert np.array_equal(lr.protect(img, circle, lambda p: p, 0.0, 2.5, 4.0, sky=False), img)


def test_a_circle_that_contains_the_image_leaves_the_inner_plane_the_image():
    img = random_image(33, 41, 1)
    inner, outer = lr.split(img, (20.0, 16.0, 80.5), 6.0, 24.0)
    assert np.array_equal(inner, img) and (outer != img).any()
    assert np.array_equal(lr.merge(img, scramble(inner), scramble(outer), (20.0, 16.0, 80.5), 6.0, 2.0 ** -10), scramble(inner))
    # and one the image lies outside of leaves the outer plane the image
    inner, outer = lr.split(img, (-50.0, -50.0, 20.0), 3.0, 8.0)
    assert np.array_equal(outer, img) and (inner != img).any()


def test_the_continuation_is_a_point_reflection_continuous_in_value_and_slope():
    """The point reflection of a linear function about a point of its graph is the same function: a ramp continues as itself within
    `reach`, to the rounding of the two samples and of the result, and holds a plateau along the ray beyond it.  Plain mirroring
    would fold the ramp back at the edge."""
    h, w = 90, 100
    r, c = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[None, :]
    ramp = np.rint(20000.0 + 150.0 * c + 90.0 * r).astype(np.uint16)
    circle, margin, reach = (48.3, 44.6, 25.4), 3.0, 12.0
    inner, outer = lr.split(ramp, circle, margin, reach)
    rho = lr.rays(h, w, circle)[0]
    e, f = circle[2] - margin, circle[2] + margin
    near = (rho > e) & (rho <= e + reach)
    off = np.abs(inner.astype(np.int64) - ramp.astype(np.int64))[near]
    print('a ramp continued outwards over %d pixels: off by up to %d counts' % (near.sum(), off.max()))
    assert near.sum() > 1000 and off.max() <= 2                   # (three values rounded to a count, one of them doubled)
    near = (rho < f) & (rho >= f - reach)
    assert np.abs(outer.astype(np.int64) - ramp.astype(np.int64))[near].max() <= 2
    # the plateau: two pixels on one ray beyond the reach hold the same value
    circle = (50.0, 40.0, 20.0)
    inner, _ = lr.split(ramp, circle, 2.0, 5.0)
    assert inner[40, 50 + 30] == inner[40, 50 + 40] == inner[40, 50 + 24] and inner[40 + 25, 50] == inner[40 + 45, 50]
    assert inner[40, 50 + 19] != inner[40, 50 + 23]
    # full scale and zero: the 2 s - m clamp at both ends
    step = np.where(c < 50.0, 65535, 0).astype(np.uint16) + 0 * ramp
    inner, outer = lr.split(step, (49.5, 40.0, 20.0), 0.0, 10.0)
    assert inner.max() == 65535 and inner.min() == 0 and outer.max() == 65535 and outer.min() == 0


def test_gain_against_planted_truth():
    got = lr.restated_measures()
    print('noise-free, 30 iterations, margin 6, blend 4, reach 24: inner annulus %.3f counts rms blurred, %.3f plain, %.3f protected: %.6f '
          'of plain; sky annulus %.3f blurred, %.3f plain, %.3f protected: %.6f of plain'
          % (got['inner_blurred_rms'], got['inner_plain_rms'], got['inner_rms'], got['inner'], got['sky_blurred_rms'], got['sky_plain_rms'],
             got['sky_rms'], got['sky']))
    print('with noise of %.2f counts: inner %.2f plain, %.2f protected: %.6f of plain; sky %.2f plain, %.2f protected: %.6f of plain'
          % (lr.dr.NOISE * 65535.0, got['noisy_inner_plain_rms'], got['noisy_inner_rms'], got['noisy_inner'], got['noisy_sky_plain_rms'],
             got['noisy_sky_rms'], got['noisy_sky']))
    print('default sharpen, noise-free: a sky-annulus pixel moves by up to %d counts plain, %d protected: %.6f of plain'
          % (got['sharpen_plain_max'], got['sharpen_max'], got['sharpen']))
    for key in ('inner', 'sky', 'sharpen'):
        assert got[key] <= lr.TOLERANCE[key], key
        assert lr.TOLERANCE[key] <= 1.3 * got[key], 'the bound on %s is no longer the measured value plus a quarter' % key
        assert got[key] < lr.HARD[key] and lr.TOLERANCE[key] < lr.HARD[key], key
    for key in ('noisy_inner', 'noisy_sky'):
        assert got[key] <= lr.TOLERANCE[key], key
        assert lr.TOLERANCE[key] <= got[key] + 0.0101, 'the bound on %s is no longer the measured value plus 0.01' % key
    # the defect is there to cure: plain Richardson-Lucy leaves the annulus inside the limb worse than the blurred image
    assert got['inner_plain_rms'] > got['inner_blurred_rms'] and got['sky_plain_rms'] > 10.0 * got['sky_blurred_rms']
    assert got['sharpen_plain_max'] > 100


def test_settings_defaults_and_refusals():
    circle = (100.0, 90.0, 50.0)
    assert limbguard.settings({'circle': circle}, 5.0) == (circle, 5.0, 4.0, 32.0, True)
    assert limbguard.settings({}, 6.0, circle) == (circle, 6.0, 4.0, 32.0, True)
    assert limbguard.settings({'margin': 30, 'blend': 2, 'reach': 64, 'sky': False, 'circle': circle}, 6.0) == (circle, 30.0, 2.0, 20.0, False)
    assert limbguard.settings({'margin': 0, 'reach': 1}, 6.0, circle) == (circle, 0.0, 4.0, 1.0, True)
    for limb in ({'circle': None}, {'circle': (-1, -1, -1)}, {'circle': (1.0, 2.0)}, {'circle': (1.0, float('nan'), 30.0)}, {'circle': (1.0, 2.0, 0.0)},
                 {'circle': (1.0, 2.0, 16384.0)}, {'circle': circle, 'margin': -1.0}, {'circle': circle, 'margin': 49.5},
                 {'circle': circle, 'margin': float('inf')}, {'circle': circle, 'blend': 0.0}, {'circle': circle, 'blend': float('nan')},
                 {'circle': circle, 'reach': 0.5}, {'circle': circle, 'reach': float('inf')}, {'circle': circle, 'edge': 3.0},
                 {'circle': circle, 'margin': 'wide'}, 6.0, circle):
        with pytest.raises(ValueError):
            limbguard.settings(limb, 6.0)
    for bad in (dict(margin=-1.0), dict(margin=50.0), dict(blend=0.0), dict(reach=0.0), dict(circle=(1.0, 2.0, -3.0))):
        with pytest.raises(ValueError):                                  # before anything touches a device
            limbguard.protect(None, bad.get('circle', circle), lambda p: p, bad.get('margin', 6.0), bad.get('blend', 4.0), bad.get('reach', 32.0))


@pytest.mark.parametrize('module', [deconvolve, sharpen], ids=['deconvolve', 'sharpen'])
def test_command_line_refusals_need_no_gpu(module, capsys):
    for argv, message in ((['x.png', '--limb-protect'], '--limb-protect on a PNG needs --circle'),
                          (['x.png', '--limb-protect', '4'], '--limb-protect on a PNG needs --circle'),
                          (['x.ser', '--limb-blend', '3'], 'go with --limb-protect'), (['x.ser', '--limb-reach', '20'], 'go with --limb-protect'),
                          (['x.ser', '--limb-disk-only'], 'go with --limb-protect'),
                          (['x.png', '--circle', '50,50,40', '--limb-blend', '3'], 'go with --limb-protect'),
                          (['x.ser', '--limb-protect', '-2'], 'margin is finite and >= 0'), (['x.ser', '--limb-protect', 'nan'], 'margin is finite'),
                          (['x.ser', '--limb-protect', '--limb-blend', '0'], 'blend is finite and > 0'),
                          (['x.ser', '--limb-protect', '--limb-reach', '0.5'], 'reach is finite and >= 1'),
                          (['x.png', '--circle', '50,50,40', '--limb-protect', '39.5'], 'rad - margin is at least 1'),
                          (['x.png', '--circle', '50,50', '--limb-protect'], '--circle is cx,cy,rad'),
                          (['x.ser', '--limb-protect', 'wide'], 'invalid float value'),
                          (['no_such_file.ser', '--limb-protect', '6', '--limb-blend', '2', '--limb-reach', '12', '--limb-disk-only'], 'no such file'),
                          (['no_such_file.png', '--circle', '50,50,40', '--limb-protect=6'], 'no such file')):
        with pytest.raises(SystemExit) as exit_:
            module.main(argv)
        said = capsys.readouterr()
        assert exit_.value.code == 2 and said.out == '' and message in said.err, (argv, said.err)


def test_c_entry_points_refuse_without_a_gpu():
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    img, inner, outer, out = (ctypes.c_void_p(a) for a in (4096, 8192, 12288, 16384))
    circle = (ctypes.c_double * 3)(4.0, 3.5, 3.0)

    def split(img=img, h=8, w=8, pitch=8, circle=circle, margin=1.0, reach=1.5, inner=inner, inner_pitch=8, outer=outer, outer_pitch=8):
        return lib.shg_limb_split_u16(img, h, w, pitch, circle, margin, reach, inner, inner_pitch, outer, outer_pitch, None)

    def merge(img=img, pitch=8, disk=inner, disk_pitch=8, sky=outer, sky_pitch=8, h=8, w=8, circle=circle, margin=1.0, blend=2.0, out=out,
              out_pitch=8):
        return lib.shg_limb_merge_u16(img, pitch, disk, disk_pitch, sky, sky_pitch, h, w, circle, margin, blend, out, out_pitch, None)

    def ring(*values):
        return (ctypes.c_double * 3)(*values)

    nan, inf = float('nan'), float('inf')
    circles = [ring(nan, 3.5, 3.0), ring(4.0, inf, 3.0), ring(4.0, 3.5, nan), ring(4.0, 3.5, 0.0), ring(4.0, 3.5, -3.0), ring(4.0, 3.5, 16384.0),
               ring(65536.0, 3.5, 3.0), ring(4.0, -65536.0, 3.0), ring(4.0, 3.5, 1.9)]
    for call, name in ((split, 'shg_limb_split_u16'), (merge, 'shg_limb_merge_u16')):
        for over in [dict(img=None), dict(circle=None), dict(pitch=7), dict(margin=-0.5), dict(margin=nan), dict(margin=inf), dict(margin=2.5)] + \
                [dict(circle=c) for c in circles]:
            assert call(**over) == -1, (name, over)
            assert name in _lib.last_error()
        for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
            assert call(**over) == -3, (name, over)
    last = 2 * (7 * 8 + 7)                                        # the byte offset of an 8 x 8 plane's last element
    for over in (dict(inner=None, outer=None), dict(inner_pitch=7), dict(outer_pitch=7), dict(reach=0.5), dict(reach=2.5), dict(reach=nan),
                 dict(reach=inf), dict(inner=img), dict(outer=img), dict(inner=ctypes.c_void_p(4096 + last)), dict(outer=ctypes.c_void_p(4096 - last)),
                 dict(outer=inner), dict(outer=ctypes.c_void_p(8192 + last)), dict(inner=ctypes.c_void_p(12288 + last))):
        assert split(**over) == -1, over
        assert 'shg_limb_split_u16' in _lib.last_error()
    assert 'overlaps' in _lib.last_error()
    for over in (dict(disk=None), dict(out=None), dict(disk_pitch=7), dict(sky_pitch=7), dict(out_pitch=7), dict(blend=0.0), dict(blend=-1.0),
                 dict(blend=nan), dict(blend=inf), dict(out=img), dict(out=inner), dict(out=outer), dict(out=ctypes.c_void_p(4096 + last)),
                 dict(out=ctypes.c_void_p(8192 - last)), dict(out=ctypes.c_void_p(12288 + last))):
        assert merge(**over) == -1, over
        assert 'shg_limb_merge_u16' in _lib.last_error()
    assert 'overlaps' in _lib.last_error()
