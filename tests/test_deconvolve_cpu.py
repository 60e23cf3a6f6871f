"""The deconvolution stage without a GPU: the restatement of its arithmetic (tests/deconvolve_ref.py) held to what the header
states of it -- a constant image and R = 0 are fixed points, zero-padded taps change no bit, the adjoint reverses the taps, the flush
leaves no value in (0, 2^-20) --, its accuracy against planted truth (re-measured against TOLERANCE), the Gaussian taps, and the
argument checks of the command line and of the C entry points."""
import ctypes

import numpy as np
import pytest

from solex_ser_recon_en_amd import deconvolve
from tests import deconvolve_ref as dr


def random_image(h, w, seed=0):
    return np.random.default_rng([h, w, seed]).integers(0, 65536, (h, w)).astype(np.uint16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_a_constant_image_is_a_fixed_point_when_the_taps_sum_to_one():
    # taps that are multiples of 2^-4 and sum to exactly 1: every partial sum of k v is exact for a 16-bit v
    taps = np.array([1, 2, 3, 4, 3, 2, 1], np.float32) / 16
    assert float(taps.astype(np.float64).sum()) == 1.0
    for value in (1, 777, 65535):
        for shape in ((1, 1), (3, 40), (17, 5), (40, 33)):
            img = np.full(shape, value, np.uint16)
            out, e = dr.deconvolve(img, taps, 6)
            assert np.array_equal(out, img) and (e == np.float32(value)).all()
    out, e = dr.deconvolve(np.zeros((9, 7), np.uint16), taps, 3)
    assert (out == 0).all() and (bits(e) == 0).all()


def test_radius_zero_with_tap_one_is_the_identity():
    img = random_image(33, 57)
    for n in (1, 2, 9):
        out, e = dr.deconvolve(img, [1.0], n)
        assert np.array_equal(out, img) and np.array_equal(e, img.astype(np.float32))


def test_zero_padded_taps_give_identical_bits():
    img = random_image(33, 57, 1)
    for taps in (dr.gaussian(1.2, 3), np.array([0.5, 0.3, 0.2], np.float32), np.array([1.0], np.float32)):
        want = dr.iterate(img, taps, 4)
        for radius in (taps.size // 2 + 1, 6, 16):
            padded = dr.pad_taps(taps, radius)
            assert padded.size == 2 * radius + 1 and np.array_equal(bits(dr.iterate(img, padded, 4)), bits(want))


def test_the_adjoint_reverses_the_taps():
    img = random_image(33, 57, 2)
    taps = np.array([0.5, 0.3, 0.2], np.float32)
    right, wrong = dr.iterate(img, taps, 3), dr.iterate(img, taps, 3, reverse=False)
    assert not np.array_equal(bits(right), bits(wrong))
    assert np.abs(right.astype(np.float64) - wrong.astype(np.float64)).max() > 1.0
    # the adjoint keeps the flux (sum e c = sum q B(e) = sum d up to the borders and rounding); the taps unreversed do not
    smooth = np.rint(dr.blur64(random_image(40, 41, 4).astype(np.float64), np.full(5, 0.2))).astype(np.uint16)
    flux = [abs(float(dr.iterate(smooth, taps, 3, reverse=rev).astype(np.float64).sum() / smooth.astype(np.float64).sum()) - 1.0) for rev in (True, False)]
    print('flux off by %.3e with the adjoint, %.3e without' % tuple(flux))
    assert flux[0] < flux[1]
    # symmetric taps are their own reverse
    sym = dr.gaussian(1.5, 6)
    assert np.array_equal(bits(dr.iterate(random_image(20, 21), sym, 2)), bits(dr.iterate(random_image(20, 21), sym, 2, reverse=False)))


def test_a_zero_sky_triggers_the_flush_and_zeros_stay_zero():
    img = dr.zero_sky_disk(90, 100)
    assert (img == 0).sum() > 2000
    taps = dr.gaussian(1.5, 6)
    d = img.astype(np.float32)
    e, fired = d, 0
    for _ in range(60):
        p = e * dr.blur(d / np.maximum(dr.blur(e, taps), dr.MIN_BLUR), np.ascontiguousarray(taps[::-1]))
        fired += int(((p > 0) & (p < dr.FLUSH)).sum())
        e = np.where(p < dr.FLUSH, np.float32(0), np.minimum(p, dr.CLAMP))
        assert not ((e > 0) & (e < dr.FLUSH)).any() and (e[img == 0] == 0).all() and np.isfinite(e).all()
    print('the flush fired %d times in 60 iterations' % fired)
    assert fired > 0
    assert np.array_equal(bits(e), bits(dr.iterate(img, taps, 60)))
    # a random image stays below the clamp for many iterations, and the clamp holds when it is reached
    e = dr.iterate(random_image(33, 57, 3), taps, 50)
    assert e.max() <= dr.CLAMP and np.isfinite(e).all()


def test_accuracy_against_planted_truth():
    got = dr.scene_measures(lambda img, taps, n: dr.deconvolve(img, taps, n)[0])
    print('noise-free: %.3f counts rms within 12 px of the spot blurred, %.3f after 10 iterations: %.6f of it; flux off by %.3e; '
          'with noise of %.2f counts: %.2f blurred, %.2f after 5 iterations: %.6f of it'
          % (got['blurred_rms'], got['clean_rms'], got['clean'], got['flux'], dr.NOISE * 65535.0, got['noisy_blurred_rms'], got['noisy_rms'],
             got['noisy']))
    for key in ('clean', 'flux', 'noisy'):
        assert got[key] <= dr.TOLERANCE[key], key
        assert dr.TOLERANCE[key] <= 1.3 * got[key], 'the bound on %s is no longer the measured value plus a quarter' % key
    assert got['blurred_rms'] > 300.0                       # the blur is worth deconvolving


def test_gaussian_taps_ranges_sums_and_symmetry():
    for sigma, radius in ((0.3, None), (1.2, None), (1.5, 6), (2.5, None), (4.0, None), (1.2, 16), (0.3, 16), (4.0, 0), (1.0, 1)):
        k = deconvolve.gaussian_taps(sigma, radius)
        r = int(np.ceil(4.0 * sigma)) if radius is None else radius
        assert k.dtype == np.float32 and k.size == 2 * r + 1 and np.array_equal(k, k[::-1])
        assert abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6
        assert ((k == 0) | ((k >= np.float32(2.0 ** -30)) & (k <= 1))).all() and k[r] == k.max() > 0
        dr.check_taps(k)                                   # what the C entry point accepts
        assert (np.diff(k[:r + 1]) >= 0).all()
    assert np.array_equal(deconvolve.gaussian_taps(1.5, 6), dr.gaussian(1.5, 6))
    assert deconvolve.gaussian_taps(4.0, 0).tolist() == [1.0]
    assert (deconvolve.gaussian_taps(0.3, 16)[:12] == 0).all()                 # flushed below 2^-30
    for sigma, radius in ((0.29, None), (4.01, None), (float('nan'), None), (float('inf'), 3), (-1.0, None), ('1', None), (1.2, -1), (1.2, 17),
                          (1.2, 2.0)):
        with pytest.raises(ValueError):
            deconvolve.gaussian_taps(sigma, radius)


def test_command_line_refusals_need_no_gpu(monkeypatch, capsys):
    for argv, message in ((['x.ser', '--psf-sigma', '0.1'], 'sigma lies in'), (['x.ser', '--psf-sigma', '5'], 'sigma lies in'),
                          (['x.ser', '--psf-sigma', 'nan'], 'sigma lies in'), (['x.ser', '--iterations', '0'], 'iterations is an integer'),
                          (['x.ser', '--iterations', '201'], 'iterations is an integer'), (['x.ser', '--radius', '17'], 'radius is an integer'),
                          (['x.ser', '-w', '1'], '-w is not a deconvolve flag'), (['no_such_file.ser'], 'no such file'),
                          (['no_such_file.png'], 'no such file'), ([], 'exactly one SER, AVI or PNG file')):
        with pytest.raises(SystemExit):
            deconvolve.main(argv)
        assert message in capsys.readouterr().err, argv
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit):
        deconvolve.main(['x.ser'])
    assert 'deconvolution is single-process: run it without torchrun' in capsys.readouterr().err
    for n in (0, 201, 2.0, None):
        with pytest.raises(ValueError):
            deconvolve._check_iterations(n)


def test_c_entry_points_without_a_gpu():
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    assert lib.shg_rl_workspace_bytes(2000, 2000) == 256 + 2000 * 2000 * 8
    assert lib.shg_rl_workspace_bytes(1, 1) == 256 + 8 and lib.shg_rl_workspace_bytes(16384, 16384) == 256 + 16384 * 16384 * 8
    assert lib.shg_rl_workspace_bytes(2000, 2000) <= 12 * 2000 * 2000 + 256
    for h, w in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, 5), (5, -3)):
        assert lib.shg_rl_workspace_bytes(h, w) == 0
    one = ctypes.c_void_p(4096)
    taps = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
    big = 1 << 20

    def call(img=one, h=8, w=8, pitch=8, k=taps, radius=1, iterations=3, out=ctypes.c_void_p(8192), out_pitch=8, estimate=None,
             ws=ctypes.c_void_p(1 << 16), ws_bytes=big):
        return lib.shg_rl_deconvolve_u16(img, h, w, pitch, k, radius, iterations, out, out_pitch, estimate, ws, ws_bytes, None)

    assert lib.shg_rl_deconvolve_u16(None, 8, 8, 8, None, 1, 3, None, 8, None, None, 0, None) == -1
    assert 'null pointer' in _lib.last_error()
    need = lib.shg_rl_workspace_bytes(8, 8)
    for over in (dict(img=None), dict(k=None), dict(out=None), dict(ws=None), dict(pitch=7), dict(out_pitch=7), dict(radius=-1), dict(radius=17),
                 dict(iterations=0), dict(iterations=201), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                 dict(out=one), dict(out=ctypes.c_void_p(4096 + 126)), dict(out=ctypes.c_void_p(4096 - 126)),             # on the image
                 dict(estimate=ctypes.c_void_p(4096 + 124)), dict(estimate=ctypes.c_void_p(8192 - 252)), dict(estimate=ctypes.c_void_p(8192 + 124)),
                 dict(ws=ctypes.c_void_p(4096 - need + 1)), dict(ws=ctypes.c_void_p(8192 + 126)),
                 dict(estimate=ctypes.c_void_p((1 << 16) + need - 4)), dict(estimate=ctypes.c_void_p((1 << 16) - 252))):
        assert call(**over) == -1, over
        assert 'shg_rl_deconvolve_u16' in _lib.last_error()
    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        assert call(**over) == -3, over
    for bad in ((0.25, float('nan'), 0.75), (float('inf'), 0.0, 0.0), (-0.25, 1.0, 0.25), (0.5, 0.5 - 2.0 ** -31, 2.0 ** -31), (0.0, 1.0625, 0.0),
                (0.25, 0.5, 0.2), (0.25, 0.5, 0.252), (0.0, 0.0, 0.0)):
        assert call(k=(ctypes.c_float * 3)(*bad)) == -1, bad
    assert 'tap' in _lib.last_error()
