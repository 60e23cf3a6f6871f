"""The sharpening stage without a GPU: the restatement of its arithmetic (tests/sharpen_ref.py) held to what can be derived -- the
identity at unity gains, an independently written dense form, planes that sum to the image, the layers' noise factors, the transfer
function within the bound DESIGN.md section 18 derives --, its accuracy against planted truth (re-measured against TOLERANCE), and
the argument checks of the Python layer and of the C entry points."""
import ctypes

import numpy as np
import pytest

from tests import sharpen_ref as sr

SHAPES = [(1, 1, 6), (1, 9, 6), (9, 1, 6), (7, 5, 6), (33, 257, 4), (70, 130, 6), (300, 520, 3)]      # (h, w, levels)
IDS = ['%dx%d_L%d' % s for s in SHAPES]


def random_image(h, w, seed=0):
    return np.random.default_rng([h, w, seed]).integers(0, 65536, (h, w)).astype(np.uint16)


@pytest.fixture(scope='module')
def decomposed():
    out = {}
    for h, w, levels in SHAPES:
        img = random_image(h, w)
        planes = sr.wavelet_planes(img, levels)
        img.setflags(write=False), planes.setflags(write=False)
        out[(h, w, levels)] = (img, planes)
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_unity_is_the_identity_and_planes_sum_to_the_image(decomposed, shape):
    img, planes = decomposed[shape]
    levels = shape[2]
    assert np.array_equal(planes.astype(np.int64).sum(axis=0), img.astype(np.int64) * 64)
    assert np.array_equal(sr.recombine(planes, [256] * levels, [0] * levels), img)
    for value in (0, 65535):
        const = np.full(shape[:2], value, np.uint16)
        out, p = sr.sharpen(const, [256] * levels)
        assert np.array_equal(out, const) and (p[:levels] == 0).all() and (p[levels] == 64 * value).all()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_the_dense_form_agrees_bit_for_bit(decomposed, shape):
    img, planes = decomposed[shape]
    dense = sr.dense_planes(img, shape[2])
    assert np.array_equal(dense, planes.astype(np.float64))


def test_reflection_repeats():
    assert sr.reflect_index(np.arange(-9, 14), 5).tolist() == [1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3]
    assert sr.reflect_index(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert sr.reflect_index(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    line = np.arange(5)
    assert np.array_equal(line[sr.reflect_index(np.arange(-64, 69), 5)], np.pad(line, 64, mode='reflect'))


def test_gates_gains_and_clipping():
    img = random_image(40, 37, 5)
    planes = sr.wavelet_planes(img, 3)
    # every layer gated: c_L rounded
    gated = sr.recombine(planes, [4096, 256, 7], [sr.MAX_THRESHOLD_Q6] * 3)
    assert np.array_equal(gated, ((planes[3].astype(np.int64) + 32) >> 6).astype(np.uint16))
    assert np.array_equal(sr.recombine(planes, [0, 0, 0], [0, 0, 0]), gated)
    # the largest gain clips both ways on a chequerboard
    board = ((np.add.outer(np.arange(12), np.arange(14)) % 2) * 65535).astype(np.uint16)
    out, p = sr.sharpen(board, [4096])
    assert set(np.unique(out).tolist()) == {0, 65535} and (np.abs(p[0]) == 32 * 65535).all()      # (the board smooths to its mean)
    # the soft threshold shrinks towards zero and is odd
    assert sr.soft(np.array([-10, -3, 0, 3, 10]), 3).tolist() == [-7, 0, 0, 0, 7]
    assert sr.soft(np.array([-10, 10]), 0).tolist() == [-10, 10]


def test_noise_is_the_lower_median():
    img = random_image(30, 41, 2)
    mag = np.abs(sr.wavelet_planes(img, 1)[0].astype(np.int64))
    med, n = sr.noise(img)
    assert n == 30 * 41 and med == np.sort(mag.ravel())[(n - 1) // 2]
    assert sr.noise(img, (-1, -1, -1)) == (med, n)
    med, n = sr.noise(img, (20.0, 15.0, 1.0))                        # five pixels
    assert n == 5 and med == sorted(mag[r, c] for r, c in ((15, 20), (14, 20), (16, 20), (15, 19), (15, 21)))[2]
    med, n = sr.noise(img, (20.0, 15.0, 0.0))
    assert n == 1 and med == mag[15, 20]
    assert sr.noise(img, (200.0, 15.0, 3.0)) == (0, 0)
    assert sr.noise(np.full((9, 9), 777, np.uint16)) == (0, 81)


def test_noise_factors_match_the_impulse_response_summed_independently():
    from solex_ser_recon_en_amd import sharpen
    got, want = sharpen.noise_factors(6), sr.layer_noise_factors(6)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert [round(f, 4) for f in got] == [0.8908, 0.2007, 0.0855, 0.0412, 0.0204, 0.0102]
    assert sharpen.noise_factors(2) == got[:2]
    # and against the restatement itself: the response of the integer transform to one impulse, up to its rounding
    img = np.zeros((129, 129), np.uint16)
    img[64, 64] = 64000
    planes = sr.wavelet_planes(img, 4).astype(np.float64) / (64.0 * 64000.0)
    for j in range(4):
        assert abs(np.sqrt((planes[j] ** 2).sum()) - got[j]) < 1e-3


@pytest.mark.parametrize('period', [4, 8, 16])
@pytest.mark.parametrize('gains', [(1.0, 1.8, 1.4, 1.0), (0.0, 2.5, 1.0), (1.0, 1.0, 1.0, 1.0, 1.0, 3.0), (4.0,)], ids=['default', 'three', 'six', 'one'])
def test_transfer_function_within_the_derived_bound(period, gains):
    """A horizontal sinusoid of amplitude 4000 on 30000 comes out with amplitude T(omega) A, A being the fundamental of the image as
    rounded to integers (an image of whole periods: its harmonics pass through the linear transform one by one); the bound is
    transfer_bound's, derived from the <= 1/128-count rounding a level, not fitted."""
    from solex_ser_recon_en_amd import sharpen
    gain_q8 = sharpen.quantise_gains(gains)
    levels = len(gains)
    reach = 2 * ((1 << levels) - 1)
    w = 2 * ((reach + 15) // 16 * 16) + 384
    x = np.arange(w, dtype=np.float64)
    omega = 2.0 * np.pi / period
    img = np.broadcast_to(np.rint(30000.0 + 4000.0 * np.cos(omega * x)), (8, w)).astype(np.uint16)
    out, _ = sr.sharpen(img, gain_q8)
    assert out.min() > 0 and out.max() < 65535
    lo = (w - 384) // 2
    carrier = np.cos(omega * x[lo:lo + 384])
    amp_in = 2.0 * (img[3, lo:lo + 384].astype(np.float64) * carrier).mean()
    amp_out = 2.0 * (out[3, lo:lo + 384].astype(np.float64) * carrier).mean()
    t = sr.transfer(omega, (gain_q8 / 256.0).tolist())
    bound = sr.transfer_bound(gain_q8.tolist())
    print('period %d gains %s: T %.6f, amplitude %.4f for %.4f, off by %.4f of %.4f allowed' % (period, gains, t, amp_out, t * amp_in,
                                                                                                abs(amp_out - t * amp_in), bound))
    assert abs(amp_in - 4000.0) < 1.0 and bound < 12.0
    assert abs(amp_out - t * amp_in) <= bound
    assert abs(float(out[3, lo:lo + 384].mean()) - float(img[3, lo:lo + 384].mean())) <= bound / 2.0      # (T(0) = 1)


def test_accuracy_against_planted_truth():
    from solex_ser_recon_en_amd import sharpen

    def sigma_of(img, circle):
        return sharpen.sigma_from_median(sr.noise(img, (circle[0], circle[1], circle[2] * sharpen.DEFAULT_REGION))[0])

    def sharpen_of(img, circle):
        thr = sharpen.thresholds(sigma_of(img, circle), sharpen.DEFAULT_DENOISE, sharpen.DEFAULT_LEVELS)
        return sr.sharpen(img, [256] * sharpen.DEFAULT_LEVELS, thr)[0]

    got = sr.scene_measures(sigma_of, sharpen_of)
    print('sigma %.3f counts for %.3f planted: off by %.6f; residual noise on the smooth part %.6f of the planted'
          % (got['estimate'], sr.NOISE * 65535.0, got['sigma'], got['residual']))
    for key in ('sigma', 'residual'):
        assert got[key] <= sr.TOLERANCE[key], key
        assert sr.TOLERANCE[key] <= 1.3 * got[key], 'the bound on %s is no longer the measured value plus a quarter' % key
    # a planted sigma of 300 counts on a flat field
    flat = np.clip(np.rint(30000.0 + 300.0 * np.random.default_rng(1).standard_normal((400, 400))), 0, 65535).astype(np.uint16)
    est = sharpen.sigma_from_median(sr.noise(flat)[0])
    print('a planted sigma of 300 counts on 400 x 400 comes back as %.2f' % est)
    assert abs(est / 300.0 - 1.0) < 0.01             # the median of 160000 values: 1.2 / sqrt(n) = 0.3 % a standard error


def test_python_layer_argument_checks(monkeypatch):
    from solex_ser_recon_en_amd import sharpen
    assert sharpen.quantise_gains([0, 1, 1.8, 16]).tolist() == [0, 256, 461, 4096]
    for bad in ([], [1] * 7, [-0.1], [16.01], [float('nan')], [float('inf')]):
        with pytest.raises(ValueError):
            sharpen.quantise_gains(bad)
    for bad in (0, 7, 2.0, None):
        with pytest.raises(ValueError):
            sharpen.noise_factors(bad)
    f = sharpen.noise_factors(4)
    thr = sharpen.thresholds(262.0, (3, 1), 4)
    assert thr.tolist() == [int(np.rint(64 * 3 * 262.0 * f[0])), int(np.rint(64 * 262.0 * f[1])), 0, 0]
    assert sharpen.thresholds(1e9, (5,), 2).tolist() == [1 << 22, 0] and sharpen.thresholds(0.0, (3, 3), 2).tolist() == [0, 0]
    for sigma, denoise, levels in ((-1.0, (1,), 2), (float('nan'), (1,), 2), (1.0, (-1,), 2), (1.0, (1, 1, 1), 2), (1.0, (float('inf'),), 2), (1.0, (1,), 0)):
        with pytest.raises(ValueError):
            sharpen.thresholds(sigma, denoise, levels)
    assert sharpen._noise_circle(None, 0.9) is None and sharpen._noise_circle((-1, -1, -1), 0.9) is None
    assert sharpen._noise_circle((10, 20, 100), 0.5) == (10.0, 20.0, 50.0)
    for circle, region in (((1, 1, float('nan')), 0.9), ((1, 1, -2), 0.9), ((1, 1, 5), 0.0), ((1, 1, 5), float('inf'))):
        with pytest.raises(ValueError):
            sharpen._noise_circle(circle, region)
    assert abs(sharpen.sigma_from_median(64) - 1.0 / 0.6744897501960817 / f[0]) < 1e-15
    # the command line refuses before it touches a GPU
    for argv in (['x.ser', '--levels', '7'], ['x.ser', '--gains', '1,17'], ['x.ser', '--gains', '1,1,1', '--levels', '2'],
                 ['x.ser', '--denoise', '-1'], ['x.ser', '--circle', '1,2'], ['x.ser', '--region', '0'], ['x.ser', '-w', '1'],
                 ['no_such_file.ser'], ['no_such_file.png'], []):
        with pytest.raises(SystemExit):
            sharpen.main(argv)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit):
        sharpen.main(['x.ser'])


def test_c_entry_points_without_a_gpu():
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    px = 2000 * 2000
    base = lib.shg_wavelet_workspace_bytes(2000, 2000, 1)
    assert 0 < base <= 32768 and lib.shg_wavelet_workspace_bytes(2000, 2000, 3) == base
    assert lib.shg_wavelet_workspace_bytes(2000, 2000, 4) == base + px * (8 + 4)
    assert lib.shg_wavelet_workspace_bytes(2000, 2000, 5) == lib.shg_wavelet_workspace_bytes(2000, 2000, 6) == base + px * (8 + 8)
    for h, w, levels in ((0, 5, 1), (5, 0, 1), (16385, 5, 1), (5, 16385, 1), (5, 5, 0), (5, 5, 7), (-1, 5, 3)):
        assert lib.shg_wavelet_workspace_bytes(h, w, levels) == 0
    assert lib.shg_wavelet_workspace_bytes(16384, 16384, 6) == base + 16384 * 16384 * 16
    one = ctypes.c_void_p(4096)
    gains, thr = (ctypes.c_int32 * 6)(256, 256, 256, 256, 256, 256), (ctypes.c_int32 * 6)()
    big = 1 << 40

    def sharpen(img=one, h=8, w=8, pitch=8, levels=2, g=gains, t=thr, out=ctypes.c_void_p(8192), out_pitch=8, planes=None, ws=one, ws_bytes=big):
        return lib.shg_wavelet_sharpen_u16(img, h, w, pitch, levels, g, t, out, out_pitch, planes, ws, ws_bytes, None)

    for over in (dict(img=None), dict(g=None), dict(t=None), dict(out=None), dict(ws=None), dict(pitch=7), dict(out_pitch=7), dict(levels=0),
                 dict(levels=7), dict(ws_bytes=base - 1), dict(levels=4, ws_bytes=base + 64 * 12 - 1), dict(out=one),
                 dict(out=ctypes.c_void_p(4096 + 126)), dict(planes=ctypes.c_void_p(4096 - 8 * 8 * 4 * 3 + 4)), dict(planes=ctypes.c_void_p(8192 + 124))):
        assert sharpen(**over) == -1, over
        assert 'shg_wavelet_sharpen_u16' in _lib.last_error()
    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        assert sharpen(**over) == -3, over
    for j, (gv, tv) in enumerate(((-1, 0), (4097, 0), (256, -1), (256, (1 << 22) + 1))):
        g, t = (ctypes.c_int32 * 2)(256, 256), (ctypes.c_int32 * 2)(0, 0)
        g[j % 2], t[j % 2] = gv, tv
        assert sharpen(g=g, t=t) == -1

    def noise(img=one, h=8, w=8, pitch=8, circle=None, out2=ctypes.c_void_p(8192), ws=one, ws_bytes=big):
        c3 = None if circle is None else (ctypes.c_double * 3)(*circle)
        return lib.shg_wavelet_noise_u16(img, h, w, pitch, c3, out2, ws, ws_bytes, None)

    for over in (dict(img=None), dict(out2=None), dict(ws=None), dict(pitch=7), dict(ws_bytes=base - 1), dict(circle=(float('nan'), 1, 1)),
                 dict(circle=(1, float('inf'), 1)), dict(circle=(1, 1, float('nan')))):
        assert noise(**over) == -1, over
    for over in (dict(h=0), dict(w=16385)):
        assert noise(**over) == -3, over
