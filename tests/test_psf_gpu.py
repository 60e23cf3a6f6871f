"""Measuring the blur from the limb, on the GPU: shg_limb_profile_u16 bit for bit against tests/psf_ref.py on
the shapes where the kernel can go wrong, its refusals, shg_rl_deconvolve_xy_u16 against shg_rl_deconvolve_u16 and against the
restatement, and the library and the command line end to end."""
import os
import shutil

import numpy as np
import pytest

from solex_ser_recon_en_amd import psf as _psf  # noqa: F401  (no feature: no tests)
from tests import deconvolve_ref as dr
from tests import flatten_ref as fr
from tests import psf_ref as pr
from tests.linemaps_util import run_json, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
PAD, FILL, GUARD = 0xBEEF, 0xA5, 16


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import deconvolve, ops, psf
    from solex_ser_recon_en_amd._lib import lib
    return {'deconvolve': deconvolve, 'ops': ops, 'psf': psf, 'lib': lib}


def up16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.uint16)


def down16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def random_image(h, w, seed=0):
    return np.random.default_rng([h, w, seed]).integers(0, 65536, (h, w)).astype(np.uint16)


def run_profile(lib, img, circle, reach, sub, sectors, extra=7, table=None, **over):
    """shg_limb_profile_u16 on the image in a padded buffer into planted tables with guards -> (status, (count, sum, sumsq) or None,
    whether the image, its padding and the guards are as they were -- and, after a refusal, the tables too)."""
    h, w = img.shape
    host = np.full((h, w + extra), PAD, np.uint16)
    host[:, :w] = img
    buf = up16(host)
    entries = sectors * 2 * reach * sub if 0 < sectors <= 64 and 0 < reach <= 64 and 0 < sub <= 8 else 64
    sizes = (4 * entries, 8 * entries, 8 * entries)
    planted = [torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda') for n in sizes]
    if table is None:
        table = pr.thresholds(sectors if sectors % 8 == 0 and 8 <= sectors <= 64 else 32)
    table = np.ascontiguousarray(table, dtype=np.float64)
    c3 = np.ascontiguousarray(circle, dtype=np.float64)
    ptrs = [over.get(name, t.data_ptr() + GUARD) for name, t in zip(('count', 'total', 'sumsq'), planted)]
    st = lib.shg_limb_profile_u16(over.get('img_ptr', buf.data_ptr()), over.get('h', h), over.get('w', w), over.get('pitch', w + extra),
                                  over.get('circle_ptr', c3.ctypes.data), reach, sub, sectors,
                                  over.get('table_ptr', table.ctypes.data if table.size else None), ptrs[0], ptrs[1], ptrs[2], None)
    torch.cuda.synchronize()
    back = down16(buf)
    intact = np.array_equal(back[:, :w], img) and (back[:, w:] == PAD).all()
    raw = [t.cpu().numpy() for t in planted]
    intact = intact and all((r[:GUARD] == FILL).all() and (r[GUARD + n:] == FILL).all() for r, n in zip(raw, sizes))
    if st != 0:
        return st, None, bool(intact and all((r == FILL).all() for r in raw))
    shape = (sectors, 2 * reach * sub)
    got = tuple(r[GUARD:GUARD + n].copy().view(dt).reshape(shape) for r, n, dt in zip(raw, sizes, (np.uint32, np.uint64, np.uint64)))
    return st, got, bool(intact)


def check_profile(lib, img, circle, reach, sub, sectors, **how):
    st, got, intact = run_profile(lib, img, circle, reach, sub, sectors, **how)
    assert st == 0 and intact
    want = pr.limb_profile(img, circle, reach, sub, sectors)
    for name, g, wnt in zip(('count', 'sum', 'sumsq'), got, want):
        bad = np.argwhere(g != wnt)
        assert bad.size == 0, '%s: %d entries differ, first at %s: %d vs %d' % (name, len(bad), bad[0], g[tuple(bad[0])], wnt[tuple(bad[0])])
    return want


# ---- the tables, bit for bit ----
# (shape, extra, circle, reach, sub, sectors)
PROFILE_CASES = {
    'odd pitch, non-integer centre': ((97, 83), 96 + 7 - 83, (40.3, 51.6, 30.4), 12, 4, 32),
    'several tiles a sector': ((200, 190), 3, (93.7, 101.2, 80.4), 12, 4, 32),
    'centre outside the image': ((97, 83), 5, (-20.5, 110.25, 60.4), 12, 4, 32),
    'centre far outside': ((40, 50), 1, (-3000.5, 20.0, 3010.3), 12, 4, 16),
    'cut by two borders': ((97, 83), 7, (70.2, 80.9, 30.4), 12, 4, 32),
    'misses the image': ((97, 83), 7, (300.0, 300.0, 30.4), 12, 4, 32),
    'inside the hole': ((20, 20), 7, (10.0, 10.0, 60.0), 12, 4, 32),
    '8 sectors': ((97, 83), 7, (40.3, 51.6, 30.4), 12, 4, 8),
    '64 sectors': ((97, 83), 7, (40.3, 51.6, 30.4), 12, 4, 64),
    'sub 1': ((97, 83), 7, (40.3, 51.6, 30.4), 12, 1, 32),
    'sub 8': ((97, 83), 7, (40.3, 51.6, 30.4), 12, 8, 32),
    'reach 1': ((97, 83), 7, (40.3, 51.6, 30.4), 1, 4, 32),
    'reach rad - 1': ((97, 83), 7, (40.3, 51.6, 30.4), 29, 4, 32),
    'reach 64, sub 8, a small hole': ((160, 170), 2, (81.5, 77.25, 65.0), 64, 8, 64),
    'the smallest disk': ((9, 11), 2, (5.0, 4.0, 2.0), 1, 8, 64),
}


@pytest.mark.parametrize('name', list(PROFILE_CASES))
def test_profile_matches_the_restatement(mods, name):
    (h, w), extra, circle, reach, sub, sectors = PROFILE_CASES[name]
    want = check_profile(mods['lib'], random_image(h, w), circle, reach, sub, sectors, extra=extra)
    if name in ('misses the image', 'inside the hole'):
        assert all((t == 0).all() for t in want)
    else:
        assert want[0].sum() > 0


def test_profile_on_a_strip_at_the_limit(mods):
    img = random_image(3, 16384)
    want = check_profile(mods['lib'], img, (8000.5, 1.0, 8000.0), 12, 4, 32, extra=0)
    assert want[0].sum() > 100
    check_profile(mods['lib'], np.ascontiguousarray(img.T), (1.0, 8000.5, 8000.0), 12, 4, 32, extra=1)


def test_profile_sums_hold_the_extremes(mods):
    circle = (93.7, 101.2, 80.4)
    full = check_profile(mods['lib'], np.full((200, 190), 65535, np.uint16), circle, 12, 1, 8)
    assert full[0].max() > 40 and np.array_equal(full[2], full[0].astype(np.uint64) * np.uint64(65535 ** 2))        # past 2^37 an entry
    zero = check_profile(mods['lib'], np.zeros((200, 190), np.uint16), circle, 12, 1, 8)
    assert np.array_equal(zero[0], full[0]) and not zero[1].any() and not zero[2].any()


def test_profile_on_the_boundaries(mods):
    """An integer centre and radius: pixels exactly on dx = 0, dy = 0, |dx| = |dy|, and, with sub 4 and sub 8, distances that are
    exact multiples of 1 / sub (every Pythagorean pixel: 18^2 + 24^2 = 30^2, ...)."""
    img = random_image(101, 101, 3)
    for sub in (1, 4, 8):
        for sectors in (8, 32, 64):
            check_profile(mods['lib'], img, (50.0, 50.0, 30.0), 5, sub, sectors)
    # the thresholds are the caller's: a table of its own, and a pixel whose q equals a threshold exactly (dy / dx = 1 / 2, 1 / 4, 3 / 4)
    own = np.array([0.25, 0.5, 0.75])
    st, got, intact = run_profile(mods['lib'], img, (50.0, 50.0, 30.0), 5, 4, 32, table=own)
    assert st == 0 and intact
    for g, wnt in zip(got, pr.limb_profile(img, (50.0, 50.0, 30.0), 5, 4, 32, table=own)):
        assert np.array_equal(g, wnt)
    s, _, counts = pr.sector_and_bin(101, 101, (50.0, 50.0, 30.0), 5, 4, 32, own)
    assert counts[50 + 14, 50 + 28] and s[50 + 14, 50 + 28] == 2                  # q = 1/2 = thresholds[1]: the index above it


def test_profile_refusals_leave_the_tables_untouched(mods):
    lib = mods['lib']
    img = random_image(97, 83)
    circle = (40.3, 51.6, 30.4)
    nan, inf = float('nan'), float('inf')

    def refused(code, circle=circle, reach=12, sub=4, sectors=32, **over):
        st, _, intact = run_profile(lib, img, circle, reach, sub, sectors, **over)
        assert st == code and intact, (circle, reach, sub, sectors, over)

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        refused(E_UNSUPPORTED, **over)
    for over in (dict(img_ptr=None), dict(circle_ptr=None), dict(table_ptr=None), dict(count=None), dict(total=None), dict(sumsq=None), dict(pitch=82),
                 dict(circle=(nan, 51.6, 30.4)), dict(circle=(40.3, inf, 30.4)), dict(circle=(40.3, 51.6, nan)), dict(circle=(40.3, 51.6, -2.0)),
                 dict(circle=(40.3, 51.6, 16384.0)), dict(circle=(65536.0, 51.6, 30.4)), dict(circle=(40.3, -65536.0, 30.4)),
                 dict(reach=0), dict(reach=65), dict(reach=30), dict(circle=(40.3, 51.6, 12.5)), dict(sub=0), dict(sub=9),
                 dict(sectors=0), dict(sectors=12), dict(sectors=72), dict(table=[0.2, nan, 0.7]), dict(table=[0.2, 0.2, 0.7]),
                 dict(table=[0.5, 0.4, 0.7]), dict(table=[0.0, 0.4, 0.7]), dict(table=[0.2, 0.4, 1.0]), dict(table=[0.2, 0.4, inf])):
        refused(E_ARG, **over)
    # a table on the image, on its last element, and on another table
    buf = up16(np.full((97, 90), PAD, np.uint16))
    tables = [torch.full((8 * 32 * 96 + 64,), FILL, dtype=torch.uint8, device='cuda') for _ in range(3)]
    a, b, c = (t.data_ptr() for t in tables)
    c3, thr = np.array(circle), pr.thresholds(32)
    last = 2 * (96 * 90 + 82)
    for count, total, sumsq in ((buf.data_ptr(), b, c), (a, buf.data_ptr() + last - 6, c), (a, b, buf.data_ptr() - 8 * 32 * 96 + 8), (a, a, c),
                                (a, b, b + 8 * 32 * 96 - 8), (a, a + 4 * 32 * 96 - 8, c), (c + 8 * 32 * 96 - 8, b, c)):
        assert lib.shg_limb_profile_u16(buf.data_ptr(), 97, 83, 90, c3.ctypes.data, 12, 4, 32, thr.ctypes.data, count, total, sumsq, None) == E_ARG
    torch.cuda.synchronize()
    assert (down16(buf) == PAD).all() and all((t.cpu().numpy() == FILL).all() for t in tables)
    # the wrapper: a ValueError before the call
    ops = mods['ops']
    dev = up16(img)
    for bad in (dict(circle=(1.0, 2.0)), dict(circle=(1.0, nan, 40.0)), dict(reach=0), dict(reach=30), dict(reach=2.5), dict(sub=9), dict(sectors=12),
                dict(thresholds=[0.5])):
        args = dict(circle=circle, reach=12, sub=4, sectors=32)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.limb_profile_u16(dev, **args)


# ---- a tap set an axis ----
def call_xy(lib, img, taps_x, taps_y, iterations, extra=3, out_extra=1):
    """shg_rl_deconvolve_xy_u16 (taps_y None: shg_rl_deconvolve_u16) -> (out, the estimate's bits)."""
    h, w = img.shape
    host = np.full((h, w + extra), PAD, np.uint16)
    host[:, :w] = img
    buf = up16(host)
    out = up16(np.full((h, w + out_extra), 0x5A5A, np.uint16))
    est = torch.full((h, w), 0x7A7A7A7A, dtype=torch.int32, device='cuda')
    need = lib.shg_rl_workspace_bytes(h, w)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    kx = np.ascontiguousarray(taps_x, dtype=np.float32)
    if taps_y is None:
        st = lib.shg_rl_deconvolve_u16(buf.data_ptr(), h, w, w + extra, kx.ctypes.data, kx.size // 2, iterations, out.data_ptr(), w + out_extra,
                                       est.data_ptr(), ws.data_ptr(), need, None)
    else:
        ky = np.ascontiguousarray(taps_y, dtype=np.float32)
        st = lib.shg_rl_deconvolve_xy_u16(buf.data_ptr(), h, w, w + extra, kx.ctypes.data, kx.size // 2, ky.ctypes.data, ky.size // 2, iterations,
                                          out.data_ptr(), w + out_extra, est.data_ptr(), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert st == 0
    got = down16(out)
    assert (got[:, w:] == 0x5A5A).all() and np.array_equal(down16(buf), host)
    return got[:, :w].copy(), est.cpu().numpy()


def asymmetric(sigma, radius):
    if radius == 0:
        return np.ones(1, np.float32)
    k = dr.gaussian(sigma, radius).astype(np.float64) * np.linspace(0.5, 1.5, 2 * radius + 1)
    return (k / k.sum()).astype(np.float32)


@pytest.mark.parametrize('radius', [1, 5, 16])
@pytest.mark.parametrize('iterations', [1, 3])
def test_equal_taps_give_the_bits_of_the_one_set_call(mods, radius, iterations):
    img = random_image(45, 70)                                                # more than one tile along x, a partial tile both ways
    k = asymmetric({1: 0.6, 5: 1.4, 16: 4.0}[radius], radius)
    out, est = call_xy(mods['lib'], img, k, k, iterations)
    out_one, est_one = call_xy(mods['lib'], img, k, None, iterations)
    assert np.array_equal(out, out_one) and np.array_equal(est, est_one)


@pytest.mark.parametrize('radii', [(2, 9), (16, 0), (9, 2), (0, 16)])
def test_unequal_taps_match_the_restatement(mods, radii):
    rx, ry = radii
    kx, ky = asymmetric(0.4 * rx + 0.5, rx), asymmetric(0.4 * ry + 0.5, ry)
    for img, n in ((random_image(45, 70), 3), (dr.zero_sky_disk(45, 70), 2)):
        out, est = call_xy(mods['lib'], img, kx, ky, n)
        want, e = pr.deconvolve_xy(img, kx, ky, n)
        assert np.array_equal(out, want) and np.array_equal(est, bits(e))


def test_a_transposed_image_with_swapped_taps(mods):
    """Transposing swaps the order of the two passes, and float32 sums are not associative: the transposed call is the restatement of
    the transposed problem bit for bit, and the transposed result within psf_ref.transpose_bound of one iteration."""
    img = random_image(45, 70, 1)
    kx, ky = asymmetric(1.3, 2), asymmetric(3.0, 9)
    turned = np.ascontiguousarray(img.T)
    out_t, est_t = call_xy(mods['lib'], turned, ky, kx, 1)
    want_t, e_t = pr.deconvolve_xy(turned, ky, kx, 1)
    assert np.array_equal(out_t, want_t) and np.array_equal(est_t, bits(e_t))
    out, est = call_xy(mods['lib'], img, kx, ky, 1)
    e, e_turned = est.view(np.float32).astype(np.float64), est_t.view(np.float32).astype(np.float64).T
    assert (np.abs(e - e_turned) <= pr.transpose_bound(kx, ky) * np.maximum(e, e_turned)).all()
    assert np.abs(out.astype(np.int64) - out_t.T.astype(np.int64)).max() <= int(np.ceil(pr.transpose_bound(kx, ky) * e.max())) + 1


# ---- end to end ----
def test_estimate_and_deconvolve_reproduce_the_cpu_figures(mods):
    psf, deconvolve = mods['psf'], mods['deconvolve']
    img = pr.limb_scene(1.0, 2.0, pr.NOISE, seed=1)
    dev = up16(img)
    count, total, sumsq, t = psf.limb_profiles(dev, pr.CIRCLE)
    want = pr.limb_profile(img, pr.CIRCLE, 12, 4, 32)
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip((count, total, sumsq), want)) and np.array_equal(t, psf.bin_centres(12, 4))
    est, cpu = psf.estimate_psf(dev, pr.CIRCLE), pr.estimate(img)
    for key in ('sigma_x', 'sigma_y', 'isotropic', 'n_used', 'rms', 'sectors'):
        assert est[key] == cpu[key], key
    assert abs(est['sigma_x'] - pr.expected(1.0)) <= pr.TOLERANCE['recovery'] and abs(est['sigma_y'] - pr.expected(2.0)) <= pr.TOLERANCE['recovery']
    small = np.ascontiguousarray(img[60:130, 20:110])
    pair = (est['sigma_x'], est['sigma_y'])
    out, rec = deconvolve.deconvolve_disk(up16(small), sigma=pair, iterations=3)
    kx, ky = deconvolve.gaussian_taps(pair[0]), deconvolve.gaussian_taps(pair[1])
    assert rec['sigma'] == list(pair) and rec['radius'] == [5, 9] and rec['taps'] == [[float(v) for v in kx], [float(v) for v in ky]]
    assert np.array_equal(down16(out), pr.deconvolve_xy(small, kx, ky, 3)[0])
    # a pair that does not differ goes the one-set way, and a pair of arrays like a pair of widths
    out, rec = deconvolve.deconvolve_disk(up16(small), sigma=(1.5, 1.5), iterations=2)
    assert rec['radius'] == 6 and np.array_equal(down16(out), dr.deconvolve(small, deconvolve.gaussian_taps(1.5), 2)[0])
    out, rec = deconvolve.deconvolve_disk(up16(small), taps=(kx, ky), iterations=3, limb={'circle': (104.3, 71.7, 100.4)})
    assert rec['limb']['margin'] == 9.0 and rec['radius'] == [5, 9]


def blurred_scan():
    """flatten_ref's scan with a blur of its own: a Gaussian of 1.5 frames along the scan and of 1.5 px along the slit (the frames
    are in file layout, [frame, sample, slit row])."""
    frames = fr.pipeline_scan().astype(np.float64)
    k = pr.gaussian64(1.5)
    r = k.size // 2
    for axis in (0, 2):
        n = frames.shape[axis]
        idx = [np.clip(np.arange(n) + i, 0, n - 1) for i in range(-r, r + 1)]
        frames = sum(k[j] * np.take(frames, idx[j], axis=axis) for j in range(k.size))
    return np.clip(np.rint(frames), 0, 65535).astype(np.uint16)


def test_command_lines_on_a_scan(mods, tmp_path_factory, tmp_path, capsys):
    from solex_ser_recon_en_amd import disk
    from solex_ser_recon_en_amd.png_io import read_png_gray
    psf, deconvolve = mods['psf'], mods['deconvolve']
    work = str(tmp_path / 'scan.ser')
    shutil.copy(write_scan(tmp_path_factory, 'psf', blurred_scan()), work)
    own = disk.scan_disk(work)
    image = down16(own['image'])
    cpu = pr.estimate(image, own['circle'])
    out = run_json(psf.main, capsys, [work])
    assert (out['sigma_x'], out['sigma_y'], out['n_used'], out['isotropic']) == (cpu['sigma_x'], cpu['sigma_y'], cpu['n_used'], cpu['isotropic'])
    assert out['circle'] == list(own['circle']) and out['shift'] == 0 and out['esf'] == work[:-4] + '_shift=0_esf.txt' and os.path.exists(out['esf'])
    assert np.loadtxt(out['esf']).shape == (32 * 96, 6)
    out = run_json(deconvolve.main, capsys, [work, '--psf-sigma', 'auto', '--iterations', '2'])
    assert out['psf'] == {k: cpu[k] for k in ('sigma_x', 'sigma_y', 'isotropic', 'n_used', 'rms')}
    pair = [min(max(cpu[k], deconvolve.MIN_SIGMA), deconvolve.MAX_SIGMA) for k in ('sigma_x', 'sigma_y')]
    assert out['psf_sigma'] == pair and out['png'] == work[:-4] + '_shift=0_deconv.png' and out['iterations'] == 2
    kx, ky = deconvolve.gaussian_taps(pair[0]), deconvolve.gaussian_taps(pair[1])
    want = dr.deconvolve(image, kx, 2)[0] if kx.tobytes() == ky.tobytes() else pr.deconvolve_xy(image, kx, ky, 2)[0]
    from solex_ser_recon_en_amd import SHG_MAIN
    assert np.array_equal(read_png_gray(out['png']), np.rot90(want, SHG_MAIN.default_options()['img_rotate'] // 90))
