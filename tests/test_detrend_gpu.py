"""The plane removal on the GPU: shg_map_plane_moments and shg_map_detrend bit for bit against the restatement written from the
header (tests/detrend_ref.py) -- the ten integers on planted values, circles with pixels on, just inside and just outside, clipping
limits met exactly, unaligned rows, many workgroups and the 8192 x 8192 limit; the detrended map and its display plane out of place
and in place with every element beyond w untouched; the rejected arguments; linemaps.detrend_plane's loop; dopplergram(...,
detrend='plane') and the command line."""
import math

import numpy as np
import pytest

from tests import detrend_ref as dr
from tests import linemaps_ref as ref
from tests.linemaps_util import IH, IW, N, run_json, same_bits, scan_reader, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
MAP_FILL, OUT_FILL, PNG_FILL = 12345.0, -777.0, 0xBEEF
GARBAGE = -0x0123456789ABCDEF
BIG = np.float32(63.999996)                    # the largest float32 below 64: q = 2^18


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import doppler, linemaps, ops
    from solex_ser_recon_en_amd._lib import lib
    return doppler, linemaps, ops, lib


def planted(h, w, seed):
    """normal(0, 0.8) with 5 % NaN and, where they fit, the values the rules turn on: the infinities, the zeros and denormals, the
    |v| < 64 edge, 1e30 and q's rounding ties (2k + 1) / 8192 for even and odd k, both signs."""
    rng = np.random.default_rng([seed, h, w])
    m = rng.normal(0.0, 0.8, (h, w)).astype(np.float32)
    m[rng.random((h, w)) < 0.05] = np.nan
    ties = [(2 * k + 1) / 8192.0 for k in (0, 1, 2, 3, 1000, 1001, 262142, 262143)]
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-42, BIG, -BIG, 64.0, -64.0, 1e30, -1e30] + ties + [-t for t in ties],
                       dtype=np.float32)
    if m.size >= 4 * special.size:
        at = rng.choice(m.size, 2 * special.size, replace=False)
        m.flat[at] = np.resize(special, at.size)
    return m


def on_device(m, extra, fill=MAP_FILL):
    """m in a buffer whose pitch is w + extra, the rest `fill` -> (the [h, w] view, the buffer)."""
    h, w = m.shape
    buf = torch.full((h, w + extra), fill, dtype=torch.float32, device='cuda')
    buf[:, :w].copy_(torch.from_numpy(m))
    return buf[:, :w], buf


def circles(h, w):
    """Integer centres, so the Pythagorean pixels lie exactly on the circle in float64: pixels on (radius 5: (3, 4)), just inside
    (nextafter(10): (6, 8)) and just outside (the radius just below 13: (5, 12)), radii whose square rounds, and fractions."""
    cx, cy = float(w // 2), float(h // 2)
    return [None, (-1.0, -1.0, -1.0), (cx, cy, 5.0), (cx, cy, math.nextafter(10.0, 11.0)), (cx, cy, math.nextafter(13.0, 0.0)),
            (cx, cy, math.sqrt(65.0)), (cx, cy, math.sqrt(145.0)), (cx - 0.3, cy + 0.4, 0.37 * min(h, w) + 0.55)]


PREV = (0.25, 1.0 / 64.0, -1.0 / 128.0, 0.5)   # small dyadic rationals: a + b c + g r and the residuals are exact in float64


def plant_limit(m, seed):
    """Pixels whose residual against PREV is +-limit exactly (used: the test is <=) and one float32 step beyond (not used)."""
    a, b, g, limit = PREV
    h, w = m.shape
    rng = np.random.default_rng([seed, 77])
    at = rng.choice(m.size, min(m.size, 16), replace=False)
    for i, flat in enumerate(at):
        r, c = divmod(int(flat), w)
        edge = np.float32((a + b * c + g * r) + (limit if i % 2 else -limit))
        assert float(edge) == (a + b * c + g * r) + (limit if i % 2 else -limit) and abs(edge) < 60
        m[r, c] = edge if i % 4 < 2 else np.nextafter(edge, np.float32(100.0 if i % 2 else -100.0))
    return m


def moments(ops, view, circle=None, prev=None):
    out = torch.full((10,), GARBAGE, dtype=torch.int64, device='cuda')           # the call overwrites, it does not add
    got = ops.map_plane_moments(view, circle, prev, out)
    assert got.data_ptr() == out.data_ptr()
    return [int(v) for v in got.cpu().numpy()]


# (rows of 1023 + 13 elements start on 16 bytes, rows of 1023 + 14 do not: the two load paths at the same size)
SHAPES = [(1, 1, 0), (3, 5, 0), (64, 64, 0), (257, 1023, 13), (257, 1023, 14), (400, 500, 12), (2048, 2048, 0)]


@pytest.mark.parametrize('h, w, extra', SHAPES, ids=['%dx%d+%d' % s for s in SHAPES])
def test_moments_equal_the_restatement(mods, h, w, extra):
    _, _, ops, _ = mods
    m = plant_limit(planted(h, w, 1), 2)
    view, buf = on_device(m, extra)
    some = circles(h, w) if h * w < 10 ** 6 else [None, circles(h, w)[3], circles(h, w)[-1]]
    reached = set()
    for circle in some:
        for prev in (None, PREV, PREV[:3] + (0.0,), PREV[:3] + (math.inf,)) if h * w < 10 ** 6 else (None, PREV):
            want = dr.plane_moments(m, circle, prev)
            assert moments(ops, view, circle, prev) == want, (circle, prev)
            reached.add((circle is not None and circle[0] >= 0, prev is not None, want[0] > 0))
    assert np.array_equal(buf.cpu().numpy()[:, w:], np.full((h, extra), MAP_FILL, dtype=np.float32))
    if h >= 64:
        assert reached >= {(x, y, True) for x in (False, True) for y in (False, True)}
        # the planted edges are where they were meant to be: on the limit and used, a step beyond and not
        used = dr.used_pixels(m, None, PREV)
        res = np.abs(m.astype(np.float64) - ((PREV[0] + PREV[1] * np.arange(w)[None, :]) + PREV[2] * np.arange(h)[:, None]))
        assert (used & (res == PREV[3])).sum() >= 4 and (~used & (res > PREV[3]) & (res < PREV[3] + 1e-5)).sum() >= 4
        on = dr.used_pixels(m, circles(h, w)[2]) ^ dr.used_pixels(m, (w // 2, h // 2, math.nextafter(5.0, 0.0)))
        assert on.sum() >= 4                                                     # pixels exactly on the radius-5 circle count


def test_moments_at_the_size_limit(mods):
    """8192 x 8192, +-63.999996 on alternate rows (q = +-2^18): the ten sums from closed forms.  A 32-bit intermediate or a carelessly
    written 64-bit accumulator goes wrong here: sum q^2 = 2^62."""
    _, _, ops, _ = mods
    n = dr.MAX_DIM
    m = torch.empty((n, n), dtype=torch.float32, device='cuda')                  # 256 MB, allocated once
    m[0::2] = float(BIG)
    m[1::2] = -float(BIG)
    want = dr.closed_form_rows(n, n, 2 ** 18, -2 ** 18)
    assert want[9] == 2 ** 62 and want[0] == 2 ** 26
    assert moments(ops, m) == want
    assert moments(ops, m, None, (0.0, 0.0, 0.0, math.inf)) == want              # the clipping path at that size
    assert moments(ops, m, (4096.0, 4096.0, 1e5)) == want                        # and the mask's
    m[1::2] = float(BIG)                                                         # every term of one sign
    assert moments(ops, m) == dr.closed_form_rows(n, n, 2 ** 18, 2 ** 18)


def raw_detrend(lib, ops, m, plane, extra, out_extra, png_extra, display_range, in_place=False, png=True, **over):
    """shg_map_detrend on m in pitched, sentinel-filled buffers -> (status, out, png, whether everything else kept its fill)."""
    h, w = m.shape
    view, buf = on_device(m, extra)
    obuf = buf if in_place else torch.full((h, w + out_extra), OUT_FILL, dtype=torch.float32, device='cuda')
    pbuf = torch.full((h, w + png_extra), PNG_FILL - 65536, dtype=torch.int16, device='cuda') if png else None
    p3 = np.ascontiguousarray(plane, dtype=np.float64)
    st = lib.shg_map_detrend(view.data_ptr(), over.get('h', h), over.get('w', w), over.get('pitch', buf.stride(0)), p3.ctypes.data,
                             obuf.data_ptr(), over.get('out_pitch', obuf.stride(0)), None if pbuf is None else pbuf.data_ptr(),
                             0 if pbuf is None else over.get('png_pitch', pbuf.stride(0)), display_range, ops._stream())
    torch.cuda.synchronize()
    o, p = obuf.cpu().numpy(), None if pbuf is None else pbuf.cpu().numpy().view(np.uint16)
    fill = MAP_FILL if in_place else OUT_FILL
    if st != 0:
        untouched = (np.array_equal(o[:, :w].view(np.uint32), m.view(np.uint32)) if in_place else bool((o == fill).all())) and \
            (p is None or bool((p == PNG_FILL).all()))
        return st, None, None, untouched
    clean = bool((o[:, w:] == fill).all()) and (p is None or bool((p[:, w:] == PNG_FILL).all()))
    if not in_place:
        assert np.array_equal(buf.cpu().numpy()[:, :w].view(np.uint32), m.view(np.uint32)), 'the call wrote into its input'
    return st, o[:, :w], None if p is None else p[:, :w], clean


LAYOUTS = [(3, 5, 0, 0, 0), (3, 5, 1, 2, 3), (64, 64, 0, 0, 0), (257, 1023, 13, 5, 7), (400, 500, 12, 4, 8), (130, 1500, 0, 0, 2),
           (33, 2052, 0, 4, 0)]


@pytest.mark.parametrize('h, w, extra, out_extra, png_extra', LAYOUTS, ids=['%dx%d+%d' % s[:3] for s in LAYOUTS])
def test_detrend_equals_the_restatement(mods, h, w, extra, out_extra, png_extra):
    _, _, ops, lib = mods
    m = planted(h, w, 3)
    plane = (-0.731, 0.010033, -0.00217)
    want, want_png = dr.detrend(m, plane, 1.7)
    for in_place in (False, True):
        st, got, png, clean = raw_detrend(lib, ops, m, plane, extra, out_extra, png_extra, 1.7, in_place)
        assert st == 0 and clean, 'an element beyond w was written'
        same_bits(got, want)
        assert np.array_equal(png, want_png)
        st, got, none, clean = raw_detrend(lib, ops, m, plane, extra, out_extra, png_extra, 0.0, in_place, png=False)
        assert st == 0 and clean and none is None
        same_bits(got, want)
    assert np.isnan(want).sum() == np.isnan(m).sum() > 0 or m.size < 100
    assert np.array_equal(np.isinf(want), np.isinf(m))
    # the wrapper: a new output, the display plane only when asked for, and the map itself as the output
    view, _ = on_device(m, extra)
    out, png = ops.map_detrend(view, plane, 1.7)
    same_bits(out.cpu().numpy(), want)
    assert np.array_equal(png.cpu().numpy(), want_png)
    out, none = ops.map_detrend(view, plane, out=view)
    assert none is None and out.data_ptr() == view.data_ptr()
    same_bits(view.cpu().numpy(), want)


def test_rejected_arguments_write_nothing(mods):
    """Only bad arguments: every one is refused on the host, before anything reaches the device."""
    _, _, ops, lib = mods
    m = planted(24, 40, 4)
    view, buf = on_device(m, 3)
    pitch = buf.stride(0)

    def moments_status(h=24, w=40, p=pitch, prev=None, slots=True, src=True):
        out = torch.full((10,), GARBAGE, dtype=torch.int64, device='cuda')
        p4 = None if prev is None else np.ascontiguousarray(prev, dtype=np.float64)
        st = lib.shg_map_plane_moments(view.data_ptr() if src else None, h, w, p, None, None if p4 is None else p4.ctypes.data,
                                       out.data_ptr() if slots else None, ops._stream())
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == GARBAGE).all() or st == 0
        return st

    assert moments_status() == 0
    assert moments_status(h=8193) == E_UNSUPPORTED and moments_status(w=8193, p=8193) == E_UNSUPPORTED
    assert moments_status(h=0) == E_UNSUPPORTED and moments_status(w=0) == E_UNSUPPORTED
    assert moments_status(p=39) == E_ARG
    assert moments_status(prev=(0.0, 0.0, 0.0, -1e-300)) == E_ARG and moments_status(prev=(0.0, 0.0, 0.0, math.nan)) == E_ARG
    assert moments_status(prev=(0.0, math.inf, 0.0, 1.0)) == E_ARG
    assert moments_status(prev=(0.0, 0.0, 0.0, 0.0)) == 0 and moments_status(prev=(0.0, 0.0, 0.0, math.inf)) == 0
    assert moments_status(slots=False) == E_ARG and moments_status(src=False) == E_ARG
    plane = (0.1, 0.2, 0.3)
    for in_place in (False, True):
        for want, plane_, over, rng in ((E_UNSUPPORTED, plane, {'h': 8193}, 1.7), (E_UNSUPPORTED, plane, {'w': 8193, 'pitch': 8200}, 1.7),
                                        (E_ARG, plane, {'pitch': 39}, 1.7), (E_ARG, plane, {'png_pitch': 39}, 1.7),
                                        (E_ARG, (math.nan, 0.0, 0.0), {}, 1.7), (E_ARG, (0.0, math.inf, 0.0), {}, 1.7),
                                        (E_ARG, (0.0, 0.0, -math.inf), {}, 1.7), (E_ARG, plane, {}, 0.0), (E_ARG, plane, {}, math.nan)):
            st, _, _, untouched = raw_detrend(lib, ops, m, plane_, 3, 5, 7, rng, in_place, **over)
            assert st == want and untouched, (want, plane_, over, rng, in_place)
    st, _, _, untouched = raw_detrend(lib, ops, m, plane, 3, 5, 7, 1.7, False, out_pitch=39)
    assert st == E_ARG and untouched
    st, _, _, untouched = raw_detrend(lib, ops, m, plane, 3, 5, 7, 1.7, True, out_pitch=44)      # in place wants equal pitches
    assert st == E_ARG and untouched


# ---- linemaps.detrend_plane ----
def traced(monkeypatch, ops):
    seen = []
    real = ops.map_plane_moments

    def spy(*args, **kw):
        out = real(*args, **kw)
        seen.append([int(v) for v in out.cpu().numpy()])
        return out

    monkeypatch.setattr(ops, 'map_plane_moments', spy)
    return seen


def same_info(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k] == v and type(got[k]) is type(v), (k, got[k], v)


def test_detrend_plane_follows_the_restatements_loop(mods, monkeypatch):
    _, linemaps, ops, _ = mods
    seen = traced(monkeypatch, ops)
    rng = np.random.default_rng(8)
    h, w = 300, 421
    r, c = np.indices((h, w))
    m = (0.4 + 0.01 * c - 0.004 * r + rng.normal(0.0, 0.1, (h, w))).astype(np.float32)
    m[rng.random((h, w)) < 0.03] += 3.0                                          # outliers the clipping drops
    m[rng.random((h, w)) < 0.05] = np.nan
    circle = (200.0, 150.0, 140.5)
    for kw in ({}, {'circle': circle, 'display_range': 1.5}, {'circle': circle, 'clip': 2.0, 'iterations': 16},
               {'circle': circle, 'clip': 4.0, 'iterations': 16}, {'iterations': 0}, {'iterations': 1, 'clip': 2.5}):
        del seen[:]
        want, want_png, info, trace = dr.detrend_plane(m, **kw)
        got, png, got_info = linemaps.detrend_plane(torch.from_numpy(m).cuda(), **kw)
        assert seen == trace and got_info['passes'] == len(trace)
        same_info(got_info, info)
        same_bits(got.cpu().numpy(), want)
        assert (png is None) == (want_png is None) and (png is None or np.array_equal(png.cpu().numpy(), want_png))
        assert ('limb_amplitude' in got_info) == ('circle' in kw)
        if kw.get('iterations', 3) == 0:
            assert len(trace) == 1 and got_info['n_used'] == got_info['n_valid']
        elif kw.get('iterations') == 16:
            # at 2 sigma every pass cuts the noise's own tails again: all sixteen run; at 4 sigma a pass drops nothing more: early end
            assert len(trace) == (17 if kw['clip'] == 2.0 else 4) and (len(trace) == 17 or trace[-1][0] == trace[-2][0])
            assert got_info['n_used'] < got_info['n_valid']
        else:
            assert got_info['n_used'] < got_info['n_valid'] and abs(got_info['b'] - 0.01) < 1e-4
    # a NumPy map goes up and the results come back as arrays
    out, png, info2 = linemaps.detrend_plane(m, iterations=1, clip=2.5)
    assert isinstance(out, np.ndarray) and png is None
    same_info(info2, info)
    same_bits(out, want)


def test_detrend_plane_stops_on_an_exact_plane(mods, monkeypatch):
    _, linemaps, ops, _ = mods
    seen = traced(monkeypatch, ops)
    r, c = np.indices((50, 70))
    a, b, g = 300 / 4096, 21 / 4096, -8 / 4096
    m = (a + b * c + g * r).astype(np.float32)
    out, _, info = linemaps.detrend_plane(torch.from_numpy(m).cuda())
    assert len(seen) == 1 and info['passes'] == 1 and info['sigma'] == 0.0 and (info['a'], info['b'], info['g']) == (a, b, g)
    assert not out.cpu().numpy().any()
    flat = torch.zeros((2, 2), dtype=torch.float32, device='cuda')
    flat[0, 0] = float('nan')
    with pytest.raises(ValueError):
        linemaps.detrend_plane(flat)                                             # three pixels: no fit


# ---- dopplergram(..., detrend='plane') ----
def ramp_in_the_map(res, plane):
    """The injected ramp rises 3 / (N - 1) px a frame.  The finish reads raw column x = h00 c + h01 r + h02 at map pixel (r, c), so
    in the map the ramp's column term is b = slope h00.  The bound is a tenth of the slope, 1e-3 px a raw column, in the map's
    units: the restatement's unclipped fit, which the clipped one must beat, is 6.5 % off on the CPU (detrend_ref.TOLERANCE's
    comment).  g is not held to the ramp: the shift is measured against the scan's own fitted line, whose zero moves from row to
    row with what the field averages to along that row's chord, and that row term is the map's own."""
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    _, _, mat3, _, _, _, _ = _warp_geometry(res['phi'], res['ratio'], IH, N)
    slope, h00, h01 = 3.0 / (N - 1), float(mat3[0, 0]), float(mat3[0, 1])
    print('ramp in the map: b %.6f (slope h00 = %.6f), g %.6f (slope h01 = %.6f)' % (plane['b'], slope * h00, plane['g'], slope * h01))
    assert abs(plane['b'] - slope * h00) < 1e-3 * abs(h00)


@pytest.mark.parametrize('noise', [0.0, 0.004])
def test_dopplergram_detrend(mods, noise):
    doppler, _, _, _ = mods
    frames, _, _ = ref.doppler_scan(ref.injected_field(IH, N), IW, noise=noise, seed=3)
    plain = doppler.dopplergram(scan_reader(frames))
    res = doppler.dopplergram(scan_reader(frames), detrend='plane')
    assert sorted(set(res) - set(plain)) == ['detrended', 'detrended_png', 'plane'] and plain['crop'] is None
    for k in ('map', 'png', 'raw'):
        assert res[k].dtype == plain[k].dtype and np.array_equal(res[k].view(np.uint8), plain[k].view(np.uint8)), k
    assert res['circle'] != (-1, -1, -1)
    want, want_png, info, _ = dr.detrend_plane(res['map'], res['circle'], 3.0, 3, 2.0)
    same_bits(res['detrended'], want)
    assert res['detrended'].dtype == np.float32 and np.array_equal(res['detrended_png'], want_png)
    same_info(res['plane'], info)
    print('noise %g: plane %s' % (noise, res['plane']))
    assert info['limb_amplitude'] == info['gradient'] * res['circle'][2]
    ramp_in_the_map(res, info)
    # other clipping, and km/s
    kms = doppler.dopplergram(scan_reader(frames), dispersion=0.05, wavelength=6562.8, detrend='plane', clip=2.0, clip_iterations=1)
    factor = (0.05 / 6562.8) * ref.C_KM_S
    want2, want_png2, info2, _ = dr.detrend_plane(res['map'], res['circle'], 2.0, 1, 2.0)
    same_bits(kms['detrended'], (want2.astype(np.float64) * factor).astype(np.float32))
    assert np.array_equal(kms['detrended_png'], want_png2) and kms['units'] == 'km/s'
    same_info(kms['plane'], dict(info2, b_kms=info2['b'] * factor, g_kms=info2['g'] * factor, sigma_kms=info2['sigma'] * factor,
                                 limb_amplitude_kms=info2['limb_amplitude'] * factor))
    with pytest.raises(ValueError):
        doppler.dopplergram(scan_reader(frames), detrend='quadric')


def test_dopplergram_detrend_in_a_cropped_map(mods):
    """With a crop the map's columns start at the crop: the mask moves with them, and the fit is the restatement's on the map with
    the circle in the map's own columns."""
    doppler, _, _, _ = mods
    from solex_ser_recon_en_amd import SHG_MAIN
    frames, _, _ = ref.doppler_scan(ref.injected_field(IH, N), IW, noise=0.004, seed=3)
    res = doppler.dopplergram(scan_reader(frames), dict(SHG_MAIN.default_options(), fixed_width=360), detrend='plane')
    nw, lo, dx0, n = res['crop']
    assert dx0 > 0 or lo > 0
    from solex_ser_recon_en_amd.linemaps import finish_circle
    fc = finish_circle(res['circle'], res['crop'], res['circle_out'])
    want, want_png, info, _ = dr.detrend_plane(res['map'], (fc[0] - lo + dx0, fc[1], fc[2]), 3.0, 3, 2.0)
    same_bits(res['detrended'], want)
    same_info(res['plane'], info)
    finite = int(np.isfinite(res['map']).sum())                                  # the disk's pixels, but for a rounding on its rim
    assert np.array_equal(res['detrended_png'], want_png) and 0.99 * finite < info['n_valid'] <= finite


# ---- the command line ----
@pytest.fixture(scope='module')
def scan_file(tmp_path_factory):
    return write_scan(tmp_path_factory, 'detrend', ref.doppler_scan(ref.injected_field(IH, N), IW, noise=0.004, seed=4)[0])


@pytest.mark.parametrize('rotate', [0, 90])
def test_cli_writes_the_detrended_pair(mods, scan_file, capsys, tmp_path, monkeypatch, rotate):
    doppler, _, _, _ = mods
    import shutil
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    options = dict(SHG_MAIN.default_options(), img_rotate=rotate)
    monkeypatch.setattr(SHG_MAIN, 'default_options', lambda: dict(options))
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir()
    b.mkdir()
    shutil.copy(scan_file, a / 'scan.ser')
    shutil.copy(scan_file, b / 'scan.ser')
    plain = run_json(doppler.main, capsys, [str(a / 'scan.ser')])
    got = run_json(doppler.main, capsys, [str(b / 'scan.ser'), '--detrend', 'plane', '--clip', '2.5'])
    for k in ('fits', 'png'):                                                    # the usual pair, byte for byte
        assert open(got[k], 'rb').read() == open(plain[k], 'rb').read()
    assert sorted(set(got) - set(plain)) == ['detrended_fits', 'detrended_png', 'plane']
    assert {k: got[k] for k in plain if k not in ('fits', 'png')} == {k: plain[k] for k in plain if k not in ('fits', 'png')}
    assert got['detrended_fits'] == str(b / 'scan_doppler_detrended.fits') and got['detrended_png'] == str(b / 'scan_doppler_detrended.png')
    res = doppler.dopplergram(str(b / 'scan.ser'), options, detrend='plane', clip=2.5)
    m, cards = read_fits_f32(got['detrended_fits'])
    same_bits(m, np.rot90(res['detrended'], rotate // 90))
    assert np.array_equal(read_png_gray(got['detrended_png']), np.rot90(res['detrended_png'], rotate // 90))
    assert got['shape'] == list(m.shape) and got['plane'] == res['plane']
    plane = got['plane']
    assert cards['DETREND'] == "'plane   '" and cards['BUNIT'] == "'pixel   '" and cards['HALFWID'] == '5'
    assert [float(cards[k]) for k in ('DTA', 'DTB', 'DTG', 'DTSIGMA')] == [plane[k] for k in ('a', 'b', 'g', 'sigma')]
    assert int(cards['DTNUSED']) == plane['n_used'] < plane['n_valid'] and plane['passes'] >= 2
    # the coefficients are those of the un-rotated map, whatever img_rotate
    want, _, info, _ = dr.detrend_plane(res['map'], res['circle'], 2.5, 3, 2.0)
    assert (plane['a'], plane['b'], plane['g']) == (info['a'], info['b'], info['g'])
    ramp_in_the_map(res, plane)
    _, plain_cards = read_fits_f32(plain['fits'])
    assert 'DETREND' not in plain_cards and 'DTA' not in plain_cards


@pytest.mark.parametrize('flags', [['--clip', '2.5'], ['--clip-iterations', '2'], ['--detrend', 'cubic'], ['--detrend', 'plane', '--clip', '0'],
                                   ['--detrend', 'plane', '--clip-iterations', '17']])
def test_cli_flags_are_checked_by_the_parser(mods, scan_file, flags):
    doppler, _, _, _ = mods
    with pytest.raises(SystemExit) as e:
        doppler.main([scan_file] + flags)
    assert e.value.code == 2
