"""k_map_finish<1> / <5> (shg_doppler_finish, shg_line_profile_finish) against the exact reference written from the header
(tests/finish_exact.py) on the adversarial geometries of tests/finish_adversarial.py, bit for bit, in pitched and offset buffers
whose every other element must stay untouched; the rejected arguments; and the finish against the products' warp
(k_warp_rows8, and k_warp_rows with SHG_WARP_WIDE=0): on the same disk and transform both sample the same positions."""
import math
from collections import Counter

import numpy as np
import pytest

from tests import finish_adversarial as adv
from tests import finish_exact as ex

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

RAW_FILL = 12345.0                  # the raw buffer around the view: a tap read there shows up as a finite wrong value
MAP_FILL = -777.0
PNG_FILL = 0xBEEF


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops
    from solex_ser_recon_en_amd._lib import lib
    return lib, ops._stream


def _f64(v):
    return None if v is None else np.ascontiguousarray([float(q) for q in v], dtype=np.float64)


def _i64(v):
    return None if v is None else np.ascontiguousarray([int(q) for q in v], dtype=np.int64)


def _ptr(a):
    return None if a is None else a.ctypes.data


def kernel_finish(lib, case, P, png=True, **over):
    """Run the finish of P planes on `case` in the buffers its layout asks for -> (status, maps [P, out_h, nw] or None, png or
    None, whether every element outside the outputs kept its fill).  `over` replaces arguments (crop, circle, pitches, range...)."""
    lib, stream = lib
    raw = case['raw']
    _, h, w = raw.shape
    lay = case['layout']
    h00, h01, h02, out_h, out_w = case['geometry']
    crop = over.get('crop', case['crop'])
    nw = int(out_w) if crop is None else max(int(crop[0]), 1)
    vr, vc = lay.get('view', (0, 0))
    rp = over.get('raw_pitch', w + lay.get('raw_pitch', 0))
    raw_plane = over.get('raw_plane', (h + vr + 1) * rp + lay.get('raw_plane', 0))
    base = vr * rp + vc
    buf = np.full(P * max(raw_plane, h * rp) + base + rp * (h + 1), RAW_FILL, dtype=np.float32)
    for q in range(P):
        for y in range(h):
            buf[base + q * raw_plane + y * rp: base + q * raw_plane + y * rp + w] = raw[q, y]
    raw_d = torch.from_numpy(buf).cuda()
    mp = over.get('map_pitch', nw + lay.get('map_pitch', 0))
    pp = over.get('png_pitch', nw + lay.get('png_pitch', 0))
    map_plane = over.get('map_plane', out_h * mp + lay.get('map_plane', 0)) if P > 1 else 0
    png_plane = over.get('png_plane', out_h * pp + lay.get('png_plane', 0)) if P > 1 else 0
    map_n = (P - 1) * max(map_plane, 0) + out_h * max(mp, nw) + nw
    png_n = (P - 1) * max(png_plane, 0) + out_h * max(pp, nw) + nw
    map_d = torch.full((map_n,), MAP_FILL, dtype=torch.float32, device='cuda')
    png_d = torch.full((png_n,), PNG_FILL - 65536, dtype=torch.int16, device='cuda') if png else None
    c3, c4 = _f64(over.get('circle', case['circle'])), _i64(crop)
    R = over.get('display_range', case['display_range'])
    raw_ptr = raw_d.data_ptr() + 4 * base
    png_ptr = None if png_d is None else png_d.data_ptr()
    if P == 1:
        st = lib.shg_doppler_finish(raw_ptr, h, w, rp, h00, h01, h02, out_h, out_w, _ptr(c3), _ptr(c4), map_d.data_ptr(), mp,
                                    png_ptr, pp, R, stream())
    else:
        st = lib.shg_line_profile_finish(raw_ptr, raw_plane, h, w, rp, h00, h01, h02, out_h, out_w, _ptr(c3), _ptr(c4),
                                         map_d.data_ptr(), map_plane, mp, png_ptr, png_plane, pp,
                                         over.get('half_width', case['half_width'] or 0), R, stream())
    torch.cuda.synchronize()
    m_all = map_d.cpu().numpy()
    p_all = None if png_d is None else png_d.cpu().numpy().view(np.uint16)
    if st != 0:
        return st, None, None, bool((m_all == MAP_FILL).all() and (p_all is None or (p_all == PNG_FILL).all()))
    q, r, c = np.meshgrid(np.arange(P), np.arange(out_h), np.arange(nw), indexing='ij')
    mi = (q * map_plane + r * mp + c).ravel()
    maps = m_all[mi].reshape(P, out_h, nw)
    keep = np.ones(m_all.size, dtype=bool)
    keep[mi] = False
    clean = bool((m_all[keep] == MAP_FILL).all())
    pngs = None
    if p_all is not None:
        pi = (q * png_plane + r * pp + c).ravel()
        pngs = p_all[pi].reshape(P, out_h, nw)
        keep = np.ones(p_all.size, dtype=bool)
        keep[pi] = False
        clean = clean and bool((p_all[keep] == PNG_FILL).all())
    assert np.array_equal(buf.view(np.uint32), raw_d.cpu().numpy().view(np.uint32)), 'the finish wrote into its input'
    return st, maps, pngs, clean


@pytest.mark.parametrize('P', [1, 5])
def test_finish_matches_the_exact_reference(lib, P):
    total = Counter()
    for case in adv.cases(P):
        h00, h01, h02, out_h, out_w = case['geometry']
        want, want_png, cls = ex.finish(case['raw'], h00, h01, h02, out_h, out_w, case['circle'], case['crop'],
                                        case['display_range'], case['half_width'])
        total.update(cls)
        st, got, got_png, clean = kernel_finish(lib, case, P)
        assert st == 0, (case['name'], st)
        assert clean, '%s: an element outside the output was written' % case['name']
        ex.within(got, want, case['name'])
        ex.within(got_png, want_png, case['name'] + ' display')
        st, got2, none, clean = kernel_finish(lib, case, P, png=False)      # without the display planes
        assert st == 0 and none is None and clean
        ex.within(got2, want, case['name'] + ' (no png)')
    required = adv.REQUIRED + (adv.REQUIRED_PROFILE if P > 1 else ())
    missing = [k for k in required if not total.get(k)]
    print('P=%d: every class of %d matched bit for bit on the kernel: %s' % (P, len(required), sorted(total)))
    assert not missing, missing


E_ARG, E_UNSUPPORTED = -1, -3


@pytest.mark.parametrize('P', [1, 5])
def test_rejected_arguments_write_nothing(lib, P):
    case = next(c for c in adv.cases(P) if c['name'] == 'crop_lo')         # out_w = 300, crop (40, 5, 0, 35)
    out_h = case['geometry'][3]
    bad = [('lo + n > out_w', dict(crop=(40, 266, 0, 35)), E_ARG), ('dx0 + n > nw', dict(crop=(40, 0, 6, 35)), E_ARG),
           ('nw = 0', dict(crop=(0, 0, 0, 0)), E_ARG), ('lo < 0', dict(crop=(40, -1, 0, 10)), E_ARG),
           ('dx0 < 0', dict(crop=(40, 0, -1, 10)), E_ARG), ('n < 0', dict(crop=(40, 0, 0, -1)), E_ARG),
           ('map pitch', dict(map_pitch=39), E_ARG), ('png pitch', dict(png_pitch=39), E_ARG),
           ('raw pitch', dict(raw_pitch=299), E_ARG),
           ('range 0', dict(display_range=0.0), E_ARG), ('range < 0', dict(display_range=-1.0), E_ARG),
           ('range NaN', dict(display_range=math.nan), E_ARG), ('range inf', dict(display_range=math.inf), E_ARG)]
    if P > 1:
        bad += [('map plane', dict(map_plane=out_h * 40 - 1), E_ARG), ('png plane', dict(png_plane=out_h * 40 - 1), E_ARG),
                ('raw plane', dict(raw_plane=2 * 300 - 1), E_ARG),
                ('half-width 0', dict(half_width=0), E_UNSUPPORTED), ('half-width 33', dict(half_width=33), E_UNSUPPORTED)]
    for name, over, code in bad:
        st, _, _, clean = kernel_finish(lib, case, P, **over)
        assert st == code, (name, st)
        assert clean, '%s: a rejected call wrote its output' % name
    # without display planes the range and half-width are not looked at
    st, _, _, _ = kernel_finish(lib, case, P, png=False, display_range=0.0, half_width=0)
    assert st == 0


# ---- the finish samples where the products' warp samples ----
def ramp_disk(h, w):
    """uint16 [h, w]: 64 j + (7 r mod 61), injective along a row, <= 65535 for w <= 1023."""
    j = np.arange(w, dtype=np.int64)[None, :]
    r = np.arange(h, dtype=np.int64)[:, None]
    img = 64 * j + (7 * r) % 61
    assert img.max() <= 65535
    return img.astype(np.uint16)


def warp_reference_with_cval(img, h00, h01, h02, out_h, out_w):
    """Where the finish has a NaN tap, what the products' warp must hold: that tap replaced by cval = img[0, 0], the float64
    blend, clip to the image's extrema, truncation (the warp's definition, ellipse_to_circle.correct_image)."""
    h, w = img.shape
    r = np.arange(out_h, dtype=np.float64)[:, None]
    c = np.arange(out_w, dtype=np.float64)[None, :]
    x = (h00 * c + h01 * r) + h02
    x0, x1 = np.floor(x), np.ceil(x)
    t = x - x0
    rows = np.broadcast_to(np.arange(out_h)[:, None], x.shape)
    cval = float(img[0, 0])

    def tap(xi):
        inside = (xi >= 0) & (xi < w) & (rows < h)
        return np.where(inside, img[np.minimum(rows, h - 1), np.where(inside, xi, 0).astype(np.int64)], cval).astype(np.float64)

    v = (1.0 - t) * tap(x0) + t * tap(x1)
    return np.clip(v, float(img.min()), float(img.max())).astype(np.int64)


def warp_cases():
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    out = []
    for (h, w) in ((160, 300), (131, 517), (96, 1000)):
        for phi, ratio, shift in ((0.0, 1.0, 0.0), (0.12, 1.07, 0.0), (-0.3, 0.91, 0.0), (0.05, 1.2, 37.5), (0.0, 1.0, -90.25),
                                  (0.2, 0.8, 0.0)):
            _, _, mat3, out_h, out_w, _, _ = _warp_geometry(phi, ratio, h, w)
            out.append((h, w, mat3[0, 0], mat3[0, 1], mat3[0, 2] + shift, out_h, out_w))
        for h00 in (1.5, 1.75):                      # column steps up to k_warp_rows8's limit
            out.append((h, w, h00, 0.03, -3.3, h, int(w / h00) + 9))
    return out


@pytest.mark.parametrize('wide', ['1', '0'])
def test_finish_samples_where_the_warp_samples(lib, monkeypatch, wide):
    from solex_ser_recon_en_amd import ops, SHG_MAIN
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    from solex_ser_recon_en_amd.doppler import finish_circle
    monkeypatch.setenv('SHG_WARP_WIDE', wide)
    n_whole = n_nan = 0
    base = SHG_MAIN.default_options()
    for h, w, h00, h01, h02, out_h, out_w in warp_cases():
        img = ramp_disk(h, w)
        src = ops.pitched_u16(h, w, 'cuda')
        src.copy_(torch.from_numpy(img.view(np.int16)).view(torch.uint16).cuda())
        warped = ops.warp_rows_u16(src, h00, h01, h02, out_h, out_w).cpu().numpy().astype(np.int64)
        f32 = torch.from_numpy(img.astype(np.float32)).cuda()
        v, _ = ops.doppler_finish(f32, h00, h01, h02, out_h, out_w)
        v = v.cpu().numpy()
        lo, hi = int(img.min()), int(img.max())
        fin = np.isfinite(v)
        fl = np.clip(np.floor(v[fin]).astype(np.int64), lo, hi)
        whole = v[fin] == np.floor(v[fin])
        got = warped[fin]
        ok = (got == fl) | (whole & (got == fl - 1))
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, 'wide=%s %s: %d pixels sample elsewhere, first %s: warp %d, finish %r' % (
            wide, (h, w, h00, h01, h02), bad.size, np.argwhere(fin)[bad[0]], got[bad[0]], v[fin][bad[0]])
        n_whole += int((whole & (got == fl - 1)).sum())
        want = warp_reference_with_cval(img, h00, h01, h02, out_h, out_w)
        nan = ~fin
        n_nan += int(nan.sum())
        assert np.array_equal(warped[nan], want[nan]), 'wide=%s %s: where the finish has no tap the warp did not take cval' % (
            wide, (h, w, h00, h01, h02))
        # mask and crop: the products' circle and crop
        circle = (out_w / 2.0 + 0.37, out_h / 2.0 - 0.21, 0.41 * min(out_h, out_w))
        for opts in (dict(base), dict(base, crop_width_square=True), dict(base, fixed_width=out_w + 41),
                     dict(base, fixed_width=max(out_w // 2 + 1, 8))):
            crop, circle_out = crop_plan(out_h, out_w, circle, opts)
            m, _ = ops.doppler_finish(f32, h00, h01, h02, out_h, out_w, finish_circle(circle, crop, circle_out), crop)
            m = m.cpu().numpy()
            nw, lo_c, dx0, n = crop if crop is not None else (out_w, 0, 0, out_w)
            want_nan = np.ones((out_h, nw), dtype=bool)
            want_nan[:, dx0:dx0 + n] = nan[:, lo_c:lo_c + n]
            cx, cy, rad = circle_out
            rr = np.arange(out_h, dtype=np.float64)[:, None]
            cc = np.arange(nw, dtype=np.float64)[None, :]
            want_nan |= (cc - cx) * (cc - cx) + (rr - cy) * (rr - cy) > rad * rad
            assert np.array_equal(np.isnan(m), want_nan), 'wide=%s crop %s: the NaN pattern is not the products\' circle %s' % (
                wide, crop, circle_out)
            held = ~want_nan
            src_cols = (np.arange(nw) - dx0 + lo_c)[None, :].repeat(out_h, 0)
            assert np.array_equal(m[held], v[np.nonzero(held)[0], src_cols[held]])
    print('SHG_WARP_WIDE=%s: %d cases; %d pixels one below a whole float32 value; %d pixels without a tap (cval)' % (
        wide, len(warp_cases()), n_whole, n_nan))
    assert n_nan > 0
