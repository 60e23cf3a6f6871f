"""The emission-line maps on the GPU: shg_line_emission against the NumPy restatement (tests/emission_ref.py) bit
for bit and within the exact reference's bound (tests/emission_exact.py) on the mirrored adversarial rows in every layout the
kernels branch on; the mirror check against shg_line_profile; shg_line_emission_finish against the restatement on the adversarial
finish geometries with rings; the rejected arguments; and emission_maps() and the command line on the emission scene."""
import math
import os
import shutil

import numpy as np
import pytest

from tests import emission_exact as ex
from tests import emission_ref as er
from tests import finish_adversarial as fadv
from tests import profile_adversarial as adv
from tests.linemaps_util import IH, IW, N, run_json, same_bits, same_region, scan_reader, upload, write_scan
from tests.test_emission_cpu import differing, edge_excess

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops
    return ops


LAYOUTS = [  # (name, n, ih, iw, bits, half_width, shift, rotated file, pitched, flip_x, sharded): test_profile_adversarial_gpu's
    ('rot_u16_vec', 12, 304, 48, 16, 7, 0, True, False, False, False),        # ih % 8 == 0: 16-byte loads
    ('rot_u16_odd', 12, 301, 48, 16, 7, 0, True, False, False, False),        # scalar loads
    ('rot_u8_vec', 12, 304, 48, 8, 7, 0, True, False, False, False),
    ('rot_tail', 17, 513, 40, 16, 5, 0, True, False, False, False),           # last tile one row, last phase one frame
    ('plain_u16', 131, 45, 40, 16, 7, 0, False, False, False, False),         # three blockIdx.x blocks, the last partial
    ('plain_u8', 131, 45, 40, 8, 7, 0, False, False, False, False),
    ('padded_rot', 12, 304, 48, 16, 7, 0, True, True, False, False),
    ('padded_plain', 70, 45, 40, 8, 7, 0, False, True, False, False),
    ('flip_sharded_rot', 12, 304, 48, 8, 7, 0, True, False, True, True),      # flip_x, n_cols = n + 9, k_offset = 4
    ('flip_sharded_plain', 70, 45, 40, 16, 7, 0, False, False, True, True),
    ('h1', 12, 200, 40, 16, 1, 0, True, False, False, False),
    ('h32_rot', 12, 320, 72, 16, 32, 0, True, False, False, False),
    ('s_max', 12, 304, 48, 16, 7, 48 - 4 + 7, True, False, False, False),     # the accepted extremes of S: +-(iw - 4 + H)
    ('s_min', 12, 304, 48, 8, 7, -(48 - 4 + 7), True, False, False, False),
]


@pytest.mark.parametrize('layout', LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_kernel_matches_the_restatement_and_the_exact_reference(ops, layout):
    name, n, ih, iw, bits, hw, shift, rot, pitched, flip, sharded = layout
    P, fit, _ = er.mirrored_profiles(n, ih, iw, bits, hw, shift, seed=9)
    raw = adv.to_file(P, bits, rot)
    assert raw.shape[1:] == ((iw, ih) if rot else (ih, iw)) and (raw.shape[2] > raw.shape[1]) == rot     # the kernel it picks
    stack = upload(ops, raw, bits, pitched)
    n_cols, k_offset = (n + 9, 4) if sharded else (n, 0)
    cols = k_offset + np.arange(n)
    held = n_cols - 1 - cols if flip else cols                     # frame k's column
    kw = dict(flip_x=flip, n_cols=n_cols, k_offset=k_offset)
    edge = edge_excess(ex.records(P, fit, hw, shift))
    assert edge is not None
    for min_excess in (0.0, edge):
        rec = ex.records(P, fit, hw, shift, min_excess)
        skip, _ = differing(rec, min_excess)
        got = ops.line_emission(stack, fit, hw, shift, min_excess, **kw).cpu().numpy()
        want = er.line_emission(raw, fit, hw, shift, min_excess, **kw)
        worst = {}
        for q, plane in enumerate(er.PLANES):
            same_bits(got[q], want[q])
            worst[plane] = ex.within(got[q][:, held], rec, *ex.plane(plane), skip=skip)
        assert np.isfinite(got[1]).any()
        print('%s E=%g: %d finite, largest error / bound %s' % (name, min_excess, int(np.isfinite(got[1]).sum()), worst))
    if bits == 16:
        # the mirror: first minimum and first maximum ties mirror, and the division's operands only change sign together
        from tests import linemaps_ref as ref
        mirrored = upload(ops, (65535 - raw.astype(np.int64)).astype(np.uint16), 16, pitched)
        absorb = ops.line_profile(mirrored, fit, hw, shift, **kw).cpu().numpy()[0]
        emit = ops.line_emission(stack, fit, hw, shift, 0.0, **kw).cpu().numpy()[0]
        on = np.isfinite(emit)
        assert on.any()
        same_bits(emit[on], absorb[on])
        assert ref.PLANES[0] == er.PLANES[0] == 'shift'


# ---- the finish ----
RAW_FILL, MAP_FILL, PNG_FILL = 12345.0, -777.0, 0xBEEF
MASK_RINGS = [  # on the 24 x 41 identity geometry, centre (20, 12): 3-4-5 and 6-8-10 pixels lie on the radii exactly
    (20.0, 12.0, 5.0, 10.0),                                                   # on r_in: masked; on r_out: kept
    (20.0, 12.0, math.nextafter(5.0, 0.0), math.nextafter(10.0, 0.0)),         # the same pixels just outside r_in / just outside r_out
    (20.0, 12.0, math.nextafter(5.0, 6.0), math.nextafter(10.0, 11.0)),
    (20.0, 12.0, -1.0, 10.0), (20.0, 12.0, -0.0, 10.0), (20.0, 12.0, 0.0, 0.0), (20.0, 12.0, 5.0, math.inf),
    (20.0, 12.0, -math.inf, math.inf), (19.7, 11.3, 4.45, 9.55), (20.0, 12.0, math.sqrt(41), math.sqrt(130)), None,
]


def ring_cases():
    """finish_adversarial's 5-plane cases with the circle replaced by a ring: every mask ring on the mask geometry, and for the
    other cases the circle as (cx, cy, rad / 2, rad), no inner mask, no outer edge or no ring in turn."""
    out = []
    for i, case in enumerate(fadv.cases(5)):
        c = case['circle']
        if case['name'] == 'circle_on':
            out += [dict(case, name='ring%d' % j, ring=ring) for j, ring in enumerate(MASK_RINGS)]
        elif c is not None and tuple(c) != (-1.0, -1.0, -1.0):
            ring = ((c[0], c[1], c[2] / 2, c[2]), (c[0], c[1], -1.0, c[2]), (c[0], c[1], c[2] / 2, math.inf))[i % 3]
            out.append(dict(case, ring=ring))
        else:
            out.append(dict(case, ring=None))
    return out


def kernel_finish(ops, case, png=True, **over):
    """shg_line_emission_finish on `case` in the pitched, offset buffers its layout asks for -> (status, maps, png, whether every
    element outside the outputs kept its fill)."""
    from solex_ser_recon_en_amd._lib import lib
    P = 5
    raw = case['raw']
    _, h, w = raw.shape
    lay = case['layout']
    h00, h01, h02, out_h, out_w = case['geometry']
    crop = over.get('crop', case['crop'])
    nw = int(out_w) if crop is None else max(int(crop[0]), 1)
    vr, vc = lay.get('view', (0, 0))
    rp = w + lay.get('raw_pitch', 0)
    raw_plane = (h + vr + 1) * rp + lay.get('raw_plane', 0)
    base = vr * rp + vc
    buf = np.full(P * raw_plane + base + rp * (h + 1), RAW_FILL, dtype=np.float32)
    for q in range(P):
        for y in range(h):
            buf[base + q * raw_plane + y * rp: base + q * raw_plane + y * rp + w] = raw[q, y]
    raw_d = torch.from_numpy(buf).cuda()
    mp, pp = nw + lay.get('map_pitch', 0), nw + lay.get('png_pitch', 0)
    map_plane, png_plane = out_h * mp + lay.get('map_plane', 0), out_h * pp + lay.get('png_plane', 0)
    map_d = torch.full(((P - 1) * map_plane + out_h * mp + nw,), MAP_FILL, dtype=torch.float32, device='cuda')
    png_d = torch.full(((P - 1) * png_plane + out_h * pp + nw,), PNG_FILL - 65536, dtype=torch.int16, device='cuda') if png else None
    ring = over.get('ring', case['ring'])
    r4 = None if ring is None else np.ascontiguousarray([float(v) for v in ring], dtype=np.float64)
    c4 = None if crop is None else np.ascontiguousarray([int(v) for v in crop], dtype=np.int64)
    st = lib.shg_line_emission_finish(raw_d.data_ptr() + 4 * base, raw_plane, h, w, rp, h00, h01, h02, out_h, out_w,
                                      None if r4 is None else r4.ctypes.data, None if c4 is None else c4.ctypes.data,
                                      map_d.data_ptr(), map_plane, mp, None if png_d is None else png_d.data_ptr(), png_plane, pp,
                                      over.get('half_width', case['half_width']), over.get('display_range', case['display_range']),
                                      ops._stream())
    torch.cuda.synchronize()
    m_all = map_d.cpu().numpy()
    p_all = None if png_d is None else png_d.cpu().numpy().view(np.uint16)
    if st != 0:
        return st, None, None, bool((m_all == MAP_FILL).all() and (p_all is None or (p_all == PNG_FILL).all()))
    q, r, c = np.meshgrid(np.arange(P), np.arange(out_h), np.arange(nw), indexing='ij')
    mi = (q * map_plane + r * mp + c).ravel()
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
    return st, m_all[mi].reshape(P, out_h, nw), pngs, clean


def test_finish_matches_the_restatement(ops):
    seen = set()
    for case in ring_cases():
        h00, h01, h02, out_h, out_w = case['geometry']
        want, want_png = er.line_emission_finish(case['raw'], h00, h01, h02, out_h, out_w, case['ring'], case['crop'],
                                                 case['half_width'], case['display_range'])
        st, got, got_png, clean = kernel_finish(ops, case)
        assert st == 0, (case['name'], st)
        assert clean, '%s: an element outside the output was written' % case['name']
        same_bits(got, want)
        assert np.array_equal(got_png, want_png), case['name']
        st, got2, none, clean = kernel_finish(ops, case, png=False)
        assert st == 0 and none is None and clean
        same_bits(got2, want)
        # each plane is shg_doppler_finish's with no circle wherever the ring keeps it
        plain, _ = er.line_emission_finish(case['raw'], h00, h01, h02, out_h, out_w, None, case['crop'])
        kept = ~np.isnan(got) | np.isnan(plain)
        same_bits(np.where(kept, got, 0), np.where(kept, plain, 0))
        if case['ring'] is not None and case['crop'] is None:
            keep = er.ring_keep(out_h, out_w, case['ring'])
            assert np.isnan(got[:, ~keep]).all()
            seen.add(('masks', bool((~keep).any())))
            seen.add(('inner', case['ring'][2] >= 0))
            seen.add(('outer_inf', math.isinf(case['ring'][3])))
        seen.add(('crop_pad', case['crop'] is not None and case['crop'][2] > 0))
    # the hand-checked pixels of the first three mask rings (row 12: columns 25 / 30 lie on r_in = 5 / r_out = 10)
    for j, (on_in, on_out) in enumerate(((False, True), (True, False), (False, True))):
        case = next(c for c in ring_cases() if c['name'] == 'ring%d' % j)
        raw = dict(case, raw=np.ones_like(case['raw']))
        _, got, _, _ = kernel_finish(ops, raw)
        assert bool(np.isfinite(got[0, 12, 25])) == on_in and bool(np.isfinite(got[0, 16, 23])) == on_in, j
        assert bool(np.isfinite(got[0, 12, 30])) == on_out and bool(np.isfinite(got[0, 20, 26])) == on_out, j
        assert np.isfinite(got[0, 12, 26]) and np.isnan(got[0, 12, 31]) and np.isnan(got[0, 12, 24])
    for key in (('masks', True), ('inner', True), ('inner', False), ('outer_inf', True), ('outer_inf', False), ('crop_pad', True)):
        assert key in seen, key


def test_finish_display_ties_and_clips(ops):
    # H = 3: flux e = v / 7; peak e = v; identity geometry, so every map is its raw input
    flux = [(3.5, 1), (10.5, 2), (17.5, 2), (24.5, 4), (0.0, 1), (-0.0, 1), (-7.0, 1), (7.0 * 65534.5, 65534), (7.0 * 65535.5, 65535),
            (1e9, 65535), (np.nan, 0), (70.0, 10)]
    peak = [(0.5, 1), (1.5, 2), (2.5, 2), (3.5, 4), (65534.5, 65534), (65535.5, 65535), (-3.0, 1), (1e9, 65535), (np.nan, 0), (0.0, 1),
            (-0.0, 1), (65535.0, 65535)]
    raw = np.zeros((5, 2, len(flux)), dtype=np.float32)
    raw[1], raw[4] = [p[0] for p in peak], [p[0] for p in flux]
    maps, png = ops.line_emission_finish(torch.from_numpy(raw).cuda(), 1.0, 0.0, 0.0, 2, len(flux), None, None, 3, 2.0)
    want, want_png = er.line_emission_finish(raw, 1.0, 0.0, 0.0, 2, len(flux), None, None, 3, 2.0)
    same_bits(maps.cpu().numpy(), want)
    png = png.cpu().numpy()
    assert np.array_equal(png, want_png)
    assert list(png[4, 0]) == [p[1] for p in flux] and list(png[1, 1]) == [p[1] for p in peak]
    assert (png[0] == 32768).all() and (png[2] == 1).all()


def test_rejected_arguments_write_nothing(ops):
    case = next(c for c in ring_cases() if c['name'] == 'ring0')
    bad = [('NaN cx', dict(ring=(math.nan, 12.0, 5.0, 10.0)), E_ARG), ('NaN cy', dict(ring=(20.0, math.nan, 5.0, 10.0)), E_ARG),
           ('NaN r_in', dict(ring=(20.0, 12.0, math.nan, 10.0)), E_ARG), ('NaN r_out', dict(ring=(20.0, 12.0, 5.0, math.nan)), E_ARG),
           ('r_out < 0', dict(ring=(20.0, 12.0, -2.0, -1.0)), E_ARG), ('r_out < r_in', dict(ring=(20.0, 12.0, 5.0, 4.0)), E_ARG),
           ('crop', dict(crop=(40, 30, 0, 35)), E_ARG), ('range 0', dict(display_range=0.0), E_ARG),
           ('half-width 0', dict(half_width=0), E_UNSUPPORTED), ('half-width 33', dict(half_width=33), E_UNSUPPORTED)]
    for name, over, code in bad:
        st, _, _, clean = kernel_finish(ops, case, **over)
        assert st == code, (name, st)
        assert clean, '%s: a rejected call wrote its output' % name
    # shg_line_emission: the output filled with a marker first
    from solex_ser_recon_en_amd._lib import lib
    stack = torch.zeros((2, 40, 304), dtype=torch.uint16, device='cuda')
    fit = torch.zeros((304, 4), dtype=torch.float64, device='cuda')
    fit[:, 0] = 20.0
    out = torch.full((5, 304, 64), -777.0, dtype=torch.float32, device='cuda')

    def call(hw=5, shift=0, min_excess=0.0, pitch=64, plane=304 * 64):
        return lib.shg_line_emission(stack.data_ptr(), 2, 40, 304, 2, 0, fit.data_ptr(), hw, shift, min_excess, 0, out.data_ptr(), plane,
                                     pitch, 2, 0, ops._stream())

    for name, kw, code in (('min_excess < 0', dict(min_excess=-1.0), E_ARG), ('min_excess NaN', dict(min_excess=math.nan), E_ARG),
                           ('min_excess inf', dict(min_excess=math.inf), E_ARG), ('-0.5', dict(min_excess=-0.5), E_ARG),
                           ('half-width 0', dict(hw=0), E_UNSUPPORTED), ('half-width 33', dict(hw=33), E_UNSUPPORTED),
                           ('shift', dict(shift=42), E_ARG), ('shift', dict(shift=-42), E_ARG), ('pitch', dict(pitch=1), E_ARG),
                           ('plane', dict(plane=304 * 64 - 1), E_ARG)):
        assert call(**kw) == code, name
        torch.cuda.synchronize()
        assert bool((out == -777.0).all()), '%s: a rejected call wrote its output' % name
    assert call(shift=41) == 0 and call(min_excess=0.0) == 0
    with pytest.raises(RuntimeError, match='min_excess'):
        ops.line_emission(stack, fit, 5, 0, -1.0)


# ---- emission_maps() and the command line on the emission scene ----
def restated_maps(res, raw, n_frames, ih):
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(res['phi'], res['ratio'], ih, n_frames)
    return er.line_emission_finish(raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, res['ring'], res['crop'],
                                   res['half_width'], res['display_range'])


@pytest.mark.parametrize('noise', sorted(er.TOLERANCE))
def test_maps_recover_the_injected_prominences(ops, noise):
    from solex_ser_recon_en_amd import prominence
    frames, truth = er.scene(IH, N, IW, noise)
    res = prominence.emission_maps(scan_reader(frames), min_excess=er.MIN_EXCESS)
    raw = np.stack([res['raw'][p] for p in er.PLANES])
    want = er.line_emission(frames, res['fit'], 10, 0, er.MIN_EXCESS)
    for q in range(5):
        same_bits(raw[q], want[q])
    got = er.scene_errors(raw, res['fit'], truth, 2.0 * er.MIN_EXCESS)
    finite_sky, lost, kept = er.gate_rates(raw, truth, er.MIN_EXCESS)
    print('noise %g: %s; gate %.4f / %.4f, %d kept; ring %s' % (noise, got, finite_sky, lost, kept, res['ring']))
    for name, (rms_tol, max_tol) in er.TOLERANCE[noise].items():
        rms, mx, nans = got[name]
        assert rms <= rms_tol and mx <= max_tol and nans <= er.NAN_ALLOWED[noise][name], name
    assert kept >= 200 and finite_sky <= er.GATE['finite_sky'] * 1.1 and lost <= er.GATE['lost_prominence'] * 1.1
    maps, png = restated_maps(res, raw, N, IH)
    for q, p in enumerate(er.PLANES):
        same_bits(res['maps'][p], maps[q])
        assert np.array_equal(res['png'][p], png[q]), p
    assert res['units'] == {'shift': 'pixel', 'peak': 'adu', 'width': 'pixel', 'cog': 'pixel', 'flux': 'adu'}
    # every finite pixel lies in the ring of circle_out: beyond the limb, within 1.4 radii
    cx, cy, rad = res['circle_out']
    assert res['ring_out'] == (cx, cy, rad + 0.0, rad * 1.4)
    keep = prominence.ring_mask(maps[1].shape, res['ring_out'])
    assert np.isfinite(res['maps']['peak']).sum() > 200 and not np.isfinite(res['maps']['peak'][~keep]).any()
    # --on-disk and --outer inf change only the mask
    wide = prominence.emission_maps(scan_reader(frames), min_excess=er.MIN_EXCESS, outer=math.inf, on_disk=True)
    same_bits(np.stack([wide['raw'][p] for p in er.PLANES]), raw)
    assert wide['ring'][2] == -1.0 and math.isinf(wide['ring'][3]) and wide['circle'] == res['circle']
    inside = np.isfinite(res['maps']['peak'])
    same_bits(wide['maps']['peak'][inside], res['maps']['peak'][inside])
    same_bits(wide['maps']['peak'], restated_maps(wide, raw, N, IH)[0][1])
    kms = prominence.emission_maps(scan_reader(frames), min_excess=er.MIN_EXCESS, dispersion=0.05, wavelength=6562.8)
    assert kms['units']['shift'] == kms['units']['cog'] == 'km/s' and kms['units']['width'] == 'pixel'
    same_bits(kms['maps']['shift'], (maps[0].astype(np.float64) * ((0.05 / 6562.8) * 299792.458)).astype(np.float32))


def test_library_route_8bit_unrotated(ops):
    from solex_ser_recon_en_amd import prominence
    frames, _ = er.scene(IH, N, IW, 0.004, rotate=False, bits=8)
    assert frames.dtype == np.uint8 and frames.shape[1] > frames.shape[2]
    res = prominence.emission_maps(scan_reader(frames), min_excess=1024.0, inner=2)
    raw = np.stack([res['raw'][p] for p in er.PLANES])
    want = er.line_emission(frames, res['fit'], 10, 0, 1024.0)
    maps, png = restated_maps(res, raw, N, IH)
    for q, p in enumerate(er.PLANES):
        same_bits(raw[q], want[q])
        same_bits(res['maps'][p], maps[q])
        assert np.array_equal(res['png'][p], png[q]), p
    assert np.isfinite(res['maps']['peak']).sum() > 200 and res['ring'][2] == res['circle'][2] + 2.0


def test_cli_8bit_unrotated_file(ops, tmp_path_factory, capsys):
    """The command line on the 8-bit un-rotated scene written as a SER file: the ten files, equal to the restatement on the frames
    through the library's geometry."""
    from solex_ser_recon_en_amd import prominence
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    frames, _ = er.scene(IH, N, IW, 0.004, rotate=False, bits=8)
    path = write_scan(tmp_path_factory, 'emission8', frames)
    got = run_json(prominence.main, capsys, [path, '--min-excess', '1024', '--inner', '2'])
    res = prominence.emission_maps(path, min_excess=1024.0, inner=2)
    raw = er.line_emission(frames, res['fit'], 10, 0, 1024.0)
    maps, png = restated_maps(res, raw, N, IH)
    base = os.path.splitext(path)[0]
    assert got['min_excess'] == 1024.0 and got['masked'] is True and got['ring'] == list(res['ring_out'])
    assert res['ring_out'][2] == res['circle_out'][2] + 2.0
    for q, name in enumerate(er.PLANES):
        assert got['fits'][name] == base + '_shift=0_emission_%s.fits' % name and got['png'][name] == base + '_shift=0_emission_%s.png' % name
        same_bits(res['raw'][name], raw[q])
        m, cards = read_fits_f32(got['fits'][name])
        same_bits(m, maps[q])
        assert float(cards['MINEXC']) == 1024.0 and float(cards['RINGIN']) == pytest.approx(res['ring_out'][2], rel=1e-12)
        assert np.array_equal(read_png_gray(got['png'][name]), png[q]), name
    assert np.isfinite(maps[1]).sum() > 200


def test_refusals(ops):
    from solex_ser_recon_en_amd import prominence
    frames, _ = er.scene(IH, N, IW, 0.0)
    for kw in (dict(min_excess=-1.0), dict(min_excess=math.nan), dict(outer=0.9), dict(outer=math.nan), dict(inner=math.inf),
               dict(half_width=0), dict(inner=1e6)):
        with pytest.raises(ValueError):
            prominence.emission_maps(scan_reader(frames), **kw)
    for argv in (['x.ser', '--min-excess', '-1'], ['x.ser', '--outer', '0.5'], ['x.ser', '-w', '1,2']):
        with pytest.raises(SystemExit):
            prominence.main(argv)


@pytest.fixture(scope='module')
def scan_file(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return write_scan(tmp_path_factory, 'emission', er.scene(IH, N, IW, 0.0, flat=True)[0])


def test_cli_end_to_end(ops, scan_file, capsys):
    from solex_ser_recon_en_amd import prominence
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    got = run_json(prominence.main, capsys, [scan_file, '--half-width', '8', '--min-excess', '500', '--inner', '3', '--outer', '1.3',
                                             '--range', '1.5'])
    res = prominence.emission_maps(scan_file, half_width=8, min_excess=500.0, inner=3, outer=1.3, display_range=1.5)
    base = os.path.splitext(scan_file)[0]
    assert sorted(got['fits']) == sorted(er.PLANES) and got['shift'] == 0 and got['min_excess'] == 500.0 and got['masked'] is True
    assert got['ring'] == list(res['ring_out']) and got['note'] is None
    for name in er.PLANES:
        assert got['fits'][name] == base + '_shift=0_emission_%s.fits' % name and got['png'][name] == base + '_shift=0_emission_%s.png' % name
        m, cards = read_fits_f32(got['fits'][name])
        same_bits(m, res['maps'][name])
        assert cards['HALFWID'] == '8' and cards['SHIFT'] == '0' and cards['BUNIT'].strip("' ") == res['units'][name]
        assert float(cards['MINEXC']) == 500.0 and float(cards['RINGIN']) == pytest.approx(res['ring_out'][2], rel=1e-12)
        assert float(cards['RINGOUT']) == pytest.approx(res['ring_out'][3], rel=1e-12)
        assert np.array_equal(read_png_gray(got['png'][name]), res['png'][name])
        assert got['shape'] == list(m.shape)
        stats = prominence.ring_stats(res['maps'][name], res['ring_out'])
        assert got['valid_fraction'][name] == stats['valid_fraction'] and 0 < stats['valid_fraction'] < 0.5
    assert got['median']['peak'] > 500.0 and 0 < got['median']['width'] < 17
    # without a limb fit there is no circle and no ring, and the JSON line says so
    fixed = run_json(prominence.main, capsys, [scan_file, '-x'])
    assert fixed['masked'] is False and fixed['ring'] is None and 'no ring' in fixed['note'] and fixed['circle'] == [-1, -1, -1]


# the corrected image is 423 columns wide with the limb at columns 34 and 384: -s and -r 380 crop through the prominences (-r 380
# through both), -r 500 pads
FLAGS = [('s', ['-s'], 0), ('r_narrow', ['-r', '380'], 0), ('r_wide', ['-r', '500'], 0), ('rot90', [], 90)]
OVERLAY_INNER = 7


@pytest.mark.parametrize('flags, rotate', [f[1:] for f in FLAGS], ids=[f[0] for f in FLAGS])
def test_prominences_overlay_protus(ops, scan_file, tmp_path, capsys, monkeypatch, flags, rotate):
    """The prominence patches sit on the same pixels of `_protus.png` and of the peak map, up to a one-pixel border.

    The ring starts OVERLAY_INNER = 7 px off the fitted circle: the disk's own limb saturates `_protus.png`, and on this scene the
    fitted circle lies up to 4.3 px inside the scene's limb (the ellipse of synth.scene_params through the warp), the crop moves its
    centre to int(cx) (< 1 px) and the resampling spreads the limb over one more pixel.

    The marker in `_protus.png` is the saturated pixels.  Along a row the corrected image has 1.41 pixels per frame, so successive
    pixels lie 0.71 frames apart.  A pixel that takes the weight w of a patch's edge frame and 1 - w of the sky frame beside it
    (sharp-edged patches: `flat`) saturates `_protus.png` from w = 0.37 at most (the patches hold 4800 and 5160 sample units at the line
    centre, the sky 210, and `_protus.png` saturates at 0.18 of the disk's 10 500), while the map, whose interpolation of a NaN is
    NaN, is finite from w = 1 only: the next pixel inwards has w >= 1.07, so the saturated set exceeds the finite one by at most one
    pixel, and every finite pixel is saturated.  (Half of full scale is reached from w = 0.18: two pixels.)"""
    from solex_ser_recon_en_amd import SHG_MAIN, outputs, prominence
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    defaults = SHG_MAIN.default_options
    monkeypatch.setattr(SHG_MAIN, 'default_options', lambda: dict(defaults(), img_rotate=rotate))
    dirs = {}
    for name in ('products', 'emission'):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
        shutil.copy(scan_file, dirs[name] / 'scan.ser')
    assert SHG_MAIN.main(flags + [str(dirs['products'] / 'scan.ser')]) == 0
    outputs.flush()
    got = run_json(prominence.main, capsys, [str(dirs['emission'] / 'scan.ser'), '--inner', str(OVERLAY_INNER), '--min-excess', '1500'] + flags)
    protus = read_png_gray(str(dirs['products'] / 'scan_shift=0_protus.png')).astype(np.float64)
    peak, _ = read_fits_f32(got['fits']['peak'])
    assert peak.shape == protus.shape
    ring = np.rot90(prominence.ring_mask(np.rot90(peak, -(rotate // 90)).shape, tuple(got['ring'])), rotate // 90)
    assert not np.isfinite(peak[~ring]).any()
    assert got['ring'][2] == pytest.approx(got['circle'][2] + OVERLAY_INNER, rel=1e-12)
    lit, finite = (protus == 65535) & ring, np.isfinite(peak)
    half = peak.shape[1] // 2 if rotate == 0 else peak.shape[0] // 2           # one prominence on either limb
    sides = (np.s_[:, :half], np.s_[:, half:]) if rotate == 0 else (np.s_[:half], np.s_[half:])
    print('%s rot %d: %d saturated, %d finite, by side %s' % (flags, rotate, int(lit.sum()), int(finite.sum()),
                                                              [int(finite[s].sum()) for s in sides]))
    for s in sides:
        same_region(lit[s], finite[s], 'peak vs protus')
