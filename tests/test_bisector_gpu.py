"""The line-bisector maps on the GPU: shg_line_bisector and shg_line_bisector_finish bit for bit against the NumPy restatement
(tests/linemaps_ref.py), against the line-profile kernels where they overlap, and against the exact reference (tests/linemaps_exact.py)
on adversarial rows; refused arguments writing nothing; line_bisector_maps() recovering the bisectors of both synthetic scans within
what the restatement achieves (linemaps_ref.TOLERANCE['bisector']); the CLI end to end, its maps overlaying the products."""
import os
import shutil

import numpy as np
import pytest

from tests import linemaps_exact as ex
from tests import linemaps_ref as ref
from tests import profile_adversarial as adv
from tests.linemaps_util import (IH, IW, N, SHIFT, SHIFT_CASES, finish_cases, fit_for, marked_scan, run_json, same_bits, same_region,
                                 scan_reader, upload, write_scan)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

LEVELS = {1: (0.5,), 3: (0.25, 0.5, 0.8), 8: (0.05, 0.15, 0.3, 0.45, 0.5, 0.7, 0.85, 0.95)}


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import bisector, ops, synth
    return bisector, ops, synth


@pytest.mark.parametrize('k', sorted(LEVELS))
@pytest.mark.parametrize('case', SHIFT_CASES, ids=['%s_s%d' % (c[0], c[-1]) for c in SHIFT_CASES])
def test_line_bisector_bit_exact(mods, case, k):
    _, ops, synth = mods
    name, n, width, height, bits, hw, flip, sharded, pitched, shift = case
    frames = synth.synth_frames_numpy(n, width, height, bits, seed=11, tilt=0.01, curv=2e-5)
    ih, iw = max(width, height), min(width, height)
    fit = fit_for(synth, ih, iw, seed=len(name))
    stack = upload(ops, frames, bits, pitched)
    n_cols, k_offset = (n + 9, 4) if sharded else (n, 0)
    levels = LEVELS[k]
    got = ops.line_bisector(stack, fit, hw, levels, shift, flip_x=flip, n_cols=n_cols, k_offset=k_offset).cpu().numpy()
    want = ref.line_bisector(frames, fit, hw, levels, shift, flip_x=flip, n_cols=n_cols, k_offset=k_offset)
    assert got.shape == want.shape == (2 * k, ih, n_cols)
    for q in range(2 * k):
        same_bits(got[q], want[q])
    assert np.isfinite(want[:, :, k_offset:k_offset + n]).any()
    if 0.5 in levels:
        i = levels.index(0.5)
        prof = ops.line_profile(stack, fit, hw, shift, flip_x=flip, n_cols=n_cols, k_offset=k_offset).cpu().numpy()
        same_bits(got[k + i], prof[2])


def test_a_level_does_not_depend_on_the_others(mods):
    _, ops, synth = mods
    for width, height, bits in ((600, 80, 16), (80, 600, 8)):
        frames = synth.synth_frames_numpy(20, width, height, bits, seed=5, tilt=0.01, curv=2e-5)
        ih, iw = max(width, height), min(width, height)
        fit = fit_for(synth, ih, iw, seed=3)
        stack = upload(ops, frames, bits)
        many = ops.line_bisector(stack, fit, 12, LEVELS[8]).cpu().numpy()
        for i, f in enumerate(LEVELS[8]):
            alone = ops.line_bisector(stack, fit, 12, (f,)).cpu().numpy()
            same_bits(alone[0], many[i])
            same_bits(alone[1], many[8 + i])


def test_line_bisector_c2_size(mods):
    _, ops, synth = mods
    stack = synth.synth_frames_torch(2000, 2000, 200, 16, seed=2, padded=True)
    frames = ops.stack_to_host(stack)
    fit = fit_for(synth, 2000, 200, seed=5, jitter=1.0, edges=False, nans=False)
    levels = (0.2, 0.4, 0.6, 0.8)
    got = ops.line_bisector(stack, fit, 12, levels).cpu().numpy()
    want = ref.line_bisector(frames, fit, 12, levels)
    for q in range(8):
        same_bits(got[q], want[q])
    assert np.isfinite(got).mean() > 0.9


ADV_LAYOUTS = [  # (name, n, ih, iw, bits, half_width, shift, rotated file)
    ('rot_u16', 12, 304, 48, 16, 7, 0, True),
    ('rot_u8', 12, 301, 48, 8, 7, 0, True),
    ('plain_u16', 70, 45, 40, 16, 7, 0, False),
    ('plain_u8', 40, 45, 40, 8, 5, 0, False),
    ('h32', 6, 320, 72, 16, 32, 0, True),
    ('s_mid', 12, 301, 48, 16, 5, -13, True),
]


@pytest.mark.parametrize('levels', adv.LEVEL_SETS, ids=['K%d' % len(s) for s in adv.LEVEL_SETS])
@pytest.mark.parametrize('layout', ADV_LAYOUTS, ids=[c[0] for c in ADV_LAYOUTS])
def test_adversarial_rows_against_the_exact_reference(mods, layout, levels):
    _, ops, _ = mods
    name, n, ih, iw, bits, hw, shift, rot = layout
    P, fit, _ = adv.level_profiles(n, ih, iw, bits, hw, levels, shift, seed=5)
    raw = adv.to_file(P, bits, rot)
    got = ops.line_bisector(upload(ops, raw, bits), fit, hw, levels, shift).cpu().numpy()
    same_bits(got, ref.line_bisector(raw, fit, hw, levels, shift))
    recs = ex.records(P, fit, hw, shift, levels)
    skip = {(y, k) for y, row in enumerate(recs) for k, r in enumerate(row or ())
            if any(exact != f64 for exact, f64, _, _ in ex.level_decisions(r))}
    kk = len(levels)
    for i in range(kk):
        ex.within(got[i], recs, *ex.level(i, 'bis'), skip)
        ex.within(got[kk + i], recs, *ex.level(i, 'chord'), skip)


def test_refused_arguments_write_nothing(mods):
    _, ops, _ = mods
    stack = torch.zeros((4, 40, 300), dtype=torch.uint16, device='cuda')
    fit = np.zeros((300, 4))
    fit[:, 0] = fit[:, 3] = 20.0
    bad = [((0.4, 0.2), 5, 0), ((0.0, 0.5), 5, 0), ((0.5, 1.0), 5, 0), ((float('nan'),), 5, 0), ((0.3, 0.3), 5, 0),
           (tuple(0.1 * i for i in range(1, 10)), 5, 0), ((0.5,), 5, 42), ((0.5,), 5, -42), ((0.5,), 33, 0), ((0.5,), 0, 0)]
    for levels, hw, s in bad:
        out = torch.full((2 * len(levels), 300, 4), 1234.5, dtype=torch.float32, device='cuda')
        with pytest.raises(RuntimeError):
            ops.line_bisector(stack, fit, hw, levels, s, out=out)
        torch.cuda.synchronize()
        assert bool((out == 1234.5).all()), (levels, hw, s)
    with pytest.raises(RuntimeError):
        ops.line_bisector(stack, fit, 5, ())
    raw = torch.zeros((4, 30, 40), dtype=torch.float32, device='cuda')
    maps = ops.line_bisector_finish(raw, 1.0, 0.0, 0.0, 30, 40, None, None, 5, 2.0)[0]
    assert maps.shape == (4, 30, 40)
    with pytest.raises(RuntimeError, match='half-width'):
        ops.line_bisector_finish(raw, 1.0, 0.0, 0.0, 30, 40, None, None, 40, 2.0)
    with pytest.raises(RuntimeError, match='levels'):
        ops.line_bisector_finish(torch.zeros((18, 30, 40), dtype=torch.float32, device='cuda'), 1.0, 0.0, 0.0, 30, 40)


@pytest.mark.parametrize('phi, ratio, shift', [(0.0, 1.0, 0.0), (0.12, 1.07, 0.0), (0.05, 1.2, 37.5)])
def test_finish_matches_doppler_finish_and_the_restatement(mods, phi, ratio, shift):
    _, ops, _ = mods
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    from solex_ser_recon_en_amd.Solex_recon import crop_plan
    rng = np.random.default_rng(3)
    h, w = 300, 400
    for k in (1, 3, 8):
        raw = np.concatenate([rng.normal(0.0, 1.5, (k, h, w)), rng.uniform(-1, 30, (k, h, w))]).astype(np.float32)
        raw[rng.random(raw.shape) < 0.05] = np.nan
        _, _, mat3, out_h, out_w, _, _ = _warp_geometry(phi, ratio, h, w)
        h00, h01, h02 = mat3[0, 0], mat3[0, 1], mat3[0, 2] + shift
        rt = torch.empty((2 * k, h, w + 12), dtype=torch.float32, device='cuda')[:, :, :w]
        rt.copy_(torch.from_numpy(raw))
        for name, circle, opts in finish_cases()[::2]:
            crop, _ = crop_plan(out_h, out_w, circle if circle is not None else (-1, -1, -1), opts)
            maps, png = ops.line_bisector_finish(rt, h00, h01, h02, out_h, out_w, circle, crop, 6, 1.7)
            want, want_png = ref.line_bisector_finish(raw, h00, h01, h02, out_h, out_w, circle, crop, 6, 1.7)
            maps, png = maps.cpu().numpy(), png.cpu().numpy()
            for q in range(2 * k):
                one, _ = ops.doppler_finish(rt[q], h00, h01, h02, out_h, out_w, circle, crop)
                same_bits(maps[q], one.cpu().numpy())
                same_bits(maps[q], want[q])
            assert np.array_equal(png, want_png), (k, name)
            maps2, none = ops.line_bisector_finish(rt, h00, h01, h02, out_h, out_w, circle, crop)
            assert none is None
            same_bits(maps2.cpu().numpy(), want)


# ---- line_bisector_maps() on the synthetic scans ----
@pytest.mark.parametrize('noise', sorted(ref.TOLERANCE['bisector']))
@pytest.mark.parametrize('kind', ('symmetric', 'asymmetric'))
def test_maps_recover_the_bisectors(mods, kind, noise):
    bisector, _, _ = mods
    frames, centre, on, truth = ref.bisector_scan(kind, IH, N, IW, noise)
    levels = ref.LEVELS
    res = bisector.line_bisector_maps(scan_reader(frames), levels=levels)
    kk = len(levels)
    raw = np.stack([res['raw']['bisector', f] for f in levels] + [res['raw']['chord', f] for f in levels])
    same_bits(raw, ref.line_bisector(frames, res['fit'], 10, levels))
    got = ref.bisector_errors(raw[:kk], truth(res['fit'], 10, levels), on)
    print('%s noise %g: %s' % (kind, noise, got))
    rms_tol, max_tol = ref.TOLERANCE['bisector'][noise][kind]
    for i, (rms, mx, nans) in got.items():
        assert nans == 0 and rms <= rms_tol and mx <= max_tol, (levels[i], rms, mx)
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(res['phi'], res['ratio'], IH, N)
    maps, png = ref.line_bisector_finish(raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, res['circle'], None, 10, 2.0)
    keys = [('bisector', f) for f in levels] + [('chord', f) for f in levels]
    for q, key in enumerate(keys):
        same_bits(res['maps'][key], maps[q])
        assert np.array_equal(res['png'][key], png[q]), key
        assert res['units'][key] == 'pixel'
    kms = bisector.line_bisector_maps(scan_reader(frames), levels=levels, dispersion=0.05, wavelength=6562.8)
    assert kms['units']['bisector', 0.5] == 'km/s' and kms['units']['chord', 0.5] == 'pixel'
    same_bits(kms['maps']['bisector', 0.5], (maps[2].astype(np.float64) * ((0.05 / 6562.8) * 299792.458)).astype(np.float32))
    same_bits(kms['maps']['chord', 0.5], maps[kk + 2])


# ---- the command line, and the overlay on the products ----
@pytest.fixture(scope='module')
def scan_file(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return write_scan(tmp_path_factory, 'bisector', ref.bisector_scan('asymmetric', IH, N, IW, noise=0.004, seed=4)[0])


def test_cli_end_to_end(mods, scan_file, capsys):
    bisector, _, _ = mods
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    levels = (0.25, 0.5, 0.875)
    got = run_json(bisector.main, capsys, [scan_file, '--half-width', '8', '--shift', '1', '--levels', '0.25,0.5,0.875', '--widths',
                                           '--range', '1.5'])
    res = bisector.line_bisector_maps(scan_file, half_width=8, shift=1, levels=levels, display_range=1.5)
    assert got['levels'] == list(levels) and got['shift'] == 1
    base = os.path.splitext(scan_file)[0]
    names = []
    for f, tag in zip(levels, ('25', '50', '87.5')):
        for kind, suffix in (('bisector', ''), ('chord', '_chord')):
            name = 'bisector_%s%s' % (tag, suffix)
            names.append(name)
            assert got['fits'][name] == base + '_shift=1_%s.fits' % name and got['png'][name] == base + '_shift=1_%s.png' % name
            m, cards = read_fits_f32(got['fits'][name])
            same_bits(m, res['maps'][kind, f])
            assert float(cards['LEVEL']) == f and cards['SHIFT'] == '1' and cards['HALFWID'] == '8'
            assert np.array_equal(read_png_gray(got['png'][name]), res['png'][kind, f])
            assert got['valid_fraction'][name] > 0.9
    assert sorted(got['fits']) == sorted(names)
    plain = run_json(bisector.main, capsys, [scan_file])
    assert sorted(plain['fits']) == ['bisector_20', 'bisector_40', 'bisector_60', 'bisector_80']
    # the C shape: the broad component lies to the red of the narrow one
    assert plain['median']['bisector_20'] < plain['median']['bisector_80']


FLAGS = [('m', ['-m'], 0), ('s', ['-s'], 0), ('r', ['-r', '300'], 0), ('x', ['-x'], 0), ('rot90', [], 90), ('m_s_rot270', ['-m', '-s'], 270)]


@pytest.mark.parametrize('flags, rotate', [f[1:] for f in FLAGS], ids=[f[0] for f in FLAGS])
def test_bisector_maps_overlay_the_line_cog(mods, tmp_path, capsys, monkeypatch, flags, rotate):
    """The overlay tests' marked scan (a bright patch 2 px to the red): the patch lies on the same pixels of _bisector_50.fits and
    _line_cog.fits, and the maps have the products' shape."""
    bisector, _, synth = mods
    from solex_ser_recon_en_amd import SHG_MAIN, lineprofile, outputs
    from solex_ser_recon_en_amd.fits_io import read_fits_f32
    from solex_ser_recon_en_amd.png_io import read_png_gray
    defaults = SHG_MAIN.default_options
    monkeypatch.setattr(SHG_MAIN, 'default_options', lambda: dict(defaults(), img_rotate=rotate))
    src = tmp_path / 'marked.ser'
    synth.write_ser(str(src), marked_scan())
    dirs = {}
    for name in ('products', 'profile', 'bisector'):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
        shutil.copy(src, dirs[name] / 'scan.ser')
    assert SHG_MAIN.main(['-t'] + flags + [str(dirs['products'] / 'scan.ser')]) == 0
    outputs.flush()
    prof = run_json(lineprofile.main, capsys, [str(dirs['profile'] / 'scan.ser')] + flags)
    bis = run_json(bisector.main, capsys, [str(dirs['bisector'] / 'scan.ser'), '--levels', '0.3,0.5', '--widths'] + flags)
    cog, _ = read_fits_f32(prof['fits']['cog'])
    b50, _ = read_fits_f32(bis['fits']['bisector_50'])
    chord, _ = read_fits_f32(bis['fits']['bisector_50_chord'])
    width, _ = read_fits_f32(prof['fits']['width'])
    clahe = read_png_gray(str(dirs['products'] / 'scan_shift=0_clahe.png'))
    assert b50.shape == cog.shape == clahe.shape and bis['shape'] == list(clahe.shape)
    with np.errstate(invalid='ignore'):
        same_region(cog > SHIFT / 2, b50 > SHIFT / 2, 'bisector 50 vs line cog')
    same_bits(chord, width)                            # the f = 0.5 chord is the profile's width, through the same geometry
    assert bis['circle'] == prof['circle'] and bis['crop'] == prof['crop']
