"""The line-bisector maps without a GPU: the NumPy restatement (tests/linemaps_ref.py) against the exact reference
(tests/linemaps_exact.py) on seeded adversarial profiles, its f = 0.5 chord against the line-profile width, symmetric lines, its
accuracy on the two synthetic scans (the tolerance the GPU tests hold line_bisector_maps() to), the display planes, and the
library's and the CLI's argument errors."""
import math

import numpy as np
import pytest

from tests import linemaps_exact as ex
from tests import linemaps_ref as ref
from tests import profile_adversarial as adv
from tests.linemaps_util import fit_at, one_row_scan

LAYOUTS = [  # (name, n, ih, iw, bits, half_width, shift, rotated file)
    ('rot_u16', 12, 304, 48, 16, 7, 0, True),
    ('plain_u8', 40, 45, 40, 8, 5, 0, False),
    ('h32', 6, 320, 72, 16, 32, 0, True),
    ('s_mid', 12, 301, 48, 16, 5, -13, True),
]


def check(name, n, ih, iw, bits, hw, shift, rot, levels):
    P, fit, cls = adv.level_profiles(n, ih, iw, bits, hw, levels, shift, seed=5)
    raw = adv.to_file(P, bits, rot)
    recs = ex.records(P, fit, hw, shift, levels)
    mism, n_dec = set(), 0
    for y, row in enumerate(recs):
        for k, r in enumerate(row or ()):
            for exact, f64, thr, _ in ex.level_decisions(r):
                n_dec += 1
                assert f64 == thr                      # p >= level <=> p >= ceil(level) for integer p
                if exact != f64:
                    mism.add((y, k))
    planes = ref.line_bisector(raw, fit, hw, levels, shift)
    kk = len(levels)
    worst = max([ex.within(planes[i], recs, *ex.level(i, 'bis'), mism) for i in range(kk)] +
                [ex.within(planes[kk + i], recs, *ex.level(i, 'chord'), mism) for i in range(kk)])
    assert np.isfinite(planes).any() and np.isnan(planes).any()
    return len(mism), n_dec, worst, cls


@pytest.mark.parametrize('levels', adv.LEVEL_SETS, ids=['K%d' % len(s) for s in adv.LEVEL_SETS])
@pytest.mark.parametrize('layout', LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_restatement_agrees_with_the_exact_reference(layout, levels):
    """NaN where the exact value is NaN, within linemaps_exact's bounds elsewhere.  Cases whose float64 level decides otherwise
    than the exact level (b < level, or p >= level for some sample) are counted and left out: non-dyadic fractions round in 1 - f
    and in the products, and the adversarial rows put samples at ceil(level) and ceil(level) - 1 on purpose.  Dyadic levels
    (0.25, 0.5, 0.75) must have none; the others hold the count under 2 % of the decisions (measured: 0.3 to 1.1 %)."""
    n_mism, n_dec, worst, cls = check(*layout, levels)
    print('%s K=%d: %d decisions, %d cases decided otherwise by the float64 level, largest error / bound %.3f'
          % (layout[0], len(levels), n_dec, n_mism, worst))
    if all(f in (0.25, 0.5, 0.75) for f in levels):
        assert n_mism == 0
    assert n_mism <= 0.02 * n_dec
    if layout[5] >= 5:
        assert all(cls.count(kind) for kind in adv.LEVEL_KINDS), 'level classes missing'


def test_integral_levels_and_hits_are_reached():
    """The adversarial rows reach: a sample at ceil(level) and at ceil(level) - 1, an integral level, p(j*) = level, crossings on
    the window's edges, an unbracketed minimum, C2 = 0 and C2 / 2 <= core."""
    levels = (0.25, 0.5, 0.75)
    P, fit, _ = adv.level_profiles(12, 304, 48, 16, 7, levels, 0, seed=5)
    seen = dict.fromkeys(('ceil', 'ceil_minus1', 'integral', 'best_eq', 'edge_lo', 'edge_hi', 'unbracketed', 'c2_zero',
                          'continuum_below_core'), 0)
    for row in ex.records(P, fit, 7, 0, levels):
        for v in row or ():
            # (C2 / 2 at or below the core leaves no vertex: p(lo) > b for a first minimum inside forces p(hi) < b)
            seen['c2_zero'] += v['C2'] == 0
            seen['continuum_below_core'] += v['C2'] <= 2 * min(v['p'][v['lo']:v['hi'] + 1])
            if v['core'] is None:
                seen['unbracketed'] += 1
                continue
            for L in v['levels']:
                lv = L['level']
                seen['integral'] += lv.denominator == 1
                seen['best_eq'] += v['b'] == lv
                c = math.ceil(lv)
                win = v['p'][v['lo'] + 1:v['hi']]
                seen['ceil'] += c in win
                seen['ceil_minus1'] += (c - 1) in win
                seen['edge_lo'] += L['jl'] == v['lo']
                seen['edge_hi'] += L['jr'] == v['hi']
    print(seen)
    assert all(seen.values()), seen


def test_chord_at_half_is_the_profile_width():
    from solex_ser_recon_en_amd import synth
    frames = synth.synth_frames_numpy(9, 160, 30, 16, seed=3, tilt=0.01, curv=2e-5)
    centre = synth.curve_of_row(np.arange(160, dtype=np.float64), 160, 30) + np.random.default_rng(1).uniform(-3, 3, 160)
    fit = fit_at(centre)
    for hw, s in ((1, 0), (5, 0), (12, 2)):
        got = ref.line_bisector(frames, fit, hw, (0.3, 0.5), s)[3]
        want = ref.line_profile(frames, fit, hw, s)[2]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.isfinite(got).any()
        # a level's planes do not depend on the others requested
        alone = ref.line_bisector(frames, fit, hw, (0.3,), s)
        same = ref.line_bisector(frames, fit, hw, (0.3, 0.5), s)
        assert np.array_equal(alone[0].view(np.uint32), same[0].view(np.uint32))
        assert np.array_equal(alone[1].view(np.uint32), same[2].view(np.uint32))


def test_symmetric_lines_give_the_shift_at_every_level():
    # a symmetric triangle of slope 400 with its tip at 20.25 (an exact V in the samples: p = 400 |j - 20.25| at integers stays
    # symmetric about 20.25 only through the crossings), flat at 4000 beyond: every level's crossings are mirror images
    j = np.arange(40)
    p = np.minimum(400 * np.abs(2 * j - 41), 8000)            # tip at 20.5, symmetric about it
    for fit0 in (20.5, 19.5, 21.25):
        got = ref.line_bisector(one_row_scan(p[None, None, :].astype(np.uint16)), fit_at([fit0], 41), 12, (0.1, 0.3, 0.5, 0.7, 0.9))
        assert np.all(got[:5, 0, 0] == np.float32(20.5 - fit0)), got[:5, 0, 0]


@pytest.mark.parametrize('noise', sorted(ref.TOLERANCE['bisector']))
@pytest.mark.parametrize('kind', ('symmetric', 'asymmetric'))
def test_restatement_recovers_the_bisectors(kind, noise):
    ih, n, iw = 400, 300, 48
    frames, centre, on, truth = ref.bisector_scan(kind, ih, n, iw, noise)
    rms_tol, max_tol = ref.TOLERANCE['bisector'][noise][kind]
    kk = len(ref.LEVELS)
    for d in ref.FIT_OFFSETS:
        fit = fit_at(centre + d)
        got = ref.bisector_errors(ref.line_bisector(frames, fit, 10, ref.LEVELS)[:kk], truth(fit, 10, ref.LEVELS), on)
        print('%s noise %g, fit %+g px: %s' % (kind, noise, d, got))
        for i, (rms, mx, nans) in got.items():
            assert nans == 0 and rms <= rms_tol and mx <= max_tol, (ref.LEVELS[i], rms, mx, nans)


def test_asymmetric_line_has_a_c_shaped_bisector():
    # the broad component lies 1.2 px to the red of the narrow one: the bisector moves redward from the core to the continuum
    frames, centre, on, truth = ref.bisector_scan('asymmetric', 200, 150, 48, 0.0)
    fit = fit_at(centre)
    b = ref.line_bisector(frames, fit, 10, (0.2, 0.5, 0.8))[:3]
    med = [float(np.median(b[i][on])) for i in range(3)]
    assert med[0] < med[1] < med[2], med


def test_display_planes():
    v = np.array([np.nan, -3.0, 0.0, 0.4, 1e9], dtype=np.float32)
    assert ref.display(v, 'bisector', 5, 2.0).tolist() == [0, 1, 32768, int(np.rint(32768 + np.float64(np.float32(0.4)) * 32767 / 2)),
                                                           65535]
    assert ref.display(v, 'chord', 5, 2.0).tolist() == [0, 1, 1, int(np.rint(1 + np.float64(np.float32(0.4)) * 65534 / 11)), 65535]
    raw = np.stack([np.arange(12, dtype=np.float32).reshape(3, 4) - 5 + q for q in range(4)]) / 4
    maps, png = ref.line_bisector_finish(raw, 1.0, 0.0, 0.0, 3, 4, half_width=5, display_range=2.0)
    assert np.array_equal(maps, raw)
    for q in range(4):
        assert np.array_equal(png[q], ref.display(maps[q], 'shift' if q < 2 else 'width', 5, 2.0))


# ---- the library's and the CLI's argument errors (no GPU: they are refused before the scan is read) ----
@pytest.fixture
def bisector():
    from solex_ser_recon_en_amd import bisector
    return bisector


BAD_LEVELS = [((), 'between 1 and 8'), (tuple(0.1 * i for i in range(1, 10)), 'between 1 and 8'), ((0.4, 0.2), 'increasing'),
              ((0.3, 0.3), 'increasing'), ((0.0, 0.5), 'strictly between'), ((0.5, 1.0), 'strictly between'),
              ((math.nan,), 'strictly between'), ((math.inf,), 'strictly between'), (('a',), 'numbers')]


@pytest.mark.parametrize('levels, message', BAD_LEVELS)
def test_library_refuses_bad_levels(bisector, levels, message):
    with pytest.raises(ValueError, match=message):
        bisector.line_bisector_maps('missing_scan.ser', levels=levels)


def test_library_argument_errors(bisector):
    with pytest.raises(ValueError, match='half_width'):
        bisector.line_bisector_maps('scan.ser', half_width=40)
    with pytest.raises(ValueError, match='both'):
        bisector.line_bisector_maps('scan.ser', dispersion=0.05)
    with pytest.raises(ValueError, match='positive'):
        bisector.line_bisector_maps('scan.ser', display_range=0.0)
    assert bisector.check_levels([0.2, '0.4']) == (0.2, 0.4)
    assert [bisector.level_tag(f) for f in (0.2, 0.35, 0.125, 0.5, 1e-6)] == ['20', '35', '12.5', '50', '0.0001']


@pytest.mark.parametrize('argv, message', [
    (['scan.ser', '--levels', ''], '--levels'),
    (['scan.ser', '--levels', ','.join(['0.1', '0.2', '0.3', '0.4', '0.5', '0.6', '0.7', '0.8', '0.9'])], '--levels'),
    (['scan.ser', '--levels', '0.6,0.4'], 'increasing'),
    (['scan.ser', '--levels', '0,0.5'], 'strictly between'),
    (['scan.ser', '--levels', '0.5,1'], 'strictly between'),
    (['scan.ser', '--levels', 'nan'], 'strictly between'),
    (['scan.ser', '--levels', '0.2,x'], 'numbers'),
    (['scan.ser', '--half-width', '0'], '--half-width'),
    (['scan.ser', '--line', '5875.6'], '--line needs --atlas'),
    (['scan.ser', '--line', '5875.6', '--shift', '3', '--atlas', 'a.npz', '--anchor', '6562.8'], 'exclude'),
    (['scan.ser', '--dispersion', '0.05'], '--dispersion and --wavelength'),
    (['scan.ser', '--range', '0'], '--range'),
    (['scan.ser', '-w', '3'], '-w'),
    (['a.ser', 'b.ser'], 'exactly one'),
    (['missing_scan.ser'], 'no such file'),
])
def test_cli_argument_errors(bisector, capsys, argv, message):
    with pytest.raises(SystemExit) as e:
        bisector.main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_cli_refuses_torchrun(bisector, capsys, monkeypatch):
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        bisector.main(['scan.ser'])
    assert e.value.code == 2 and 'single-process' in capsys.readouterr().err
