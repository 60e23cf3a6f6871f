"""The emission-line maps without a GPU: the NumPy restatement (tests/emission_ref.py) against the exact reference
(tests/emission_exact.py) on the mirrored adversarial rows, the argument rules, and the accuracy and gate rates the restatement
reaches on the emission scene (emission_ref.TOLERANCE, emission_ref.GATE)."""
from fractions import Fraction

import numpy as np
import pytest

from tests import emission_exact as ex
from tests import emission_ref as er
from tests import linemaps_ref as ref
from tests import profile_adversarial as adv
from tests.linemaps_util import IH, IW, N, fit_at, same_bits

SETS = [('u16', 12, 120, 48, 16, 7, 0), ('u8', 12, 120, 48, 8, 7, 0), ('h1', 8, 60, 40, 16, 1, 0), ('h32', 6, 90, 72, 16, 32, 0),
        ('s_max', 8, 120, 48, 16, 7, 48 - 4 + 7), ('s_min', 8, 120, 48, 8, 7, -(48 - 4 + 7))]


def differing(records, min_excess):
    """(the (y, k) whose float64 gate or half-level decisions differ from the exact ones, the number of decisions compared)."""
    skip, count = set(), 0
    for y, row in enumerate(records):
        for k, r in enumerate(row or ()):
            if r['bracket']:
                exact, f64 = ex.decisions64(r, min_excess)
                count += len(exact)
                if exact != f64:
                    skip.add((y, k))
    return skip, count


def edge_excess(records):
    """A positive excess_d of the set that float64 holds exactly (min_excess set to it sits exactly on that row's excess), or None."""
    for row in records:
        for r in row or ():
            if r['bracket'] and r['excess'] > 0:
                e64 = (float(r['b']) - float(r['d'] * r['d']) / (8.0 * float(r['den']))) - 0.5 * float(r['B2'])
                if Fraction(e64) == r['excess']:
                    return e64
    return None


@pytest.mark.parametrize('case', SETS, ids=[c[0] for c in SETS])
def test_restatement_matches_the_exact_reference(case):
    name, n, ih, iw, bits, hw, shift = case
    P, fit, _ = er.mirrored_profiles(n, ih, iw, bits, hw, shift, seed=9)
    raw = adv.to_file(P, bits, True)
    edge = edge_excess(ex.records(P, fit, hw, shift))
    assert edge is not None, 'no row whose excess float64 holds exactly'
    for min_excess in (0.0, edge):
        rec = ex.records(P, fit, hw, shift, min_excess)
        skip, count = differing(rec, min_excess)
        got = er.line_emission(raw, fit, hw, shift, min_excess)
        worst = {p: ex.within(got[q], rec, *ex.plane(p), skip=skip) for q, p in enumerate(er.PLANES)}
        on_edge = sum(r['bracket'] and r['excess'] == Fraction(min_excess) for row in rec for r in row or ())
        finite = int(np.isfinite(got[1]).sum())
        print('%s E=%g: %d decisions, %d rows differ in float64, %d on the gate, %d finite; error / bound %s'
              % (name, min_excess, count, len(skip), on_edge, finite, worst))
        assert len(skip) <= 0.01 * max(count, 1) and finite > 0
        if min_excess > 0:
            assert on_edge >= 1                                  # the >= is exercised: that row is kept
            assert finite < int(np.isfinite(er.line_emission(raw, fit, hw, shift, 0.0)[1]).sum())
        for p in ('width', 'cog', 'flux'):
            assert np.isfinite(got[er.PLANES.index(p)]).any(), p


def test_plain_and_rotated_files_agree():
    P, fit, _ = er.mirrored_profiles(6, 60, 40, 8, 5, 0, seed=2)
    a = er.line_emission(adv.to_file(P, 8, True), fit, 5)
    b = er.line_emission(adv.to_file(P, 8, False), fit, 5, flip_x=True, n_cols=9, k_offset=2)
    same_bits(a, b[:, :, ::-1][:, :, 2:8])


def test_a_gated_pixel_is_nan_in_every_plane():
    P, fit, _ = er.mirrored_profiles(12, 120, 48, 16, 7, 0, seed=9)
    got = er.line_emission(adv.to_file(P, 16, True), fit, 7, 0, 2000.0)
    gated = np.isnan(got[0])
    assert gated.any() and not gated.all()
    for q in range(1, 5):
        assert np.isnan(got[q][gated]).all()
    assert (got[1][~gated] >= 2000.0).all()


def test_argument_rules():
    frames = np.zeros((2, 40, 60), dtype=np.uint16)
    fit = fit_at(np.full(60, 20.0))
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            er.line_emission(frames, fit, 5, 0, bad)
    er.line_emission(frames, fit, 5, 0, 0.0)
    raw = np.zeros((5, 4, 6), dtype=np.float32)
    for bad in ((np.nan, 0, 1, 2), (0, np.nan, 1, 2), (0, 0, np.nan, 2), (0, 0, 1, np.nan), (0, 0, -1, -0.5), (0, 0, 3, 2)):
        with pytest.raises(ValueError):
            er.line_emission_finish(raw, 1.0, 0.0, 0.0, 4, 6, bad)
    for good in ((0, 0, -1, 0), (0, 0, 2, 2), (0, 0, -5, np.inf), (np.inf, 0, 1, 2), None):
        er.line_emission_finish(raw, 1.0, 0.0, 0.0, 4, 6, good)


def test_ring_edges_and_display():
    raw = np.stack([np.full((24, 41), v, dtype=np.float32) for v in (0.5, 100.0, 3.0, -0.25, 70.0)])
    maps, png = er.line_emission_finish(raw, 1.0, 0.0, 0.0, 24, 41, (20.0, 12.0, 5.0, 10.0), None, 3, 2.0)
    m = maps[1]
    assert np.isnan(m[12, 25]) and np.isnan(m[16, 23]) and np.isnan(m[12, 20])      # on r_in (3-4-5 too) and inside: masked
    assert m[12, 26] == 100.0 and m[12, 30] == 100.0 and m[20, 26] == 100.0         # just outside r_in, on r_out (6-8-10 too): kept
    assert np.isnan(m[12, 31])
    assert png[4][12, 26] == 10 and png[1][12, 26] == 100 and png[4][12, 31] == 0   # flux / (2H + 1) = 70 / 7
    on_disk, _ = er.line_emission_finish(raw, 1.0, 0.0, 0.0, 24, 41, (20.0, 12.0, -1.0, np.inf))
    assert np.isfinite(on_disk).all()
    # flux display ties and clips at H = 3: e = v / 7, rint half to even
    v = np.array([3.5, 10.5, 17.5, 24.5, 0.0, -7.0, 7.0 * 65534.5, 7.0 * 65535.5, 1e9, np.nan, np.inf], dtype=np.float32)
    assert list(er.flux_display(v, 3)) == [1, 2, 2, 4, 1, 1, 65534, 65535, 65535, 0, 65535]


@pytest.fixture(scope='module', params=sorted(er.TOLERANCE))
def measured(request):
    noise = request.param
    frames, truth = er.scene(IH, N, IW, noise)
    return noise, frames, truth


def test_accuracy_on_the_scene(measured):
    noise, frames, truth = measured
    worst = {}
    for off in ref.FIT_OFFSETS:
        fit = fit_at(truth['centre'] + off)
        planes = er.line_emission(frames, fit, 10, 0, er.MIN_EXCESS)
        for name, (rms, mx, nans) in er.scene_errors(planes, fit, truth, 2.0 * er.MIN_EXCESS).items():
            w = worst.get(name, (0.0, 0.0, 0))
            worst[name] = (max(w[0], rms), max(w[1], mx), max(w[2], nans))
    print('noise %g: %s' % (noise, worst))
    for name, (rms_tol, max_tol) in er.TOLERANCE[noise].items():
        rms, mx, nans = worst[name]
        assert rms <= rms_tol and mx <= max_tol and nans <= er.NAN_ALLOWED[noise][name], name
        assert rms_tol <= 1.1 * rms and max_tol <= 1.1 * mx, '%s: the recorded tolerance is more than 10 %% above the measurement' % name


def test_gate_rates_on_the_scene(measured):
    noise, frames, truth = measured
    fit = fit_at(truth['centre'])
    finite_sky, lost, kept = er.gate_rates(er.line_emission(frames, fit, 10, 0, er.MIN_EXCESS), truth, er.MIN_EXCESS)
    open_sky = er.gate_rates(er.line_emission(frames, fit, 10, 0, 0.0), truth, er.MIN_EXCESS)[0]
    print('noise %g: %.4f of the empty sky finite at 6 sigma (%.4f at min_excess 0), %.4f of the prominence lost, %d kept'
          % (noise, finite_sky, open_sky, lost, kept))
    assert kept >= 200
    assert finite_sky <= er.GATE['finite_sky'] * 1.1 and lost <= er.GATE['lost_prominence'] * 1.1
    if noise > 0:
        assert open_sky > 0.5                                    # the gate is what empties the sky: noise bumps pass at 0
