"""The NumPy restatement of the line-core and line-profile kernels (tests/linemaps_ref.py) against the exact reference
(tests/linemaps_exact.py) on seeded adversarial profiles (tests/profile_adversarial.py) and on a synthetic scan:
NaN where the exact value is NaN, and within the bound the header's operations allow everywhere else.  Also the argument that
the float64 half level always takes the exact decision, checked case by case."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import linemaps_exact as ex
from tests import linemaps_ref as ref
from tests import profile_adversarial as adv

LAYOUTS = [  # (name, n, ih, iw, bits, half_width, shift, rotated file)
    ('rot_u16', 12, 304, 48, 16, 7, 0, True),
    ('rot_u8', 12, 301, 48, 8, 7, 0, True),
    ('plain_u16', 131, 45, 40, 16, 7, 0, False),
    ('plain_u8', 40, 45, 40, 8, 5, 0, False),
    ('h1', 12, 200, 40, 16, 1, 0, True),
    ('h32', 12, 320, 72, 16, 32, 0, True),
    ('h32_u8_plain', 20, 80, 72, 8, 32, 0, False),
    ('s_plus', 12, 304, 48, 16, 7, 48 - 4 + 7, True),
    ('s_minus', 12, 304, 48, 8, 7, -(48 - 4 + 7), True),
    ('s_mid', 12, 301, 48, 16, 5, -13, True),
]


def check_coverage(name, counts, half_width, shift):
    print('%s: %s' % (name, ', '.join('%s %d' % kv for kv in sorted(counts.items()))))
    if half_width >= 5 and shift == 0:
        missing = [c for c in adv.REQUIRED if not counts.get(c)]
        assert not missing, 'classes never reached: %s' % missing
    if half_width == 32:
        assert counts.get('maxsum'), 'no window of 65 samples at the maximum'


@pytest.mark.parametrize('layout', LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_restatements_agree_with_the_exact_reference(layout):
    name, n, ih, iw, bits, hw, shift, rot = layout
    P, fit, cls = adv.profiles(n, ih, iw, bits, hw, shift, seed=5)
    raw = adv.to_file(P, bits, rot)
    assert (raw.shape[2] > raw.shape[1]) == rot
    assert np.array_equal(np.stack([ref.profiles(raw, y) for y in range(ih)], axis=1), P)   # the layout round trip
    records = {s: ex.records(P, fit, hw, s) for s in sorted({0, shift})}
    check_coverage(name, adv.occurrences(records[shift], cls, fit, bits, shift), hw, shift)
    worst = {'line_core_shift': ex.within(ref.line_core_shift(raw, fit, hw), records[0], *ex.plane('shift'))}
    for s, rec in records.items():
        planes = ref.line_profile(raw, fit, hw, s)
        for q, plane in enumerate(ref.PLANES):
            worst['%s S=%d' % (plane, s)] = ex.within(planes[q], rec, *ex.plane(plane, s))
            assert np.isfinite(planes[q]).any() and np.isnan(planes[q]).any(), plane
    print('%s: largest error / bound %s' % (name, ', '.join('%s %.3f' % kv for kv in worst.items())))


def test_restatements_agree_on_a_synthetic_scan():
    from solex_ser_recon_en_amd import synth
    n, width, height, hw = 24, 301, 40, 6
    frames = synth.synth_frames_numpy(n, width, height, 16, seed=11, tilt=0.01, curv=2e-5)
    ih, iw = width, height
    rng = np.random.default_rng(2)
    centre = synth.curve_of_row(np.arange(ih, dtype=np.float64), ih, iw) + rng.uniform(-3.0, 3.0, ih)
    centre[0:ih:11] = rng.uniform(-1.5, 4.0, centre[0:ih:11].shape)                  # windows on either frame edge
    centre[5:ih:13] = rng.uniform(iw - 5.0, iw + 1.5, centre[5:ih:13].shape)
    fit = np.stack([np.floor(centre), centre - np.floor(centre), np.arange(ih, dtype=np.float64), centre], axis=1)
    fit[3, 0], fit[7, 0], fit[9, 3] = np.nan, np.inf, np.nan
    P = np.stack([ref.profiles(frames, y) for y in range(ih)], axis=1)
    for s in (0, 4):
        rec = ex.records(P, fit, hw, s)
        planes = ref.line_profile(frames, fit, hw, s)
        for q, plane in enumerate(ref.PLANES):
            ex.within(planes[q], rec, *ex.plane(plane, s))
            assert np.isfinite(planes[q]).any(), plane
        if s == 0:
            ex.within(ref.line_core_shift(frames, fit, hw), rec, *ex.plane('shift'))
            assert np.isfinite(planes[2]).mean() > 0.5


def test_float64_half_takes_the_exact_decision():
    """half = C2/4 + b/2 - d^2/(16 den) exactly.  When it is an integer, d^2/(8 den) is a multiple of 1/2, so every float64 step
    of the header (q = d^2/(8 den), b - q, 0.5 C2 + core, x 0.5) is exact and the float64 half is the exact one.  Otherwise the
    exact half, a fraction over 16 den, is at least 1/(16 den) from every integer, and the float64 half is closer to it than that
    (linemaps_exact.bound's E_half): p >= half and b < half come out the same for every integer p, and so does p >= ceil(half)."""
    n_int = n_frac = 0
    for name, n, ih, iw, bits, hw, shift, _ in LAYOUTS:
        P, fit, _ = adv.profiles(n, ih, iw, bits, hw, shift, seed=5)
        for row in ex.records(P, fit, hw, shift):
            for r in row or ():
                if r['half'] is None:
                    continue
                b, d, den, c2, half = r['b'], r['d'], r['den'], r['C2'], r['half']
                core = float(b) - float(d * d) / (8.0 * float(den))
                half64 = 0.5 * (0.5 * float(c2) + core)
                if half.denominator == 1:
                    n_int += 1
                    assert (2 * d * d) % (8 * den) == 0 and Fraction(half64) == half
                else:
                    n_frac += 1
                    gap = min(half - math.floor(half), math.ceil(half) - half)
                    e_half = ex.U64 * ex.SLACK * (Fraction(d * d, 8 * den) + abs(r['core']) + 2 * abs(half))
                    assert gap >= Fraction(1, 16 * den) > e_half and abs(Fraction(half64) - half) <= e_half
                assert (b < half64) == r['has_width']
                thr = math.ceil(half64)
                for j in range(r['lo'], r['hi'] + 1):
                    exact = 16 * den * r['p'][j] >= 4 * den * c2 + 8 * den * b - d * d
                    assert (r['p'][j] >= half64) == exact == (r['p'][j] >= thr)
    print('integer half levels %d, fractional %d' % (n_int, n_frac))
    assert n_int > 100 and n_frac > 1000


def test_exact_reference_by_hand():
    """A few values of linemaps_exact worked out on paper, so that the reference itself is pinned."""
    # window: truncation toward zero (not floor), the 2^30 clamp, non-finite lines
    assert ex.window(-0.5, 0, 5, 40) == (1, 5) and ex.window(-1.5, 0, 5, 40) == (1, 4)
    assert ex.window(2.0 ** 31, 0, 5, 40) is None and ex.window(1e300, 0, 5, 40) is None and ex.window(math.nan, 0, 5, 40) is None
    assert ex.window(36.9, 0, 5, 40) == (31, 38) and ex.window(0.5, 36, 5, 40) == (31, 38)
    # a = 9, b = 1, e = 5 at j* = 3, window [1, 5]: den = 12, d = 4
    p = [0, 20, 9, 1, 5, 20, 0]
    r = ex.measure(p, 1, 5, 2.5)
    assert r['jstar'] == 3 and r['shift'] == 3 + Fraction(4, 24) - Fraction(5, 2)
    assert r['core'] == 1 - Fraction(16, 96) and r['half'] == Fraction(40, 4) + Fraction(1, 2) - Fraction(16, 192)
    # half = 10.41666...: jl = 1 (20 >= half, 9 < half), jr = 5
    assert (r['jl'], r['jr']) == (1, 5)
    assert r['width'] == (5 - (20 - r['half']) / 15) - (1 + (20 - r['half']) / 11)
    s0 = 5 * 40 - 2 * 55
    assert r['S0'] == s0 and r['cog'] == Fraction(40 * 15 - 2 * (20 + 18 + 3 + 20 + 100), s0) - Fraction(5, 2)
    assert r['ew'] == Fraction(s0, 40)
    # the first of tied minima; none on the window's edge; best >= half (p(lo) = b + 1, a = b + 4, e = p(hi) = b: half = b)
    assert ex.measure([0, 7, 3, 3, 9, 0], 1, 4, 0.0)['jstar'] == 2
    assert ex.measure([0, 1, 2, 3, 4, 0], 1, 4, 0.0)['shift'] is None
    r = ex.measure([0, 11, 14, 10, 10, 10, 0], 1, 5, 0.0)
    assert r['half'] == r['b'] == 10 and not r['has_width'] and r['width'] is None
    # C2 = 0: no cog, no ew
    r = ex.measure([5, 0, 0, 0, 0, 5], 1, 4, 0.0)
    assert r['C2'] == 0 and r['cog'] is None and r['ew'] is None
    assert ex.ulp32(Fraction(1)) == Fraction(1, 2 ** 23) and ex.ulp32(Fraction(3, 4)) == Fraction(1, 2 ** 24)
