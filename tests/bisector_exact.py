"""Exact restatement of shg_line_bisector (include/shg_hip.h), one (slit row, frame) at a time, in Python int and
fractions.Fraction, in the manner of tests/profile_exact.py (whose window and vertex it takes): every value is the mathematical one
the header's formulas define, with no rounding anywhere, or None where the header says NaN.  The level of fraction f is the exact
(1 - f) core + f C2 / 2 with f the exact value of the float64 fraction.  Written from the header, not from the kernels nor from
tests/bisector_ref.py.

Also seeded adversarial rows for the level decisions on top of tests/profile_adversarial.py's (which already hold unbracketed
minima, C2 = 0, emission lines with C2 / 2 <= core, ties and window edges): a sample at ceil(level) or ceil(level) - 1 beside the
core, integral levels, p(j*) equal to the level, and crossings on the window's edges.  level_decisions() reports, case by case,
whether the float64 level takes the exact level's decisions (b < level, p >= level for every sample of the window)."""
import math
from fractions import Fraction

import numpy as np

from tests import profile_adversarial as adv
from tests import profile_exact as ex

U64 = ex.U64
SLACK = ex.SLACK
# the level sets the tests run: one level, the usual four, dyadic levels (integral levels need them), and eight reaching near 0 and 1
LEVEL_SETS = ((0.5,), (0.2, 0.4, 0.6, 0.8), (0.25, 0.5, 0.75), (1e-6, 0.1, 0.3, 0.45, 0.55, 0.7, 0.9, 1.0 - 1e-6))


def level64(f, core_d, c2):
    """The header's float64 level: ((1.0 - f) * core_d) + (f * (0.5 * (double)C2))."""
    return ((1.0 - f) * core_d) + (f * (0.5 * float(c2)))


def measure(p, lo, hi, f3, levels, shift=0):
    """The exact bisector and chord of one profile p (Python ints) over [lo, hi] at each level: a dict with profile_exact.measure's
    vertex record ('vertex') and, per level, a dict with f, level (Fraction or None), has (b < level), jl, jr, bis, chord (Fraction
    or None) and the samples either side of the crossings."""
    r = ex.measure(p, lo, hi, f3, shift)
    f3 = float(f3)
    ref = Fraction(f3) + shift if math.isfinite(f3) else None
    out = {'vertex': r, 'levels': []}
    for f in levels:
        L = dict(f=f, level=None, has=False, jl=None, jr=None, bis=None, chord=None, p_cross=None)
        out['levels'].append(L)
        if r['core'] is None:
            continue
        F = Fraction(f)
        level = (1 - F) * r['core'] + F * Fraction(r['C2'], 2)
        L['level'] = level
        if not r['b'] < level:
            continue
        L['has'] = True
        left = [j for j in range(lo, r['jstar']) if p[j] >= level]
        right = [j for j in range(r['jstar'] + 1, hi + 1) if p[j] >= level]
        L['jl'] = left[-1] if left else None
        L['jr'] = right[0] if right else None
        if left and right:
            jl, jr = left[-1], right[0]
            xl = jl + (p[jl] - level) / (p[jl] - p[jl + 1])
            xr = jr - (p[jr] - level) / (p[jr] - p[jr - 1])
            L['chord'] = xr - xl
            L['p_cross'] = (p[jl], p[jl + 1], p[jr], p[jr - 1])
            if ref is not None:
                L['bis'] = (xl + xr) / 2 - ref
    return out


def bound(rec, L, plane, shift=0):
    """The largest |computed - exact| the header's operations allow for one level's bisector or chord (as profile_exact.bound):
      core: E_c = u (q + |core|), q = d^2 / (8 den)
      level: t = 1 - f (u |1 - f|), t core_d, f (0.5 C2), their sum:  E_l = |1 - f| E_c + 2 u |1 - f| |core| + u |f C2 / 2| + u |level|
      xl = jl + (p(jl) - level) / Dl:  E_xl = (E_l + u |p(jl) - level|) / Dl + u |fl| + u |xl|, the same on the right
      chord = xr - xl:  E_xl + E_xr + u |chord|
      bis = 0.5 (xl + xr) - ref:  E_xl + E_xr + u |xl + xr| + u (|mid| + |ref| + |bis|)   (0.5 x exact; ref = f3 + S: u |ref|)
    Every E times SLACK, plus one float32 ulp of |exact| + E for the final cast."""
    r, u = rec['vertex'], U64
    x = L[plane]
    F = Fraction(L['f'])
    core, level = r['core'], L['level']
    q = Fraction(r['d'] ** 2, 8 * r['den'])
    e_c = u * (q + abs(core))
    e_l = abs(1 - F) * e_c + 2 * u * abs(1 - F) * abs(core) + u * abs(F * Fraction(r['C2'], 2)) + u * abs(level)
    pl, pl1, pr, pr1 = L['p_cross']
    dl, dr = pl - pl1, pr - pr1
    fl, fr = (pl - level) / dl, (pr - level) / dr
    xl, xr = L['jl'] + fl, L['jr'] - fr
    e_xl = (e_l + u * abs(pl - level)) / dl + u * abs(fl) + u * abs(xl)
    e_xr = (e_l + u * abs(pr - level)) / dr + u * abs(fr) + u * abs(xr)
    if plane == 'chord':
        E = e_xl + e_xr + u * abs(x)
    else:
        mid = (xl + xr) / 2
        ref = mid - x
        E = e_xl + e_xr + u * abs(xl + xr) + u * (abs(mid) + abs(ref) + abs(x))
    E *= SLACK
    return ex.ulp32(abs(x) + E) + E


def level_decisions(rec):
    """Per level with a vertex: (exact decisions, float64 decisions) of b < level and of p(j) >= level over the window; the float64
    ones also through ceil(level) for integer p, as the kernel takes them."""
    r = rec['vertex']
    out = []
    for L in rec['levels']:
        if L['level'] is None:
            continue
        lv = level64(L['f'], float(r['b']) - float(r['d'] * r['d']) / (8.0 * float(r['den'])), r['C2'])
        p = r['p'][r['lo']:r['hi'] + 1]
        exact = (r['b'] < L['level'],) + tuple(v >= L['level'] for v in p)
        f64 = (float(r['b']) < lv,) + tuple(v >= lv for v in p)
        thr = (float(r['b']) < lv,) + tuple(v >= math.ceil(lv) for v in p)
        out.append((exact, f64, thr, L))
    return out


def records(P, fit, half_width, levels, shift=0):
    """measure() of every (slit row y, frame k) of the profiles P [n, ih, iw] (rotated-frame coordinates, sample scale):
    records[y][k], None for rows without a window."""
    n, ih, iw = P.shape
    out = []
    for y in range(ih):
        win = ex.window(fit[y][0], shift, half_width, iw)
        if win is None:
            out.append(None)
            continue
        row = []
        for k in range(n):
            p = [int(v) for v in P[k, y]]
            rec = measure(p, win[0], win[1], fit[y][3], levels, shift)
            rec['vertex']['p'] = p
            row.append(rec)
        out.append(row)
    return out


def within(got, recs, i, plane, shift=0, skip=None):
    """Check one computed plane float32 [ih, n] of level i against the records: NaN exactly where the exact value is None, and
    |got - exact| <= bound() elsewhere; (y, k) in `skip` are left out (cases whose float64 level decides otherwise).  Returns the
    largest |got - exact| / bound."""
    worst = 0.0
    for y, row in enumerate(recs):
        for k in range(got.shape[1]):
            if skip and (y, k) in skip:
                continue
            g = float(got[y, k])
            L = None if row is None else row[k]['levels'][i]
            x = None if L is None else L[plane]
            if x is None:
                assert math.isnan(g), '%s %d (%d, %d): %r where the exact value is NaN' % (plane, i, y, k, g)
                continue
            assert math.isfinite(g), '%s %d (%d, %d): %r where the exact value is %s' % (plane, i, y, k, g, float(x))
            err = abs(Fraction(g) - x)
            b = bound(row[k], L, plane, shift)
            assert err <= b, '%s %d (%d, %d): %r is %g from the exact %r, bound %g' % (plane, i, y, k, g, float(err), float(x), float(b))
            worst = max(worst, float(err / b))
    return worst


# ---- adversarial rows for the levels ----
KINDS = ('hit_left', 'hit_right', 'integral', 'best_eq', 'edges')


def _level_row(kind, k, rng, Q, iw, lo, hi, levels):
    """One profile (raw ints 0..Q) of a level class for frame k, or None when the window is too narrow.  Levels scale with the
    samples (x 256 for 8-bit files is exact), so the classes are built in raw units."""
    if hi - lo < 6:
        return None
    p = rng.integers(0, Q + 1, iw)
    js = int(rng.integers(lo + 3, hi - 2))
    if kind == 'best_eq':                  # p(lo) = b + 1, a = b + 4, e = p(hi) = b: at f = 0.5 the level is b itself
        b = int(rng.integers(0, Q - 8))
        p[lo:hi + 1] = rng.integers(b + 1, Q + 1, hi - lo + 1)
        p[js + 1:hi + 1] = rng.integers(b, Q + 1, hi - js)
        p[lo], p[js - 1], p[js], p[js + 1], p[hi] = b + 1, b + 4, b, b, b
        return p
    if kind == 'integral':                 # a = e: core = b; b and C2 / 2 multiples of 4: the levels at f = k / 4 are integers
        b = 4 * int(rng.integers(0, Q // 16))
        alpha = eps = int(rng.integers(1, 4))
        c2h = 4 * int(rng.integers((b + Q // 4) // 4, Q // 4))
        plo = min(Q, c2h + int(rng.integers(0, 4)))
        phi = 2 * c2h - plo
    else:
        b = int(rng.integers(0, Q // 4))
        alpha, eps = (int(v) for v in rng.integers(1, max(Q // 16, 2), 2))
        plo, phi = (int(v) for v in rng.integers(b + Q // 2, Q + 1, 2))
    core = b - (alpha - eps) ** 2 / (8.0 * (alpha + eps))
    for t in range(len(levels)):           # the frame's level, else the next one with room between the core and the continuum
        c = math.ceil(level64(levels[(k + t) % len(levels)], core, plo + phi))
        if b + max(alpha, eps) < c - 1 and c <= Q:
            break
    else:
        return None
    # every interior sample above b and below the level, then one sample at ceil(level) or ceil(level) - 1
    p[lo:hi + 1] = rng.integers(b + max(alpha, eps) + 1, c, hi - lo + 1)
    p[lo], p[hi] = plo, phi
    p[js - 1], p[js], p[js + 1] = b + alpha, b, b + eps
    hit = c if (k // len(levels)) % 2 == 0 else c - 1
    if kind == 'hit_left':
        p[int(rng.integers(lo + 1, js - 1))] = hit
    elif kind == 'hit_right':
        p[int(rng.integers(js + 2, hi))] = hit
    elif kind == 'integral':
        p[int(rng.integers(lo + 1, js - 1))] = hit
        p[int(rng.integers(js + 2, hi))] = c if hit == c - 1 else c - 1
    elif kind == 'edges':                  # the crossings on the window's edges, or a side that never reaches the level
        if k % 3 == 1:
            p[lo] = c - 1
        elif k % 3 == 2:
            p[hi] = c - 1
    return p


def profiles(n, ih, iw, bits, half_width, levels, shift=0, seed=0):
    """(P int64 [n, ih, iw] on the sample scale, fit [ih, 4], classes [ih]): profile_adversarial's rows, every third slit row
    (with a window wide enough) replaced by a level class."""
    P, fit, cls = adv.profiles(n, ih, iw, bits, half_width, shift, seed)
    rng = np.random.default_rng([seed, n, ih, iw, bits, half_width, shift + 1000, len(levels), 7])
    Q, scale = (65535, 1) if bits == 16 else (255, 256)
    cls = list(cls)
    for y in range(2, ih, 3):
        win = ex.window(fit[y, 0], shift, half_width, iw)
        if win is None:
            continue
        kind = KINDS[(y // 3) % len(KINDS)]
        rows = [_level_row(kind, k, rng, Q, iw, *win, levels) for k in range(n)]
        if any(r is None for r in rows):
            continue
        P[:, y] = np.stack(rows) * scale
        cls[y] = kind
    return P, fit, cls
