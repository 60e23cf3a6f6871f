"""Exact restatement of shg_line_emission (include/shg_hip.h), one (slit row, frame) at a time, in Python int and
fractions.Fraction, in the manner of tests/linemaps_exact.py (whose window, ulp32, U64, SLACK and within() it shares): every value
is the mathematical one the header's formulas define, or None where the header says NaN.  Written from the header, not from the
kernels nor from tests/emission_ref.py.

The decisions, all exact: the first maximum; the bracket lo < j* < hi; excess >= E (E the exact value of the float64 min_excess);
p(j) <= half and p(j*) > half with half = B2/4 + b/2 - d^2/(16 den) (den < 0); S0 <= 0.  decisions64() takes the two that involve
a rounded float64 (the gate and the half level) as the header's float64 steps take them, for the tests to compare case by case.

bound() turns the header's sequence of IEEE operations into a tolerance for each plane."""
import math
from fractions import Fraction

from tests.linemaps_exact import SLACK, U64, ulp32, window, within  # noqa: F401  (within and window are part of this module's use)

PLANES = ('shift', 'peak', 'width', 'cog', 'flux')


def measure(p, lo, hi, f3, shift=0, min_excess=0.0):
    """Every intermediate and the exact planes of one profile p (Python ints) over [lo, hi]."""
    p = [int(v) for v in p]
    f3 = float(f3)
    ref = Fraction(f3) + shift if math.isfinite(f3) else None
    E = Fraction(float(min_excess))
    r = dict(p=p, lo=lo, hi=hi, jstar=None, bracket=False, gate=False, a=None, b=None, e=None, den=None, d=None, peak_d=None,
             excess=None, half=None, has_width=False, jl=None, jr=None, p_cross=None, shift=None, peak=None, width=None, cog=None,
             flux=None)
    js = range(lo, hi + 1)
    B2 = p[lo] + p[hi]
    S0 = 2 * sum(p[j] for j in js) - len(js) * B2
    S1 = 2 * sum(j * p[j] for j in js) - B2 * sum(js)
    r.update(B2=B2, S0=S0, S1=S1)
    best = max(p[j] for j in js)
    jstar = next(j for j in js if p[j] == best)                  # the first maximum
    r['jstar'] = jstar
    if jstar == lo or jstar == hi:
        return r
    a, b, e = p[jstar - 1], p[jstar], p[jstar + 1]
    den, d = a + e - 2 * b, a - e
    assert den < 0                                               # a < b (first maximum), e <= b
    peak_d = b - Fraction(d * d, 8 * den)
    excess = peak_d - Fraction(B2, 2)
    r.update(bracket=True, a=a, b=b, e=e, den=den, d=d, peak_d=peak_d, excess=excess, gate=excess >= E)
    if not r['gate']:
        return r
    r['peak'] = excess
    if ref is not None:
        r['shift'] = jstar + Fraction(d, 2 * den) - ref
    if S0 > 0:
        r['flux'] = Fraction(S0, 2)
        if ref is not None:
            r['cog'] = Fraction(S1, S0) - ref
    half = Fraction(B2, 4) + Fraction(b, 2) - Fraction(d * d, 16 * den)
    r['half'] = half
    if not b > half:
        return r
    left = [j for j in range(lo, jstar) if p[j] <= half]
    right = [j for j in range(jstar + 1, hi + 1) if p[j] <= half]
    r.update(has_width=True, jl=left[-1] if left else None, jr=right[0] if right else None)
    if left and right:
        jl, jr = left[-1], right[0]
        xl = jl + (half - p[jl]) / (p[jl + 1] - p[jl])
        xr = jr - (half - p[jr]) / (p[jr - 1] - p[jr])
        r.update(width=xr - xl, p_cross=(p[jl], p[jl + 1], p[jr], p[jr - 1]))
    return r


def records(P, fit, half_width, shift=0, min_excess=0.0):
    """measure() of every (slit row y, frame k) of the profiles P [n, ih, iw]: records[y][k], None for rows without a window."""
    n, ih, iw = P.shape
    out = []
    for y in range(ih):
        win = window(fit[y][0], shift, half_width, iw)
        out.append(None if win is None else [measure(P[k, y], win[0], win[1], fit[y][3], shift, min_excess) for k in range(n)])
    return out


def decisions64(r, min_excess=0.0):
    """(exact, float64) decisions of a bracketed record: the gate, then (past it) p(j*) > half and p(j) <= half over the window, the
    float64 ones by the header's steps (and through floor(half) for integer p, as a kernel may take them)."""
    peak64 = float(r['b']) - float(r['d'] * r['d']) / (8.0 * float(r['den']))
    excess64 = peak64 - 0.5 * float(r['B2'])
    exact, f64 = [r['gate']], [excess64 >= float(min_excess)]
    if r['gate'] and f64[0]:
        half64 = 0.5 * (0.5 * float(r['B2']) + peak64)
        win = r['p'][r['lo']:r['hi'] + 1]
        exact += [r['b'] > r['half']] + [v <= r['half'] for v in win]
        f64 += [float(r['b']) > half64] + [v <= half64 for v in win]
        assert f64[2:] == [v <= math.floor(half64) for v in win]
    return exact, f64


def bound(r, plane):
    """The largest |computed - exact| the header's operations allow for one plane (as linemaps_exact.bound): E, the float64 rounding
    of the stated steps, times SLACK, plus one float32 ulp of |exact| + E for the final cast.  u = 2^-53.
      shift: q = (a-e)/(2 den), t = j* + q, ref' = f3 + S, s = t - ref'.      E = u (|q| + (|j*| + |q|) + |ref| + |shift|)
      peak:  q = d^2/(8 den), c = b - q, x = c - 0.5 B2.                       E_p = u (|q| + |peak_d|), E = E_p + u |excess|
      half:  h = 0.5 (0.5 B2 + c)                                              E_h = E_p + u |2 half|
      width: nl = h - p(jl), fl = nl / Dl, xl = jl + fl (Dl = p(jl+1) - p(jl) >= 1), the same on the right, w = xr - xl.
             E = E_h (1/Dl + 1/Dr) + u (2|fl| + |xl| + 2|fr| + |xr| + |width|)
      cog:   g = S1/S0, c = g - ref'.                                          E = u (|S1/S0| + |ref| + |cog|)
      flux:  0.5 S0 is exact.                                                  E = 0"""
    x = r[plane]
    u = U64
    q8 = abs(Fraction(r['d'] ** 2, 8 * r['den']))
    e_p = u * (q8 + abs(r['peak_d']))
    if plane == 'shift':
        q = Fraction(r['d'], 2 * r['den'])
        ref = r['jstar'] + q - x
        E = u * (abs(q) + abs(r['jstar']) + abs(q) + abs(ref) + abs(x))
    elif plane == 'peak':
        E = e_p + u * abs(x)
    elif plane == 'width':
        p_jl, p_jl1, p_jr, p_jr1 = r['p_cross']
        half = r['half']
        e_half = e_p + u * 2 * abs(half)
        dl, dr = p_jl1 - p_jl, p_jr1 - p_jr
        fl, fr = (half - p_jl) / dl, (half - p_jr) / dr
        xl, xr = r['jl'] + fl, r['jr'] - fr
        E = e_half * (Fraction(1, dl) + Fraction(1, dr)) + u * (2 * abs(fl) + abs(xl) + 2 * abs(fr) + abs(xr) + abs(x))
    elif plane == 'cog':
        g = Fraction(r['S1'], r['S0'])
        ref = g - x
        E = u * (abs(g) + abs(ref) + abs(x))
    else:
        E = Fraction(0)
    E *= SLACK
    return ulp32(abs(x) + E) + E


def plane(name):
    """within()'s (value, bound) for a PLANES plane."""
    return (lambda r: r[name]), (lambda r: bound(r, name))
