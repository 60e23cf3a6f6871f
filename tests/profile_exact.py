"""Exact restatement of shg_line_core_shift and shg_line_profile (include/shg_hip.h), one (slit row, frame) at a time, in Python
int and fractions.Fraction: every value is the mathematical one the header's formulas define, with no rounding anywhere, or None
where the header says NaN.  Written from the header, not from the kernels nor from doppler_ref.py / lineprofile_ref.py.

The one float64 operation kept is the header's window: c = (int64)(fit[y][0] + (double)S), where the sum is itself part of the
definition.  The half-level decisions are made in integers (den > 0):
    p >= half   <=>  16 den p >= 4 den C2 + 8 den b - d^2
    b <  half   <=>   8 den b <  4 den C2 - d^2
and ref = Fraction(fit[y][3]) + S.

bound() turns the header's sequence of IEEE operations into a tolerance for each computed value; within() checks a plane."""
import math
from fractions import Fraction

PLANES = ('shift', 'core', 'width', 'cog', 'ew')
CLAMP = 2 ** 30
U64 = Fraction(1, 2 ** 53)          # unit roundoff of float64 (round to nearest)
SLACK = Fraction(10001, 10000)      # covers the products of two or more rounding errors (each <= 2^-53 relative)


def window(f0, shift, half_width, iw):
    """(lo, hi) or None.  c = f0 + S in float64, clamped to +-2^30 and truncated toward zero; lo = max(c - H, 1),
    hi = min(c + H, iw - 2); none when f0 is not finite or hi - lo < 2."""
    f0 = float(f0)
    if not math.isfinite(f0):
        return None
    x = Fraction(f0 + float(shift))
    c = int(min(max(x, Fraction(-CLAMP)), Fraction(CLAMP)))      # int(Fraction) truncates toward zero
    lo, hi = max(c - half_width, 1), min(c + half_width, iw - 2)
    return None if hi - lo < 2 else (lo, hi)


def measure(p, lo, hi, f3, shift=0):
    """Every intermediate and the five exact values of one profile p (a sequence of Python ints) over [lo, hi]: a dict with lo,
    hi, jstar, a, b, e, den, d, C2, S0, S1, half (None without a vertex), has_width, jl, jr and the PLANES (Fraction or None)."""
    p = [int(v) for v in p]
    f3 = float(f3)
    ref = Fraction(f3) + shift if math.isfinite(f3) else None      # (NaN propagates: no finite shift or cog)
    r = dict(lo=lo, hi=hi, jstar=None, a=None, b=None, e=None, den=None, d=None, half=None, has_width=False, jl=None, jr=None,
             shift=None, core=None, width=None, cog=None, ew=None)
    js = range(lo, hi + 1)
    n = hi - lo + 1
    C2 = p[lo] + p[hi]
    S0 = n * C2 - 2 * sum(p[j] for j in js)
    S1 = C2 * sum(js) - 2 * sum(j * p[j] for j in js)
    r.update(C2=C2, S0=S0, S1=S1)
    if S0 > 0 and ref is not None:
        r['cog'] = Fraction(S1, S0) - ref
    if C2 != 0:
        r['ew'] = Fraction(S0, C2)
    best = min(p[j] for j in js)
    jstar = next(j for j in js if p[j] == best)                  # the first minimum
    r['jstar'] = jstar
    if jstar == lo or jstar == hi:
        return r
    a, b, e = p[jstar - 1], p[jstar], p[jstar + 1]
    den, d = a + e - 2 * b, a - e
    assert den > 0                                               # a > b (first minimum), e >= b
    r.update(a=a, b=b, e=e, den=den, d=d)
    if ref is not None:
        r['shift'] = jstar + Fraction(d, 2 * den) - ref
    r['core'] = b - Fraction(d * d, 8 * den)
    r['half'] = Fraction(C2, 4) + Fraction(b, 2) - Fraction(d * d, 16 * den)
    rhs = 4 * den * C2 + 8 * den * b - d * d                     # p >= half  <=>  16 den p >= rhs
    if not 8 * den * b < 4 * den * C2 - d * d:                   # b < half
        return r
    ge = [16 * den * p[j] >= rhs for j in range(len(p))]
    left = [j for j in range(lo, jstar) if ge[j]]
    right = [j for j in range(jstar + 1, hi + 1) if ge[j]]
    r['has_width'] = True
    r['jl'] = left[-1] if left else None
    r['jr'] = right[0] if right else None
    if left and right:
        half, jl, jr = r['half'], left[-1], right[0]
        xl = jl + (p[jl] - half) / (p[jl] - p[jl + 1])
        xr = jr - (p[jr] - half) / (p[jr] - p[jr - 1])
        r['width'] = xr - xl
    return r


def ulp32(x):
    """The float32 ulp at |x| (a Fraction): 2^(e - 24) for |x| in [2^(e-1), 2^e), 2^-149 below the normals."""
    x = abs(x)
    if x < Fraction(1, 2 ** 126):
        return Fraction(1, 2 ** 149)
    e = x.numerator.bit_length() - x.denominator.bit_length()   # 2^(e-1) < x < 2^(e+1)
    if Fraction(2) ** e <= x:
        e += 1
    return Fraction(2) ** (e - 24)


def bound(r, plane, shift=0):
    """The largest |computed - exact| the header's sequence of operations allows for one plane of a measure() record: E, the
    float64 rounding of the stated steps (each IEEE operation adds at most 2^-53 of the magnitude of its exact result; integers
    below 2^53 and the products by 0.5 and by 8.0 are exact), plus one float32 ulp of |exact| + E for the final (float) cast
    (round to nearest adds half an ulp of the float64 value, whose ulp is at most one binade above the exact value's).
      shift: q = (a-e)/(2 den), t = j* + q, ref' = f3 + S, s = t - ref'.      E = u (|q| + (|j*| + |q|) + |ref| + |shift|)
      core:  q = d^2/(8 den), c = b - q.                                       E = u (|q| + |core|)
      half:  h = 0.5 (0.5 C2 + c)                                              E_h = E_core + u |2 half|
      width: nl = p(jl) - h, fl = nl / Dl, xl = jl + fl (Dl = p(jl) - p(jl+1) >= 1), the same on the right, w = xr - xl.
             E = E_h (1/Dl + 1/Dr) + u (2|fl| + |xl| + 2|fr| + |xr| + |width|)
      cog:   g = S1/S0, c = g - ref'.                                          E = u (|S1/S0| + |ref| + |cog|)
      ew:    S0/C2.                                                            E = u |ew|
    Every E is multiplied by SLACK for the second-order terms.  ref = f3 + S exact; with S = 0 the sum is exact, which only
    makes the bound conservative.  The absolute part matters where shift and cog cancel to near zero."""
    x = r[plane]
    u = U64
    if plane == 'shift':
        q = Fraction(r['d'], 2 * r['den'])
        ref = r['jstar'] + q - x
        E = u * (abs(q) + abs(r['jstar']) + abs(q) + abs(ref) + abs(x))
    elif plane == 'core':
        E = u * (Fraction(r['d'] ** 2, 8 * r['den']) + abs(x))
    elif plane == 'width':
        p_jl, p_jl1, p_jr, p_jr1 = r['p_cross']
        half = r['half']
        e_half = u * (Fraction(r['d'] ** 2, 8 * r['den']) + abs(r['core']) + 2 * abs(half))
        dl, dr = p_jl - p_jl1, p_jr - p_jr1
        fl, fr = (p_jl - half) / dl, (p_jr - half) / dr
        xl, xr = r['jl'] + fl, r['jr'] - fr
        E = e_half * (Fraction(1, dl) + Fraction(1, dr)) + u * (2 * abs(fl) + abs(xl) + 2 * abs(fr) + abs(xr) + abs(x))
    elif plane == 'cog':
        g = Fraction(r['S1'], r['S0'])
        ref = g - x
        E = u * (abs(g) + abs(ref) + abs(x))
    else:
        E = u * abs(x)
    E *= SLACK
    return ulp32(abs(x) + E) + E


def profile_records(P, fit, half_width, shift=0):
    """measure() of every (slit row y, frame k) of the profiles P [n, ih, iw] (rotated-frame coordinates, sample scale):
    records[y][k], None for rows without a window."""
    n, ih, iw = P.shape
    out = []
    for y in range(ih):
        win = window(fit[y][0], shift, half_width, iw)
        if win is None:
            out.append(None)
            continue
        row = []
        for k in range(n):
            p = [int(v) for v in P[k, y]]
            r = measure(p, win[0], win[1], fit[y][3], shift)
            if r['width'] is not None:
                r['p_cross'] = (p[r['jl']], p[r['jl'] + 1], p[r['jr']], p[r['jr'] - 1])
            r['p'] = p
            row.append(r)
        out.append(row)
    return out


def within(got, records, plane, shift=0):
    """Check one computed plane float32 [ih, n] (frame columns in order) against the records: NaN exactly where the exact value
    is None, and |got - exact| <= bound() elsewhere.  Returns the largest |got - exact| / bound (0 when all are exact)."""
    worst = 0.0
    for y, row in enumerate(records):
        for k in range(got.shape[1]):
            g = float(got[y, k])
            x = None if row is None else row[k][plane]
            if x is None:
                assert math.isnan(g), '%s (%d, %d): %r where the exact value is NaN' % (plane, y, k, g)
                continue
            assert math.isfinite(g), '%s (%d, %d): %r where the exact value is %s' % (plane, y, k, g, float(x))
            err = abs(Fraction(g) - x)
            b = bound(row[k], plane, shift)
            assert err <= b, '%s (%d, %d): %r is %g from the exact %r, bound %g' % (plane, y, k, g, float(err), float(x), float(b))
            worst = max(worst, float(err / b))
    return worst
