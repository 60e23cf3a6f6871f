"""Exact restatement of shg_line_core_shift, shg_line_profile and shg_line_bisector (include/shg_hip.h), one (slit row, frame) at a
time, in Python int and fractions.Fraction: every value is the mathematical one the header's formulas define, with no rounding
anywhere, or None where the header says NaN.  Written from the header, not from the kernels nor from tests/linemaps_ref.py.

The one float64 operation kept is the header's window: c = (int64)(fit[y][0] + (double)S), where the sum is itself part of the
definition.  ref = Fraction(fit[y][3]) + S.  The width is the chord at the exact half = C2/4 + b/2 - d^2/(16 den), and the
level of fraction f is the exact (1 - f) core + f C2 / 2 with f the exact value of the float64 fraction; one crossing walk takes
both.  (The half's decisions in integers, den > 0: p >= half <=> 16 den p >= 4 den C2 + 8 den b - d^2, and b < half <=>
8 den b < 4 den C2 - d^2.)

bound() and level_bound() turn the header's sequence of IEEE operations into a tolerance for each computed value; within() checks a
plane against the records."""
import math
from fractions import Fraction

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


def cross(p, lo, hi, jstar, b, level, ref):
    """The crossings of p at an exact level: has (b < level), jl, jr, and where both exist the chord, the bisector (None without
    ref) and the samples either side of the crossings."""
    L = dict(level=level, has=False, jl=None, jr=None, chord=None, bis=None, p_cross=None)
    if not b < level:
        return L
    left = [j for j in range(lo, jstar) if p[j] >= level]
    right = [j for j in range(jstar + 1, hi + 1) if p[j] >= level]
    L.update(has=True, jl=left[-1] if left else None, jr=right[0] if right else None)
    if left and right:
        jl, jr = left[-1], right[0]
        xl = jl + (p[jl] - level) / (p[jl] - p[jl + 1])
        xr = jr - (p[jr] - level) / (p[jr] - p[jr - 1])
        L.update(chord=xr - xl, p_cross=(p[jl], p[jl + 1], p[jr], p[jr - 1]))
        if ref is not None:
            L['bis'] = (xl + xr) / 2 - ref
    return L


def measure(p, lo, hi, f3, shift=0, levels=()):
    """Every intermediate and the exact values of one profile p (a sequence of Python ints) over [lo, hi]: a dict with p, lo, hi,
    jstar, a, b, e, den, d, C2, S0, S1, half (None without a vertex), has_width, jl, jr, p_cross, the PLANES shift, core, width,
    cog, ew (Fraction or None) and, per level, cross()'s dict with f (all None without a vertex)."""
    p = [int(v) for v in p]
    f3 = float(f3)
    ref = Fraction(f3) + shift if math.isfinite(f3) else None      # (NaN propagates: no finite shift, cog or bisector)
    r = dict(p=p, lo=lo, hi=hi, jstar=None, a=None, b=None, e=None, den=None, d=None, half=None, has_width=False, jl=None,
             jr=None, p_cross=None, shift=None, core=None, width=None, cog=None, ew=None)
    js = range(lo, hi + 1)
    C2 = p[lo] + p[hi]
    S0 = len(js) * C2 - 2 * sum(p[j] for j in js)
    S1 = C2 * sum(js) - 2 * sum(j * p[j] for j in js)
    r.update(C2=C2, S0=S0, S1=S1)
    if S0 > 0 and ref is not None:
        r['cog'] = Fraction(S1, S0) - ref
    if C2 != 0:
        r['ew'] = Fraction(S0, C2)
    best = min(p[j] for j in js)
    jstar = next(j for j in js if p[j] == best)                  # the first minimum
    r['jstar'] = jstar
    r['levels'] = [dict(f=f, level=None, has=False, jl=None, jr=None, bis=None, chord=None, p_cross=None) for f in levels]
    if jstar == lo or jstar == hi:
        return r
    a, b, e = p[jstar - 1], p[jstar], p[jstar + 1]
    den, d = a + e - 2 * b, a - e
    assert den > 0                                               # a > b (first minimum), e >= b
    r.update(a=a, b=b, e=e, den=den, d=d, core=b - Fraction(d * d, 8 * den))
    if ref is not None:
        r['shift'] = jstar + Fraction(d, 2 * den) - ref
    r['half'] = Fraction(C2, 4) + Fraction(b, 2) - Fraction(d * d, 16 * den)
    h = cross(p, lo, hi, jstar, b, r['half'], ref)
    r.update(has_width=h['has'], jl=h['jl'], jr=h['jr'], width=h['chord'], p_cross=h['p_cross'])
    for L in r['levels']:
        F = Fraction(L['f'])
        L.update(cross(p, lo, hi, jstar, b, (1 - F) * r['core'] + F * Fraction(C2, 2), ref))
    return r


def records(P, fit, half_width, shift=0, levels=()):
    """measure() of every (slit row y, frame k) of the profiles P [n, ih, iw] (rotated-frame coordinates, sample scale):
    records[y][k], None for rows without a window."""
    n, ih, iw = P.shape
    out = []
    for y in range(ih):
        win = window(fit[y][0], shift, half_width, iw)
        out.append(None if win is None else [measure(P[k, y], win[0], win[1], fit[y][3], shift, levels) for k in range(n)])
    return out


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


def level_bound(r, L, plane):
    """The largest |computed - exact| the header's operations allow for one level's bisector or chord (as bound()):
      core: E_c = u (q + |core|), q = d^2 / (8 den)
      level: t = 1 - f (u |1 - f|), t core_d, f (0.5 C2), their sum:  E_l = |1 - f| E_c + 2 u |1 - f| |core| + u |f C2 / 2| + u |level|
      xl = jl + (p(jl) - level) / Dl:  E_xl = (E_l + u |p(jl) - level|) / Dl + u |fl| + u |xl|, the same on the right
      chord = xr - xl:  E_xl + E_xr + u |chord|
      bis = 0.5 (xl + xr) - ref:  E_xl + E_xr + u |xl + xr| + u (|mid| + |ref| + |bis|)   (0.5 x exact; ref = f3 + S: u |ref|)
    Every E times SLACK, plus one float32 ulp of |exact| + E for the final cast."""
    u = U64
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
    return ulp32(abs(x) + E) + E


def level64(f, core_d, c2):
    """The header's float64 level: ((1.0 - f) * core_d) + (f * (0.5 * (double)C2))."""
    return ((1.0 - f) * core_d) + (f * (0.5 * float(c2)))


def level_decisions(r):
    """Per level with a vertex: (exact decisions, float64 decisions) of b < level and of p(j) >= level over the window; the float64
    ones also through ceil(level) for integer p, as the kernel takes them."""
    out = []
    for L in r['levels']:
        if L['level'] is None:
            continue
        lv = level64(L['f'], float(r['b']) - float(r['d'] * r['d']) / (8.0 * float(r['den'])), r['C2'])
        p = r['p'][r['lo']:r['hi'] + 1]
        exact = (r['b'] < L['level'],) + tuple(v >= L['level'] for v in p)
        f64 = (float(r['b']) < lv,) + tuple(v >= lv for v in p)
        thr = (float(r['b']) < lv,) + tuple(v >= math.ceil(lv) for v in p)
        out.append((exact, f64, thr, L))
    return out


def plane(name, shift=0):
    """within()'s (value, bound) for a PLANES plane."""
    return (lambda r: r[name]), (lambda r: bound(r, name, shift))


def level(i, name):
    """within()'s (value, bound) for level i's 'bis' or 'chord'."""
    return (lambda r: r['levels'][i][name]), (lambda r: level_bound(r, r['levels'][i], name))


def within(got, records, value, bound, skip=()):
    """Check one computed plane float32 [ih, n] (frame columns in order) against the records: NaN exactly where value(record) is
    None, and |got - exact| <= bound(record) elsewhere; (y, k) in `skip` are left out.  Returns the largest |got - exact| / bound
    (0 when all are exact)."""
    worst = 0.0
    for y, row in enumerate(records):
        for k in range(got.shape[1]):
            if (y, k) in skip:
                continue
            g = float(got[y, k])
            x = None if row is None else value(row[k])
            if x is None:
                assert math.isnan(g), '(%d, %d): %r where the exact value is NaN' % (y, k, g)
                continue
            assert math.isfinite(g), '(%d, %d): %r where the exact value is %s' % (y, k, g, float(x))
            err = abs(Fraction(g) - x)
            b = bound(row[k])
            assert err <= b, '(%d, %d): %r is %g from the exact %r, bound %g' % (y, k, g, float(err), float(x), float(b))
            worst = max(worst, float(err / b))
    return worst
