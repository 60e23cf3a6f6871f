"""Seeded adversarial line profiles for the line maps (shg_line_core_shift, shg_line_profile, shg_line_bisector): P[k, y, j] in the
rotated frame's coordinates (sample scale: 8-bit samples are multiples of 256), one class per slit row, windows placed by a fit
whose rows also cover the window's own edge cases.  to_file() gives the raw file layout; occurrences() counts, on linemaps_exact's
records, which of the decisions each class exists for were actually reached.

level_profiles() adds rows for the bisector's level decisions on top of these (which already hold unbracketed minima, C2 = 0,
emission lines with C2 / 2 <= core, ties and window edges): a sample at ceil(level) or ceil(level) - 1 beside the core, integral
levels, p(j*) equal to the level, and crossings on the window's edges."""
import math

import numpy as np

from tests import linemaps_exact as ex

CLASSES = ('noise', 'plateau', 'monotone', 'constant', 'halfhit', 'nowidth', 'emission', 'maxsum', 'nearedge')
# the window's edge cases, taken in turn by the fit rows of every other cycle of classes
FIT_KINDS = ('integer', 'trunc', 'clamp_hi', 'clamp_lo', 'huge', 'nan', 'inf', '-huge', '-inf', 'edge_lo', 'edge_hi')
# (a - b, e - b) with d^2 / (8 den) a multiple of 1/2: the half level can then be an exact integer
HALF_PAIRS = ((1, 1), (2, 2), (3, 3), (5, 5), (4, 0), (8, 0), (12, 4), (4, 4))


def _fit(rng, ih, iw, half_width, shift):
    """fit [ih, 4]: column 0 the line, column 3 the reference position (finite).  Rows of every other cycle of classes take the
    FIT_KINDS in turn; the rest get a line whose window at S lies inside the frame.  At S != 0 those lines lie where a scan's
    would: in [0, iw), so that near S's extremes only the lines at the frame's far edge keep a window."""
    fit = np.zeros((ih, 4))
    ncl = len(CLASSES)
    special = 0
    for y in range(ih):
        cc = int(rng.integers(1 + half_width, max(iw - 1 - half_width, 2 + half_width)))     # a window inside the frame
        f0 = cc - shift + float(rng.random())
        if shift != 0:
            f0 = float(np.clip(f0, 0.0, iw - 1e-6)) if abs(shift) < iw // 2 else (
                float(rng.uniform(-0.99, 1.0)) if shift > 0 else iw - 1.0 + float(rng.uniform(0.0, 1.99)))
        if (y // ncl) % 2 == 1:
            kind = FIT_KINDS[special % len(FIT_KINDS)]
            special += 1
            f0 = {'integer': float(math.floor(f0)), 'trunc': -float(rng.uniform(0.01, 0.99)) - shift,
                  'clamp_hi': 2.0 ** 30 + 5.5 - shift, 'clamp_lo': -2.0 ** 30 - 7.5 - shift, 'huge': 1e300, '-huge': -1e300,
                  'nan': math.nan, 'inf': math.inf, '-inf': -math.inf,
                  'edge_lo': 2.0 - shift + float(rng.random()), 'edge_hi': iw - 3.0 - shift + float(rng.random())}[kind]
        fit[y] = (f0, 0.0, y, f0 + float(rng.uniform(-0.75, 0.75)) if math.isfinite(f0) else cc + 0.25)
    return fit


def _row(cls, k, rng, Q, iw, lo, hi, pair_seed):
    """One profile (ints 0..Q, length iw) of class cls for frame k and window [lo, hi]; samples outside the window are noise."""
    p = rng.integers(0, Q + 1, iw)
    m = hi - lo + 1
    w = np.arange(lo, hi + 1)
    if cls == 'noise':
        if k % 3 == 0:
            i, j = rng.choice(m, 2, replace=False)
            p[lo + i], p[lo + j] = 0, Q
    elif cls == 'plateau':
        sub, L = k % 4, min(2 + (k // 4) % 3, m - 1)
        p[w] = rng.integers(Q // 2, Q + 1, m)
        start = (lo, lo + 1, int(rng.integers(lo + 1, hi - L + 2)), hi - L + 1)[sub]
        start = min(start, hi - L + 1)
        p[start:start + L] = rng.integers(0, Q // 2)
    elif cls == 'monotone':
        v = np.sort(rng.choice(Q + 1, m, replace=k % 4 >= 2))
        p[w] = v if k % 2 == 0 else v[::-1]
    elif cls == 'constant':
        p[w] = 0 if k % 2 == 0 else Q
    elif cls == 'halfhit':
        return _halfhit(k, pair_seed, Q, p, lo, hi)
    elif cls == 'nowidth':
        sub = k % 5
        if sub <= 1 and m >= 4:              # b >= half: p(lo) = b + 1, a = b + 4 (half = b) or b + 8 (half = b - 1/4), e = p(hi) = b
            b = int(rng.integers(0, Q - 8))
            js = int(rng.integers(lo + 2, hi))
            p[w] = rng.integers(b + 1, Q + 1, m)
            p[js + 1:hi + 1] = rng.integers(b, Q + 1, hi - js)
            p[lo], p[js - 1], p[js], p[js + 1], p[hi] = b + 1, b + (4 if sub == 0 else 8), b, b, b
        elif sub <= 3:                       # negative core: a = Q, b = e = 0; crossings on the left only, or on both sides
            js = lo + 1 if sub == 2 else int(rng.integers(lo + 1, hi))
            p[w] = 0
            p[lo:js] = Q
            if sub == 3:
                p[hi] = Q
        else:                                # a crossing on the right only: everything left of the core below the half level
            p[w] = 0
            p[lo], p[hi] = 1, Q
            p[hi - 1] = Q
            p[lo + 1:hi - 1] = rng.integers(1, 3, m - 3)
            p[hi - 2] = 0
    elif cls == 'emission':
        p[w] = rng.integers(Q // 2, Q + 1, m)
        p[lo], p[hi] = rng.integers(1, Q // 4 + 1, 2)
    elif cls == 'maxsum':
        p[w] = Q
        if k % 2:
            p[int(rng.integers(lo + 1, hi))] = 0
    elif cls == 'nearedge':
        p[w] = rng.integers(Q // 2, Q + 1, m)
        p[lo + 1 if k % 2 == 0 else hi - 1] = rng.integers(0, Q // 2)
    return p


def _halfhit(k, pair_seed, Q, p, lo, hi):
    """A crossing sample exactly at an integer half level, left (even k // 2) or right of the core; odd k: the same profile as
    k - 1 (the same pair_seed) with that sample one below."""
    pair = np.random.default_rng(pair_seed)
    left = (k // 2) % 2 == 0
    if hi - lo < 4:
        return p
    for _ in range(200):
        g = np.random.default_rng(pair.integers(1 << 30))
        q = g.integers(0, Q + 1, len(p))
        alpha, eps = HALF_PAIRS[int(g.integers(len(HALF_PAIRS)))]
        js = int(g.integers(lo + 3, hi)) if left else int(g.integers(lo + 1, hi - 2))
        b = int(g.integers(0, max(Q // 3, 1)))
        d, den = alpha - eps, alpha + eps
        h = int(g.integers(b + max(alpha, eps) + 2, b + max(alpha, eps) + 2 + max(Q // 8, 4)))
        c2 = 4 * h - 2 * b + d * d // (4 * den)             # C2 / 4 + b / 2 - d^2 / (16 den) = h
        plo, phi = c2 // 2, c2 - c2 // 2
        if phi > Q or plo > Q:
            continue
        q[lo:hi + 1] = g.integers(b + 1, Q + 1, hi - lo + 1)
        q[lo], q[hi] = plo, phi
        q[js - 1], q[js], q[js + 1] = b + alpha, b, b + eps
        jc = int(g.integers(lo + 1, js - 1)) if left else int(g.integers(js + 2, hi))
        between = range(jc + 1, js - 1) if left else range(js + 2, jc)
        for j in between:
            q[j] = g.integers(b + 1, h)
        q[jc] = h
        r = ex.measure([int(v) for v in q], lo, hi, 0.0)
        if r['half'] != h or not r['has_width'] or (r['jl'] if left else r['jr']) != jc:
            continue
        if k % 2:
            q[jc] -= 1
        return q
    return p


def profiles(n, ih, iw, bits, half_width, shift=0, seed=0):
    """(P int64 [n, ih, iw] on the sample scale, fit [ih, 4], classes [ih]) for line_profile at `shift` (S = 0: line_core_shift)."""
    rng = np.random.default_rng([seed, n, ih, iw, bits, half_width, shift + 1000])
    Q = 65535 if bits == 16 else 255
    fit = _fit(rng, ih, iw, half_width, shift)
    cls = [CLASSES[y % len(CLASSES)] for y in range(ih)]
    P = rng.integers(0, Q + 1, (n, ih, iw))
    for y in range(ih):
        win = ex.window(fit[y, 0], shift, half_width, iw)
        if win is None:
            continue
        for k in range(n):
            P[k, y] = _row(cls[y], k, rng, Q, iw, *win, pair_seed=[seed, y, k // 2])
    return P * (256 if bits == 8 else 1), fit, cls


def to_file(P, bits, rotate):
    """Raw frames in file layout.  ih >= iw either way: a rotated file (width = ih > height = iw) inverts a1,
    raw[k, j, W - 1 - y] = P[k, y, j]; a plain file (height = ih >= width = iw) is P itself."""
    q = P // 256 if bits == 8 else P
    raw = np.ascontiguousarray(q[:, ::-1, :].transpose(0, 2, 1)) if rotate else q
    return raw.astype(np.uint8 if bits == 8 else np.uint16)


def occurrences(records, cls, fit, bits, shift=0):
    """How often each decision was reached, counted on linemaps_exact's records (and fit kinds on the fit)."""
    top, one = (65535, 1) if bits == 16 else (255 * 256, 256)       # the largest sample, and one raw step on the sample scale
    c = {}

    def add(name, ok=True):
        c[name] = c.get(name, 0) + int(bool(ok))

    for y, row in enumerate(records):
        for name in ('nan', 'inf', 'clamp'):
            add('fit_' + name, False)
        f0 = fit[y, 0]
        add('fit_nan', np.isnan(f0))
        add('fit_inf', np.isinf(f0))
        add('fit_clamp', np.isfinite(f0) and abs(f0 + shift) > ex.CLAMP)
        if row is None:
            continue
        add('fit_integer', f0 == np.floor(f0))
        add('fit_trunc', -1 < f0 + shift < 0)
        for r in row:
            p, lo, hi, js = r['p'], r['lo'], r['hi'], r['jstar']
            win = p[lo:hi + 1]
            best = min(win)
            ties = [j for j in range(lo, hi + 1) if p[j] == best]
            ok = r['jl'] is not None, r['jr'] is not None
            if cls[y] == 'noise':
                add('noise_0', 0 in win)
                add('noise_max', top in win)
            if len(ties) >= 2 and all(ties[i + 1] == ties[i] + 1 for i in range(len(ties) - 1)):
                add('plateau_lo', ties[0] == lo)
                add('plateau_lo1', ties[0] == lo + 1)
                add('plateau_inside', lo + 1 < ties[0] and ties[-1] < hi)
                add('plateau_hi', ties[-1] == hi)
            if len(set(win)) > 1:
                add('mono_up', all(win[i] < win[i + 1] for i in range(len(win) - 1)))
                add('mono_down', all(win[i] > win[i + 1] for i in range(len(win) - 1)))
            add('const_0', r['C2'] == 0 and r['S0'] == 0)
            add('const_max', all(v == top for v in win))
            add('maxsum', len(win) == 65 and all(v == top for v in win))
            add('emission', r['S0'] <= 0 and r['C2'] > 0)
            add('near_lo1', js == lo + 1)
            add('near_hi1', js == hi - 1)
            if r['half'] is None:
                continue
            h = r['half']
            add('core_neg', r['core'] < 0)
            add('best_ge_half', not r['has_width'])
            add('best_eq_half', r['b'] == h)
            if not r['has_width']:
                continue
            add('one_side', ok[0] != ok[1])
            if h.denominator == 1:
                add('half_left', ok[0] and p[r['jl']] == h)
                add('half_right', ok[1] and p[r['jr']] == h)
                add('half_minus1', any(p[j] == h - one for j in range(lo + 1, hi) if j != js))
    return c


# what every layout with windows of at least 5 samples (H >= 5, S = 0) must reach; maxsum needs H = 32
REQUIRED = ('noise_0', 'noise_max', 'plateau_lo', 'plateau_lo1', 'plateau_inside', 'plateau_hi', 'mono_up', 'mono_down',
            'const_0', 'const_max', 'emission', 'near_lo1', 'near_hi1', 'core_neg', 'best_ge_half', 'best_eq_half', 'one_side',
            'half_left', 'half_right', 'half_minus1', 'fit_nan', 'fit_inf', 'fit_clamp', 'fit_integer', 'fit_trunc')


# ---- rows for the bisector's levels ----
# the level sets the tests run: one level, the usual four, dyadic levels (integral levels need them), and eight reaching near 0 and 1
LEVEL_SETS = ((0.5,), (0.2, 0.4, 0.6, 0.8), (0.25, 0.5, 0.75), (1e-6, 0.1, 0.3, 0.45, 0.55, 0.7, 0.9, 1.0 - 1e-6))
LEVEL_KINDS = ('hit_left', 'hit_right', 'integral', 'best_eq', 'edges')


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
        c = math.ceil(ex.level64(levels[(k + t) % len(levels)], core, plo + phi))
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


def level_profiles(n, ih, iw, bits, half_width, levels, shift=0, seed=0):
    """(P int64 [n, ih, iw] on the sample scale, fit [ih, 4], classes [ih]): profiles()' rows, every third slit row (with a
    window wide enough) replaced by a level class."""
    P, fit, cls = profiles(n, ih, iw, bits, half_width, shift, seed)
    rng = np.random.default_rng([seed, n, ih, iw, bits, half_width, shift + 1000, len(levels), 7])
    Q, scale = (65535, 1) if bits == 16 else (255, 256)
    cls = list(cls)
    for y in range(2, ih, 3):
        win = ex.window(fit[y, 0], shift, half_width, iw)
        if win is None:
            continue
        kind = LEVEL_KINDS[(y // 3) % len(LEVEL_KINDS)]
        rows = [_level_row(kind, k, rng, Q, iw, *win, levels) for k in range(n)]
        if any(r is None for r in rows):
            continue
        P[:, y] = np.stack(rows) * scale
        cls[y] = kind
    return P, fit, cls
