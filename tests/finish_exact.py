"""Exact restatement of shg_doppler_finish and shg_line_profile_finish (include/shg_hip.h), one output pixel at a time, written from
the header's comments, not from the kernel nor from linemaps_ref.py.

The float64 steps the header defines stay IEEE float64 steps (Python floats: no fused operations): x = (h00 c + h01 r) + h02,
t = x - floor(x), the blend (1 - t) L + t R, the mask's (c - cx)^2 + (r - cy)^2 > rad^2 and the display expression e.  Every
decision is also made exactly, with fractions.Fraction on those float64 values:
    which of the taps floor(x), ceil(x) lie in [0, w), whether x is whole (one tap or two), whether r < h,
    whether the exact (c - cx)^2 + (r - cy)^2 exceeds the exact rad^2 (flagged whenever the float64 compare decides otherwise:
    the header makes the float64 compare the rule, so the output follows it),
    which crop column maps to which source column, and whether e lies on a .5 tie or outside [1, 65535].
A decision the float64 arithmetic takes differently from the exact one is an assertion failure, except the mask's, which is
counted (class 'mask_disagree').

finish() returns the planes, the display planes and a Counter of the decision classes reached; within() holds a kernel's output
to it bit for bit (NaN positions included, NaN payloads not)."""
import math
from collections import Counter
from fractions import Fraction

import numpy as np

PLANES = ('shift', 'core', 'width', 'cog', 'ew')
F32_MIN_NORMAL = 2.0 ** -126


def display_scales(display_range, half_width):
    """(32767 / display_range, 65534 / (2 H + 1)) as the header writes them, each one float64 division (None where not given)."""
    s = None if display_range is None else 32767.0 / float(display_range)
    wd = None if half_width is None else 65534.0 / float(2 * int(half_width) + 1)
    return s, wd


def display_e(v, plane, shift_scale, width_scale):
    """The header's display expression e (float64) of the float32 value v for plane q (0 shift, 1 core, 2 width, 3 cog, 4 ew)."""
    v = float(v)
    if plane in (0, 3):
        return 32768.0 + v * shift_scale
    if plane == 1:
        return v
    return 1.0 + v * width_scale


def display_code(e, cls, plane='shift'):
    """clip(rint(e), 1, 65535) decided on the exact value of the float64 e; ties (up and down) and the clip recorded in cls under
    the plane's name."""
    if math.isinf(e):                                    # (an infinite value: clipped like any other)
        cls[plane + ('_above_65535' if e > 0 else '_below_1')] += 1
        return 65535 if e > 0 else 1
    E = Fraction(e)
    fl = math.floor(E)
    if E - fl == Fraction(1, 2):
        cls[plane + '_tie_up' if fl % 2 == 1 else plane + '_tie_down'] += 1
    q = round(E)                                         # Fraction.__round__: to nearest, ties to even (as rint)
    if q < 1:
        cls[plane + '_below_1'] += 1
        q = 1
    elif q > 65535:
        cls[plane + '_above_65535'] += 1
        q = 65535
    return q


def _tap_classes(x, X, x0, w, cls, left, right):
    whole = X.denominator == 1
    cls['x_whole' if whole else 'x_fraction'] += 1
    if x == 0.0 and math.copysign(1.0, x) < 0:
        cls['x_neg_zero'] += 1
    if -1 < X < 0:
        cls['x_in_minus1_0'] += 1
    if X == w - 1:
        cls['x_w_minus_1'] += 1
    if w - 1 < X < w:
        cls['x_in_last'] += 1
    if whole and 0 <= x0 < w:
        if left is not None and math.isnan(left):
            cls['whole_tap_nan'] += 1
        elif left is not None and math.isinf(left):
            cls['whole_tap_inf'] += 1
        if x0 + 1 < w and right is not None and math.isnan(right):
            cls['whole_right_neighbour_nan'] += 1


def finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, display_range=None, half_width=None):
    """raw float32 [P, h, w] (P = 1: shg_doppler_finish, 5: shg_line_profile_finish) -> (maps float32 [P, out_h, nw],
    png uint16 [P, out_h, nw] or None, Counter of the classes reached).  Plane q's display uses q's expression (P = 1: the shift's)."""
    raw = np.asarray(raw, dtype=np.float32)
    if raw.ndim == 2:
        raw = raw[None]
    P, h, w = raw.shape
    h00, h01, h02 = float(h00), float(h01), float(h02)
    cls = Counter()
    masked = circle is not None and not tuple(float(q) for q in circle) == (-1.0, -1.0, -1.0)
    cls['mask_none' if circle is None else ('mask_off' if not masked else 'mask_on')] += 1
    if masked:
        cx, cy, rad = (float(q) for q in circle)
        rr64, rr = rad * rad, Fraction(rad) ** 2
    nw, lo, dx0, n = (int(out_w), 0, 0, int(out_w)) if crop is None else (int(q) for q in crop)
    shift_scale, width_scale = display_scales(display_range, half_width)
    maps = np.full((P, out_h, nw), np.nan, dtype=np.float32)
    png = None if display_range is None else np.zeros((P, out_h, nw), dtype=np.uint16)
    rows = [[float(v) for v in raw[q, y]] for q in range(P) for y in range(h)]     # Python floats: exact float32 values
    for r in range(out_h):
        for oc in range(nw):
            i = oc - dx0
            if not 0 <= i < n:                               # the crop's padding
                cls['crop_pad'] += 1
                continue
            c = lo + i                                       # the source column, exactly
            if r >= h:
                cls['row_beyond_h'] += 1
                continue
            x = (h00 * float(c) + h01 * float(r)) + h02
            if masked:
                dx, dy = float(c) - cx, float(r) - cy
                d2 = dx * dx + dy * dy
                off = d2 > rr64
                exact = (Fraction(c) - Fraction(cx)) ** 2 + (Fraction(r) - Fraction(cy)) ** 2
                if d2 == rr64:
                    cls['mask_on_circle_f64'] += 1
                if (exact > rr) != off:
                    cls['mask_disagree'] += 1
                if exact != rr and abs(exact - rr) <= 4 * rr * Fraction(1, 2 ** 52):
                    cls['mask_just_out' if exact > rr else 'mask_just_in'] += 1
                if off:
                    cls['masked'] += 1
                    continue
            if not math.isfinite(x):
                cls['x_nan' if math.isnan(x) else 'x_inf'] += 1
                v = [math.nan] * P
            else:
                X = Fraction(x)
                x0, x1 = math.floor(X), math.ceil(X)
                t = x - float(math.floor(x))                 # (floor of a float is a float: exact)
                assert Fraction(t) == X - x0                 # x - floor(x) is exact in float64
                in0, in1 = 0 <= x0 < w, 0 <= x1 < w
                if abs(X) > 2 ** 62:
                    cls['x_far'] += 1
                if not (in0 and in1):
                    cls['tap_outside'] += 1
                if h00 == 0.0:
                    cls['h00_zero'] += 1
                v = []
                for q in range(P):
                    row = rows[q * h + r]
                    left = row[x0] if in0 else math.nan
                    right = row[x1] if in1 else math.nan
                    if q == 0:
                        _tap_classes(x, X, x0, w, cls, left, row[x0 + 1] if in0 and x0 + 1 < w else None)
                    v.append((1.0 - t) * left + t * right)
            for q in range(P):
                f = np.float32(v[q])                         # the header's (float) cast: round to nearest
                maps[q, r, oc] = f
                _value_classes(float(f), cls)
                if png is not None and not math.isnan(f):
                    png[q, r, oc] = display_code(display_e(f, q if P > 1 else 0, shift_scale, width_scale), cls, PLANES[q])
    return maps, png, cls


def _value_classes(f, cls):
    if math.isnan(f):
        cls['v_nan'] += 1
    elif math.isinf(f):
        cls['v_inf'] += 1
    elif f == 0.0:
        cls['v_neg_zero' if math.copysign(1.0, f) < 0 else 'v_pos_zero'] += 1
    elif abs(f) < F32_MIN_NORMAL:
        cls['v_denormal'] += 1
    else:
        cls['v_finite'] += 1


def classes(raw, *geometry, **kw):
    """The decision classes finish() reaches on one input (a Counter)."""
    return finish(raw, *geometry, **kw)[2]


def within(got, want, what=''):
    """got == want bit for bit: the same shape, NaN at the same positions and the same bits elsewhere (NaN payloads are not part
    of the contract).  Works for float32 planes and uint16 display planes; returns the number of values compared."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, '%s: shape %s, want %s' % (what, got.shape, want.shape)
    if want.dtype == np.uint16:
        bad = np.flatnonzero(got.astype(np.int64) != want.astype(np.int64))
        assert bad.size == 0, '%s: %d display codes differ, first at %s: %d vs %d' % (
            what, bad.size, np.unravel_index(bad[0], got.shape), got.flat[bad[0]], want.flat[bad[0]])
        return want.size
    got, want = got.astype(np.float32), want.astype(np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero(gn != wn)
    assert bad.size == 0, '%s: NaN positions differ at %d places, first at %s: %r vs %r' % (
        what, bad.size, np.unravel_index(bad[0], got.shape), got.flat[bad[0]], want.flat[bad[0]])
    g, w = got.view(np.uint32).copy(), want.view(np.uint32).copy()
    g[gn] = w[wn] = 0
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, '%s: %d values differ, first at %s: %r vs %r' % (
        what, bad.size, np.unravel_index(bad[0], got.shape), got.flat[bad[0]], want.flat[bad[0]])
    return want.size
