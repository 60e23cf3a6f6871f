"""Exact reference for shg_atlas_correlate (include/shg_hip.h), written for the tests from spectralAnalyserUI.py's definitions and
tests/spectral_ref.py, not from the kernel.

  run_ends()      the run [k0, k1] that select() keeps for any guess, found on a slice of the reference's own atlas axis that is
                  checked to bracket both ends (no closed form is trusted: the estimate only places the slice);
  row()           the reference's row (spectral_ref.interp_row, np.interp) fed that slice: the same bits as on the full axis;
  pearson()       the Pearson correlation of a float64 row and the float32 log spectrum in integer arithmetic, NaN when an
                  exact variance is 0;
  kernel_bound()  the kernel's error against pearson(), derived from its summation order;
  numpy_bound()   a looser bound that holds for np.corrcoef's sums in any order.

The bounds.  Write u for the unit roundoff 2^-53 and g(n) = n u / (1 - n u).  Both computations centre the rows by rounded means
mu' = mu + du and nu' = nu + dv, form S_ab = sum (a_i - mu')(b_i - nu') with a few roundings per term, and finish with
c = (S_uv f) / sqrt(S_uu f) / sqrt(S_vv f), whose f = 1 / (W - 1) cancels in exact arithmetic.  Each centred product carries the
two centring roundings and the product's own (3), then the roundings of the sum it goes through: in the kernel ceil(W / 256)
serial additions in a thread, 6 levels of the 64-lane DPP fold and 2 of the four-wave combine, so k = ceil(W / 256) + 11; in
np.corrcoef the BLAS dot may add in any order, so k = W + 2.  By Cauchy-Schwarz, sum |a_i b_i| <= sqrt(S'_uu S'_vv), so the sums
move the correlation of the centred rows by at most 2 g(k) / (1 - g(k)).  The finish adds g(6) (two products, two square roots
that halve their argument's error and add their own, two divisions).  Centring by mu' instead of mu changes the correlation by at
most A + B, A = W du^2 / S_uu and B = W dv^2 / S_vv, S_uu and S_vv the exact centred sums of squares, and any summation order
gives |du| <= g(W + 1) sum |u_i| / W.  That term is second order unless a row is nearly constant (its spread a few ulps of its
mean), which is why the tests treat such rows as their own class.  bound = (2 g(k) / (1 - g(k)) + g(6) + A + B) (1 + 1e-4).  At
W = 8192 the kernel's bound is 1.0e-14 for rows that are not nearly constant; np.corrcoef's is 1.8e-12."""
import math
from fractions import Fraction
from operator import mul

import numpy as np

from tests import spectral_ref

U = 2.0 ** -53
SLACK = 1.0001            # covers the products of two or more rounding errors
THREADS = 256             # the kernel's workgroup: the threads' serial sums
FOLD_LEVELS = 6 + 2       # the 64-lane DPP fold, then the four waves' partials
DIGITS = 256              # pearson()'s value: its error is below 2^-DIGITS


def gamma(n):
    return n * U / (1.0 - n * U)


def kernel_terms(w):
    """k of the kernel's sums: ceil(W / 256) serial additions per thread, the fold's levels, and the three roundings of a term."""
    return -(-w // THREADS) + FOLD_LEVELS + 3


# ---- the run select() keeps ------------------------------------------------------------------------------------------------
def x_of(a, anchor_wavelength, anchor_x, scale):
    """The reference's pixel position of atlas points a (:279): ((a - lambda_a) / s) + anchor_x, elementwise in float64."""
    return (a - anchor_wavelength) / scale + anchor_x


def bracket(a, anchor_wavelength, anchor_x, scale, w, pad=16):
    """(lo, hi) with a[lo:hi] holding the whole run of points with 0 <= x < w, checked rather than trusted: x rises with k (s > 0),
    and the slice starts at 0 or at a point with x < 0, and ends at the last point or at one with x >= w.  The closed-form
    estimate only places the first try; the slice is widened until the check holds."""
    n = a.shape[0]
    first, d = float(a[0]), float(a[1] - a[0]) if n > 1 else 1.0
    e = [(anchor_wavelength + (p - anchor_x) * scale - first) / d for p in (0.0, float(w))]
    e = [min(max(v, 0.0), n - 1.0) if math.isfinite(v) else 0.0 for v in e]
    lo, hi = int(min(e)), int(max(e)) + 1
    while True:
        lo, hi = max(lo - pad, 0), min(hi + pad, n)
        x = x_of(a[[lo, hi - 1]], anchor_wavelength, anchor_x, scale)
        if (lo == 0 or x[0] < 0.0) and (hi == n or x[1] >= w):
            return lo, hi
        pad *= 4


def run_ends(a, anchor_wavelength, anchor_x, scale, w):
    """-> (k0, k1, lo, hi): select()'s run [k0, k1] on the full axis a (None, None when it is empty) and the bracketing slice."""
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError('the run is defined for finite positive scales, not %r' % scale)
    lo, hi = bracket(a, anchor_wavelength, anchor_x, scale, w)
    x = x_of(a[lo:hi], anchor_wavelength, anchor_x, scale)
    assert np.all(np.diff(x) >= 0.0)
    inside = np.flatnonzero((x >= 0.0) & (x < w))
    if inside.size == 0:
        return None, None, lo, hi
    k0, k1 = lo + int(inside[0]), lo + int(inside[-1])
    assert k1 - k0 + 1 == inside.size          # contiguous, as x rises
    return k0, k1, lo, hi


def row(a, yv, anchor_wavelength, anchor_x, scale, w, lo, hi):
    """spectral_ref.interp_row (np.interp, the window set to np.mean) on the bracketing slice a[lo:hi] (the same bits as on the
    whole axis: every step is elementwise or confined to the run)."""
    return spectral_ref.interp_row(a[lo:hi], yv[lo:hi], anchor_wavelength, anchor_x, scale, w)


# ---- the exact correlation --------------------------------------------------------------------------------------------------
def _ints(x):
    """x (float64, finite) -> (ints I, E) with x_i = I_i 2^-E exactly."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.isfinite(x))
    nz = x[x != 0.0]
    if nz.size == 0:
        return [0] * x.shape[0], 0
    _, e = np.frexp(nz)
    shift = 53 - int(e.min())
    scaled = np.ldexp(x, shift)
    assert np.all(np.isfinite(scaled))
    ints = list(map(int, scaled))
    assert np.array_equal(np.ldexp(np.array(ints, dtype=np.float64), -shift), x)
    return ints, shift


class Series:
    """A row's exact sums: n, S = sum x_i and Q = n sum x_i^2 - S^2 (n^2 times the variance), in units of 2^-E."""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        self.n = self.x.shape[0]
        self.ints, self.e = _ints(self.x)
        self.s = sum(self.ints)
        self.q = self.n * sum(map(mul, self.ints, self.ints)) - self.s * self.s
        self.abs_sum = Fraction(sum(abs(i) for i in self.ints), 1 << self.e)

    def centred_sq(self):
        """Sum (x_i - mean)^2 as a Fraction."""
        return Fraction(self.q, self.n * (1 << (2 * self.e)))


class Corr:
    """The exact Pearson correlation num / sqrt(qu qv) of two Series; nan when qu or qv is 0."""

    def __init__(self, su, sv):
        assert su.n == sv.n
        self.su, self.sv = su, sv
        self.num = su.n * sum(map(mul, su.ints, sv.ints)) - su.s * sv.s
        self.nan = su.q == 0 or sv.q == 0

    def value(self):
        """A Fraction within 2^-DIGITS of the correlation (None for nan)."""
        if self.nan:
            return None
        root = math.isqrt((self.su.q * self.sv.q) << (2 * DIGITS))
        return Fraction(self.num << DIGITS, root) if root else None

    def __float__(self):
        v = self.value()
        return math.nan if v is None else float(v)

    def same(self, other):
        """Exactly equal correlations (both nan counts as equal)."""
        if self.nan or other.nan:
            return self.nan and other.nan
        if (self.num > 0) != (other.num > 0) or (self.num < 0) != (other.num < 0):
            return False
        return self.num ** 2 * other.su.q * other.sv.q == other.num ** 2 * self.su.q * self.sv.q


def pearson(u, v):
    """Exact correlation of a float64 row u and the float32 log spectrum v (a Series may be passed for v to reuse its sums)."""
    sv = v if isinstance(v, Series) else Series(np.asarray(v, dtype=np.float64))
    return Corr(Series(u), sv)


def second_order(c):
    """A + B of the module's derivation: the most centring by rounded means can move the correlation (inf for a constant row)."""
    w = c.su.n
    out = 0.0
    for s in (c.su, c.sv):
        sq = s.centred_sq()
        if sq == 0:
            return math.inf
        dmean = Fraction(gamma(w + 1)) * s.abs_sum / w
        out += float(w * dmean * dmean / sq)
    return out


def kernel_bound(c):
    """The kernel's error bound against the exact correlation c (a Corr)."""
    k = kernel_terms(c.su.n)
    return (2.0 * gamma(k) / (1.0 - gamma(k)) + gamma(6) + second_order(c)) * SLACK


def numpy_bound(c):
    """np.corrcoef's error bound against c: its dot may sum in any order."""
    k = c.su.n + 2
    return (2.0 * gamma(k) / (1.0 - gamma(k)) + gamma(6) + second_order(c)) * SLACK


def nearly_constant(c):
    """The second-order term dominates the kernel's bound: one row's spread is a few ulps of its mean."""
    return second_order(c) > gamma(kernel_terms(c.su.n))


def within(got, c, bound):
    """|got - c| <= bound, in exact arithmetic (got a float, c a non-nan Corr)."""
    return math.isfinite(got) and abs(Fraction(got) - c.value()) <= Fraction(bound)
