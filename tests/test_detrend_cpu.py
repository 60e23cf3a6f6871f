"""The plane fit's host side without a GPU: linemaps.plane_from_moments against the restatement's own exact solve
(tests/detrend_ref.py) bit for bit, its rejections, the bound that keeps the ten sums inside int64, and the accuracy the
sigma-clipped fit reaches on the injected-field scan -- where detrend_ref.TOLERANCE comes from."""
import struct

import numpy as np
import pytest

from tests import detrend_ref as dr
from tests import linemaps_ref as ref
from tests.linemaps_util import IH, IW, N, fit_at


def bits(x):
    return struct.pack('<d', x)


def test_solve_equals_the_restatement_exactly():
    from solex_ser_recon_en_amd.linemaps import plane_from_moments
    rng = np.random.default_rng(5)
    maps = []
    for h, w in ((2, 2), (3, 5), (17, 9), (64, 64), (120, 77)):
        m = rng.normal(0.0, 0.8, (h, w)).astype(np.float32)
        if h * w > 8:
            m[rng.random((h, w)) < 0.05] = np.nan
        maps.append(m)
    maps.append((rng.normal(0.0, 20.0, (40, 50))).astype(np.float32))           # some beyond |v| < 64
    for m in maps:
        m10 = dr.plane_moments(m)
        got, want = plane_from_moments(m10), dr.solve(m10)
        assert [bits(v) for v in got[:4]] == [bits(v) for v in want[:4]] and got[4] == want[4] == m10[0], (got, want)
        assert got == plane_from_moments(np.asarray(m10, dtype=np.int64))       # the readback's array as well as a list
    # an exact plane of multiples of 1 / 4096: the coefficients come back exactly, sigma is 0
    r = np.arange(33, dtype=np.float64)[:, None]
    c = np.arange(47, dtype=np.float64)[None, :]
    a, b, g = -5325 / 4096, 37 / 4096, -12 / 4096
    m = (a + b * c + g * r).astype(np.float32)
    m[3, 4] = m[20, 30] = np.nan
    m10 = dr.plane_moments(m)
    assert plane_from_moments(m10) == (a, b, g, 0.0, 33 * 47 - 2) == dr.solve(m10)


def test_solve_rejections():
    from solex_ser_recon_en_amd.linemaps import plane_from_moments
    rng = np.random.default_rng(6)
    base = rng.normal(0.0, 0.8, (12, 12)).astype(np.float32)

    def only(mask):
        return dr.plane_moments(np.where(mask, base, np.float32(np.nan)))

    r, c = np.indices(base.shape)
    few = only((r == 2) & (c < 2) | (r == 7) & (c == 9))                        # three pixels, not on a line
    assert few[0] == 3
    for name, m10 in (('N < 4', few), ('one row', only(r == 5)), ('one column', only(c == 8)), ('diagonal', only(r == c)),
                      ('anti-diagonal', only(r + c == 11)), ('empty', only(r < 0))):
        with pytest.raises(ValueError):
            plane_from_moments(m10)
        with pytest.raises(ValueError):
            dr.solve(m10)
    four = only((r == 2) & (c < 3) | (r == 7) & (c == 9))                       # four pixels off a line: the smallest fit
    assert plane_from_moments(four)[4] == 4 and [bits(v) for v in plane_from_moments(four)[:4]] == [bits(v) for v in dr.solve(four)[:4]]


@pytest.mark.parametrize('q', [2 ** 18 - 1, 2 ** 18])
def test_the_ten_sums_stay_inside_int64(q):
    """At h = w = 8192 with every |q| at the limit (2^18 - 1, and the 2^18 the largest float32 below 64 rounds to), each of the ten
    sums, in Python ints, stays below 2^63 -- also when every term has the same sign."""
    h = w = dr.MAX_DIM
    for sums in (dr.closed_form_rows(h, w, q, q), dr.closed_form_rows(h, w, -q, -q), dr.closed_form_rows(h, w, q, -q)):
        assert len(sums) == 10 and all(abs(s) < 2 ** 63 for s in sums), sums
    assert dr.closed_form_rows(h, w, q, q)[9] == q * q * 2 ** 26 <= 2 ** 62
    # the closed forms themselves, against a pass over a small map
    m = np.empty((7, 5), dtype=np.float32)
    m[0::2], m[1::2] = 3.25, -1.5
    assert dr.closed_form_rows(7, 5, 13312, -6144) == dr.plane_moments(m)


@pytest.fixture(scope='module')
def truth():
    field = ref.injected_field(IH, N)
    ramp = 1.5 * (2.0 * np.arange(N, dtype=np.float64)[None, :] / (N - 1) - 1.0)
    return field, field - ramp, 3.0 / (N - 1)


@pytest.mark.parametrize('noise', sorted(dr.TOLERANCE['slope']))
def test_clipped_fit_recovers_the_ramp(truth, noise):
    """The sigma-clipped fit on the restated Dopplergram of the injected field: nearer the ramp's slope than the unclipped fit,
    within TOLERANCE['slope'], and the detrended map is the blob within TOLERANCE['residual'] (RMS on the disk)."""
    field, blob, slope = truth
    frames, centre, on = ref.doppler_scan(field, IW, noise, seed=3)
    m = ref.line_core_shift(frames, fit_at(centre), 5)
    m[~on] = np.nan
    out, _, info, trace = dr.detrend_plane(m)
    _, _, plain, _ = dr.detrend_plane(m, iterations=0)
    err, err_plain = abs(info['b'] - slope), abs(plain['b'] - slope)
    res = (out.astype(np.float64) - blob)[on]
    rms = float(np.sqrt(np.mean(res * res)))
    print('noise %g: |b - truth| %.4g clipped, %.4g unclipped; residual RMS %.5f px; %d of %d pixels used after %d passes'
          % (noise, err, err_plain, rms, info['n_used'], info['n_valid'], info['passes']))
    assert plain['passes'] == 1 and plain['n_used'] == plain['n_valid'] == info['n_valid'] == int(on.sum())
    assert info['passes'] == len(trace) == 4 and info['n_used'] < info['n_valid']
    assert err < err_plain
    assert err <= dr.TOLERANCE['slope'][noise]
    assert not np.isnan(res).any() and rms <= dr.TOLERANCE['residual'][noise]
    # the package's solve on the same moments: the same plane
    from solex_ser_recon_en_amd.linemaps import plane_from_moments
    assert plane_from_moments(trace[-1])[:3] == (info['a'], info['b'], info['g'])


def test_detrend_plane_rejects_bad_arguments():
    from solex_ser_recon_en_amd.linemaps import detrend_plane
    m = np.zeros((4, 4), dtype=np.float32)
    for kw in ({'clip': 0.0}, {'clip': -1.0}, {'clip': float('nan')}, {'clip': float('inf')}, {'iterations': -1}, {'iterations': 17},
               {'iterations': 1.5}):
        with pytest.raises(ValueError):
            detrend_plane(m, **kw)
