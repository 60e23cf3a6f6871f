"""The exact reference for shg_atlas_correlate (tests/spectral_exact.py) and the seeded adversarial configurations
(tests/spectral_adversarial.py) without a GPU: every class reached, the constructed scales exact, the run finder equal to
select() on the whole axis, np.corrcoef within its general bound of the exact correlation, NaN where the exact variance is 0,
np.argmax's NaN rule, and spectral.correlate's scale validation."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import spectral_adversarial as adv
from tests import spectral_exact as ex
from tests import spectral_ref as ref

ATLAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'alps.npz')


@pytest.fixture(scope='module')
def atlas():
    z = dict(np.load(ATLAS))
    z['a'] = ref.atlas_axis(z['first'], z['last'], z['step'])
    z['yv'] = z['y'] / 255
    return z


@pytest.fixture(scope='module')
def cases(atlas):
    return [(cfg, adv.records(cfg, atlas['a'], atlas['yv'])) for cfg in adv.configs(atlas['a'], atlas['y'])]


def test_every_class_is_reached(atlas, cases):
    counts = dict.fromkeys(adv.CLASSES, 0)
    for cfg, recs in cases:
        for k, v in adv.occurrences(cfg, recs, atlas['a']).items():
            counts[k] += v
    print('%d configurations, %d guesses: %s' % (len(cases), sum(len(c['scales']) for c, _ in cases),
                                                 ', '.join('%s %d' % kv for kv in counts.items())))
    missing = [c for c in adv.CLASSES if not counts[c]]
    assert not missing, 'classes never reached: %s' % missing
    assert {c['w'] for c, _ in cases} >= set(adv.SWEEP_W)


def test_constructed_scales_hit_exactly(atlas, cases):
    a = atlas['a']
    n_hits = 0
    for cfg, recs in cases:
        w = cfg['w']
        for g, k, target in cfg['hits']:
            s = cfg['scales'][g]
            assert ex.x_of(a[k], cfg['lam'], cfg['ax'], s) == target, (cfg['name'], g)
            k0, k1 = recs[g]['k0'], recs[g]['k1']
            if target == 0.0:
                assert k0 == k, (cfg['name'], g)                       # included
            elif target == w:
                assert k1 == k - 1, (cfg['name'], g)                   # excluded
            else:
                assert k0 <= k <= k1, (cfg['name'], g)
                if target > w - 1:
                    assert k1 == k
            n_hits += 1
    assert n_hits >= 4 * len(adv.SWEEP_W)
    # an anchor on an atlas point at an integer anchor_x: that point is on the pixel for every scale
    for cfg, recs in cases:
        if cfg['name'].startswith('anchor_point'):
            k = int(np.searchsorted(a, cfg['lam']))
            assert a[k] == cfg['lam'] and all(ex.x_of(a[k], cfg['lam'], cfg['ax'], s) == cfg['ax'] for s in cfg['scales'])


def test_run_finder_equals_select_run(atlas, cases):
    """On every adversarial guess of the small configurations and a stride of the rest: select() on the whole axis, and the
    reference's row on the whole axis is the bracketed slice's, bit for bit."""
    a, yv = atlas['a'], atlas['yv']
    checked = empty = 0
    for i, (cfg, recs) in enumerate(cases):
        guesses = cfg['special'] if (cfg['w'] <= 64 or not cfg['name'].startswith('sweep')) else cfg['special'][i % 3::3]
        for g in guesses:
            s, r = float(cfg['scales'][g]), recs[g]
            x = ex.x_of(a, cfg['lam'], cfg['ax'], s)
            if r['k0'] is None:
                assert not np.any((x >= 0) & (x < cfg['w']))
                with pytest.raises(ValueError):
                    ref.select_run(x, 0, cfg['w'])
                empty += 1
                continue
            assert ref.select_run(x, 0, cfg['w']) == (r['k0'], r['k1']), (cfg['name'], g)
            whole = ref.interp_row(a, yv, cfg['lam'], cfg['ax'], s, cfg['w'])
            assert np.array_equal(whole.view(np.uint64), r['row'].view(np.uint64)), (cfg['name'], g)
            checked += 1
    print('run finder: %d runs and %d empty runs equal to select() on the whole axis' % (checked, empty))
    assert checked >= 200 and empty >= 1


def test_run_finder_widens_a_bad_estimate(atlas):
    """The bracketing check, not the estimate, decides: a slice started far from the run is widened until it brackets."""
    a = atlas['a']
    lo, hi = ex.bracket(a[:2000], 3010.0, 5.0, 0.05, 100)
    x = ex.x_of(a[:2000], 3010.0, 5.0, 0.05)
    assert (lo == 0 or x[lo] < 0) and (hi == 2000 or x[hi - 1] >= 100)
    assert ex.run_ends(a, 3010.0, 5.0, 0.05, 100)[:2] == ref.select_run(ex.x_of(a, 3010.0, 5.0, 0.05), 0, 100)
    for s in (0.0, -0.05, math.nan, math.inf):
        with pytest.raises(ValueError):
            ex.run_ends(a, 3010.0, 5.0, s, 100)


def test_pearson_is_exact():
    """Small rows whose correlation is known in closed form, a scale change that must not move it, and NaN for a zero variance."""
    u = np.array([1.0, 2.0, 3.0, 4.0])
    assert ex.pearson(u, np.array([2.0, 4.0, 6.0, 8.0], np.float32)).value() == 1
    assert ex.pearson(u, np.array([8.0, 6.0, 4.0, 2.0], np.float32)).value() == -1
    c = ex.pearson(np.array([0.0, 1.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0, 1.0], np.float32))
    assert c.num == 0 and c.value() == 0
    c = ex.pearson(np.array([1.0, 2.0, 4.0]), np.array([1.0, 3.0, 2.0], np.float32))   # r = 1 / sqrt(14 / 3 * 2)
    assert c.value() > 0 and abs(c.value() ** 2 - Fraction(3, 28)) < Fraction(1, 2 ** 200)
    x = np.random.default_rng(1).random(300)
    v = np.random.default_rng(2).random(300).astype(np.float32)
    assert ex.pearson(x, v).same(ex.pearson(x * 2.0 ** -40 + 0.0, v)) and ex.pearson(x, v).same(ex.pearson(x * 4.0, v))
    assert ex.pearson(np.full(5, 0.7), v[:5]).nan and ex.pearson(x[:5], np.full(5, 3.0, np.float32)).nan


def test_corrcoef_within_the_general_bound(cases):
    worst, worst_kernel = 0.0, 0.0
    n = 0
    for cfg, recs in cases:
        for r in recs:
            if r['corr'] is None or r['corr'].nan:
                continue
            err = abs(Fraction(r['numpy']) - r['corr'].value())
            assert ex.within(r['numpy'], r['corr'], r['general']), (cfg['name'], float(err), r['general'])
            worst = max(worst, float(err) / r['general'])
            if not ex.nearly_constant(r['corr']):
                worst_kernel = max(worst_kernel, float(err) / r['bound'])
            n += 1
    print('np.corrcoef vs exact over %d rows: largest error %.3f of the general bound (%.3f of the kernel\'s)' % (n, worst, worst_kernel))


def test_the_bounds():
    """The kernel's bound is its summation's (about 1e-14 at W = 8192), not np.corrcoef's (about 1.8e-12)."""
    u = np.random.default_rng(5).random(8192)
    c = ex.pearson(u, np.random.default_rng(6).random(8192).astype(np.float32))
    assert ex.kernel_terms(8192) == 32 + 8 + 3 and ex.kernel_terms(256) == 12 and ex.kernel_terms(257) == 13
    assert 0.9e-14 < ex.kernel_bound(c) < 1.1e-14
    assert 1.7e-12 < ex.numpy_bound(c) < 1.9e-12
    assert ex.second_order(c) < 1e-22 and not ex.nearly_constant(c)


def test_nan_where_the_exact_variance_is_zero(cases):
    """np.corrcoef gives NaN only where the exact variance is 0.  The converse fails in one way only: a constant row with no
    window, whose float mean is not its value, is centred to a nonzero constant and gets a correlation of a few ulps."""
    nan = inexact = 0
    for cfg, recs in cases:
        for r in recs:
            if r['corr'] is None:
                assert math.isnan(r['numpy'])
                continue
            if math.isnan(r['numpy']):
                assert r['corr'].nan, cfg['name']
                nan += 1
            elif r['corr'].nan:
                u = r['row']
                lo, hi = ref.window(cfg['ax'], cfg['w']).indices(cfg['w'])[:2]
                assert np.all(u == u[0]) and hi <= lo and np.mean(u) != u[0], cfg['name']
                assert abs(r['numpy']) < 1e-12
                inexact += 1
    print('NaN rows: %d; constant rows with an inexact mean: %d' % (nan, inexact))
    assert nan >= 4 and inexact >= 1


def test_argmax_takes_the_first_nan(atlas):
    """The reference picks its dispersion with np.argmax, which returns the first NaN when there is one."""
    assert int(np.argmax(np.array([0.1, np.nan, 0.9, np.nan]))) == 1
    s2, ax, lam = adv.auto_nan_case(atlas['a'], atlas['y'])
    with np.errstate(invalid='ignore', divide='ignore'):
        corr, scales = ref.correlations(s2, ax, lam, atlas['first'], atlas['last'], atlas['step'], atlas['y'])
    nans = np.flatnonzero(np.isnan(corr))
    assert 0 < nans.size < corr.size
    assert int(np.argmax(corr)) == nans[0]


@pytest.mark.parametrize('bad', [0.0, -0.05, math.nan, math.inf, -math.inf])
def test_correlate_rejects_scales_that_are_not_finite_positive(bad):
    from solex_ser_recon_en_amd import spectral
    s2 = np.full(50, 1000, dtype=np.uint16)
    with pytest.raises(ValueError, match='guess 1'):
        spectral.correlate(s2, 25.0, 6562.808, spectral.load_atlas(ATLAS), np.array([0.05, bad, 0.06]), device='cpu')
