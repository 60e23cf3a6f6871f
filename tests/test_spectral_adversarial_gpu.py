"""shg_atlas_correlate on the seeded adversarial configurations (tests/spectral_adversarial.py), called through ops so that the run
is visible: every guess's run equal to select()'s, rows bit for bit np.interp's with the fill, the correlation within the derived
bound of the exact one (tests/spectral_exact.py), NaN exactly where np.corrcoef's is, the argmax the exact maximiser, and no
guess leaking into another."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import spectral_adversarial as adv
from tests import spectral_exact as ex
from tests import spectral_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ATLAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'alps.npz')
ROWS_ALL_W = 600          # every guess's row up to this W; above it a stride and every adversarial guess


@pytest.fixture(scope='module')
def spectral():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import spectral
    return spectral


@pytest.fixture(scope='module')
def atlas():
    z = dict(np.load(ATLAS))
    z['a'] = ref.atlas_axis(z['first'], z['last'], z['step'])
    z['yv'] = z['y'] / 255
    return z


def row_guesses(cfg):
    g = cfg['scales'].shape[0]
    if cfg['w'] <= ROWS_ALL_W:
        return list(range(g))
    return sorted(set(range(0, g, 3)) | set(cfg['special']))


def launch(spectral, cfg, scales=None, rows=None):
    """ops.atlas_correlate on cfg -> (corr, run, rows) as NumPy arrays."""
    from solex_ser_recon_en_amd import ops
    at = spectral.load_atlas(ATLAS)
    lspec = spectral.log_spectrum(cfg['s2'], cfg['ax'])
    lo, hi = spectral.window(cfg['ax'], cfg['w'])
    scales = cfg['scales'] if scales is None else scales
    corr, run, out = ops.atlas_correlate(at.on('cuda'), at.first, at.d, cfg['lam'], cfg['ax'], torch.from_numpy(lspec).cuda(), lo, hi,
                                         torch.from_numpy(np.ascontiguousarray(scales)).cuda(), row_guesses(cfg) if rows is None else rows)
    return corr.cpu().numpy(), run.cpu().numpy(), None if out is None else out.cpu().numpy()


@pytest.fixture(scope='module')
def results(spectral, atlas):
    out = []
    for cfg in adv.configs(atlas['a'], atlas['y']):
        out.append((cfg, adv.records(cfg, atlas['a'], atlas['yv']), launch(spectral, cfg)))
    return out


def test_runs(results):
    n = empty = 0
    for cfg, recs, (corr, run, _) in results:
        for g, r in enumerate(recs):
            if r['k0'] is None:
                assert run[g, 0] > run[g, 1] and math.isnan(corr[g]), (cfg['name'], g, run[g])
                empty += 1
            else:
                assert (int(run[g, 0]), int(run[g, 1])) == (r['k0'], r['k1']), (cfg['name'], g, run[g], r['k0'], r['k1'])
            n += 1
    print('runs: %d guesses equal to select(), %d of them empty' % (n, empty))


def test_rows_bit_exact(results):
    n = 0
    for cfg, recs, (_, _, rows) in results:
        for slot, g in enumerate(row_guesses(cfg)):
            want = recs[g]['row']
            if want is None:
                assert np.isnan(rows[slot]).all(), (cfg['name'], g)
                continue
            assert np.array_equal(rows[slot].view(np.uint64), want.view(np.uint64)), \
                '%s guess %d (s = %r): row differs from np.interp at pixels %s' % (
                    cfg['name'], g, float(cfg['scales'][g]), np.flatnonzero(rows[slot] != want)[:8])
            n += 1
    print('rows: %d bit-exact' % n)


def test_correlation_within_the_bound(results):
    worst = worst_abs = 0.0
    worst_at = None
    n = near = 0
    for cfg, recs, (corr, _, _) in results:
        for g, r in enumerate(recs):
            got = float(corr[g])
            assert math.isnan(got) == math.isnan(r['numpy']), (cfg['name'], g, got, r['numpy'])
            if r['corr'] is None or math.isnan(got):
                continue
            if r['corr'].nan or ex.nearly_constant(r['corr']):
                assert abs(got - r['numpy']) <= 1e-12, (cfg['name'], g, got, r['numpy'])
                near += 1
                continue
            err = float(abs(Fraction(got) - r['corr'].value()))
            assert ex.within(got, r['corr'], r['bound']), (cfg['name'], g, err, r['bound'])
            if err / r['bound'] > worst:
                worst, worst_at = err / r['bound'], (cfg['name'], g, err, r['bound'])
            worst_abs = max(worst_abs, err)
            n += 1
    print('corr: %d guesses within the bound, largest error %.3e = %.3f of the bound (%s guess %d: %.3e, bound %.3e); '
          '%d nearly constant or constant rows within 1e-12 of np.corrcoef' % ((n, worst_abs, worst) + worst_at + (near,)))


def _ge(a, b, slack):
    """a >= b - slack for exact correlations a, b (Fractions) and a float slack that may be inf."""
    return math.isinf(slack) or a >= b - Fraction(slack)


def test_argmax_is_the_exact_maximiser(results):
    decided = loose = 0
    for cfg, recs, (corr, _, _) in results:
        numpy_corr = np.array([r['numpy'] for r in recs])
        pick = int(np.argmax(corr))
        if np.isnan(numpy_corr).any():                       # np.argmax takes the first NaN: so must the kernel's
            assert pick == int(np.argmax(numpy_corr)), cfg['name']
            continue
        best = adv.exact_best(recs)
        if best is None:
            continue
        rb, rp = recs[best], recs[pick]
        gap = adv.top_two_gap(recs)
        bound = max(r['bound'] for r in recs if r['bound'] is not None)
        if gap is not None and math.isfinite(bound) and gap > 2 * Fraction(bound):
            assert rp['corr'].same(rb['corr']), (cfg['name'], pick, best, float(gap), bound)
            decided += 1
        else:
            assert _ge(rp['corr'].value(), rb['corr'].value(), rp['bound'] + rb['bound']), (cfg['name'], pick, best)
            loose += 1
    print('argmax: %d configurations decided by a gap above twice the bound, %d within it (a near-tie taken)' % (decided, loose))
    assert decided >= 100 and loose >= 1


def test_auto_dispersion_takes_the_references_nan(spectral, atlas):
    s2, ax, lam = adv.auto_nan_case(atlas['a'], atlas['y'])
    with np.errstate(invalid='ignore', divide='ignore'):
        want, _ = ref.correlations(s2, ax, lam, atlas['first'], atlas['last'], atlas['step'], atlas['y'])
    disp, corr, scales = spectral.auto_dispersion(s2, ax, lam, spectral.load_atlas(ATLAS))
    assert np.array_equal(np.isnan(corr), np.isnan(want)) and np.isnan(want).any()
    assert disp == float(scales[int(np.argmax(want))])


@pytest.mark.parametrize('name', ['sweep_w37', 'sweep_w130', 'sweep_w513', 'sweep_w8192', 'last_one_point', 'flat_250_ax10.25',
                                  'partly_empty', 'repeated_scales'])
def test_guesses_do_not_leak(spectral, results, name):
    """Each scale of a configuration placed at three positions among the others: the same bits at every position, and the same as
    the configuration's own launch."""
    cfg, _, (corr0, run0, rows0) = next(x for x in results if x[0]['name'] == name)
    s = cfg['scales']
    g = s.shape[0]
    mixed = np.concatenate([s, s[::-1], np.roll(s, 1)])
    where = [np.array([i, 2 * g - 1 - i, g * 2 + (i + 1) % g]) for i in range(g)]
    rows = sorted(set(int(p) for i in range(g) for p in where[i]))
    corr, run, out = launch(spectral, cfg, mixed, rows)
    slot = {p: k for k, p in enumerate(rows)}
    base = {p: k for k, p in enumerate(row_guesses(cfg))}
    for i in range(g):
        for p in where[i]:
            assert corr[p].tobytes() == corr0[i].tobytes() and np.array_equal(run[p], run0[i]), (name, i, p)
            assert out[slot[int(p)]].tobytes() == out[slot[int(where[i][0])]].tobytes(), (name, i, p)
            if i in base:
                assert out[slot[int(p)]].tobytes() == rows0[base[i]].tobytes(), (name, i, p)
