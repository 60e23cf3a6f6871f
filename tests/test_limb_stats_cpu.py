"""tests/limb_stats_ref.py -- the exact restatement the GPU test holds the limb stage's statistics kernels to -- against the oracle
and NumPy on every adversarial case, bit for bit, and the condition that keeps the GPU test from passing on easy inputs: the case
set reaches every decision class in REQUIRED.  No GPU."""
from collections import Counter

import numpy as np
import pytest

from oracle import limb_oracle
from oracle import shg_oracle as orc
from solex_ser_recon_en_amd import order_stats
from tests import limb_stats_ref as ref


@pytest.fixture(scope='module')
def prepared():
    return [(c, ref.prepare(c['disk'], c['k'])) for c in ref.cases()]


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_restatement_equals_the_oracle_and_numpy(prepared, monkeypatch):
    """Block mean == limb_oracle.downscale_local_mean(img / 65536, 4); both blurs == shg_oracle.box_blur_f64; the order statistics
    give np.median and np.percentile; data, its histogram, min and max are NumPy's; and where the reference does not raise (data
    is not empty) flooding at the restatement's threshold gives limb_oracle.get_flood_image's image (its blur window set to the
    case's k: the reference derives it from the height, int(0.01 * sh), which is 0 for these small images)."""
    real_blur = orc.box_blur_f64
    for c, p in prepared:
        tag = c['name']
        k = c['k']
        small = limb_oracle.downscale_local_mean(c['disk'] / 65536, 4)
        assert same_bits(p['B'].astype(np.float64) * ref.UNIT, small), tag
        assert p['B'].shape == (-(-c['disk'].shape[0] // 4), -(-c['disk'].shape[1] // 4)), tag
        want_k, want_5 = real_blur(small, k, k), real_blur(small, 5, 5)
        assert same_bits(p['blur_k'], want_k), tag
        assert same_bits(p['blur_5'], want_5), tag
        assert same_bits(ref.blurred_plane(p['Wk'], k), want_k) and p['Wk'].dtype == np.int64, tag
        assert 0 <= p['Wk'].min() and p['Wk'].max() <= k * k * ref.BLOCK_MAX < 2 ** 32, tag
        n = small.size
        assert p['ranks'][3] < n and same_bits(p['median5'], np.median(want_5)), tag
        assert same_bits(p['very_bright'], np.percentile(want_k, 99)), tag
        assert p['gamma'] == order_stats.lerp_gamma(n, 99) and 0.0 <= p['gamma'] < 1.0, tag
        assert same_bits(p['total'], np.sum(small)), tag
        data = want_k.flatten()
        data = data[data < np.percentile(want_k, 99)]
        assert same_bits(p['data'], data), tag
        if data.size == 0:
            assert p['mn'] is None and p['mx'] is None and p['threshold'] is None and not p['counts'].any(), tag
            with pytest.raises(ValueError):
                data.min()
            continue
        assert same_bits(p['mn'], data.min()) and same_bits(p['mx'], data.max()), tag
        assert np.array_equal(p['counts'], np.histogram(data, bins=20)[0]) and p['counts'].sum() == data.size, tag
        monkeypatch.setattr(limb_oracle.orc, 'box_blur_f64', lambda img, kw, kh, k=k: real_blur(img, k, k))
        with np.errstate(all='ignore'):
            flooded = limb_oracle.get_flood_image(small.copy())
        monkeypatch.undo()
        assert np.array_equal(np.where(want_k < p['threshold'], 0.0, 65000.0), flooded), tag


def test_reflection_folds_as_often_as_needed():
    for n in (1, 2, 3, 5):
        want = np.pad(np.arange(n), (40, 40), mode='reflect') if n > 1 else np.zeros(81, int)
        np.testing.assert_array_equal(ref.reflect101(np.arange(-40, n + 40), n), want)


def test_disk_from_block_sums_gives_the_sums():
    rng = np.random.default_rng(3)
    B = rng.integers(0, ref.BLOCK_MAX + 1, (7, 9))
    B[0, :4] = (0, 1, ref.BLOCK_MAX, ref.BLOCK_MAX - 1)
    for r in (None, rng):
        np.testing.assert_array_equal(ref.block_sums(ref.disk_from_block_sums(B, r)), B)


def test_case_set_reaches_every_required_class(prepared):
    """What the GPU test's worth rests on: counted on the reference alone."""
    total, most = Counter(), Counter()
    for c, p in prepared:
        cls = p['classes'] + ref.layout_classes(c)
        total.update(cls)
        for name, v in cls.items():
            most[name] = max(most[name], v)
        print('LIMB STATS CASE %-24s %4d x %-4d k=%-2d %-4s %s' % (c['name'], p['B'].shape[0], p['B'].shape[1], c['k'], c['layout'],
                                                                 ' '.join('%s=%d' % kv for kv in sorted(cls.items()) if kv[1])))
    print('LIMB STATS CLASSES ' + ' '.join('%s=%d' % (name, total[name]) for name in ref.REQUIRED))
    assert [name for name in ref.REQUIRED if total[name] == 0] == []
    assert {name: most[name] for name, v in ref.REQUIRED_MIN.items() if most[name] < v} == {}
    assert sorted({c['k'] for c, _ in prepared}) == list(ref.WINDOWS)
    assert sum(c['big'] for c, _ in prepared) == 1
    assert len({c['name'] for c, _ in prepared}) == len(prepared)
    for rem_h in (1, 2, 3):
        assert any(c['disk'].shape[0] % 4 == rem_h for c, _ in prepared) and any(c['disk'].shape[1] % 4 == rem_h for c, _ in prepared)
    sides = {s for _, p in prepared for s in p['B'].shape}
    assert {3, 15, 16, 17, 32, 33, 64} <= sides
    sizes = {p['B'].size for _, p in prepared}
    assert {9, 2048, 2049} <= sizes and any((n - 1) % 100 == 0 for n in sizes)


def test_host_refuses_the_empty_flood():
    """What the kernels leave as min / max when nothing lies below very_bright (two NaNs, tests/test_limb_stats_gpu.py) is refused by
    the host's threshold with ValueError, as is any NaN; a threshold is never built on them."""
    from solex_ser_recon_en_amd import hostmath
    lo, hi = np.array([0x7fffffffffffffff, 0xffffffffffffffff], np.uint64).view(np.float64)
    zeros = np.zeros(20, np.int64)
    for mn, mx in ((lo, hi), (float('nan'), 0.5), (0.25, float('nan'))):
        with pytest.raises(ValueError, match='99th percentile'):
            hostmath.flood_threshold(123.0, (100, 10), mn, mx, zeros)
