"""The Python layer of the emission-line maps that needs no GPU (solex_ser_recon_en_amd/prominence.py): the ring of a circle, its
mask and statistics against the restatement's ring test (tests/emission_ref.py), and the refusals of emission_maps() and of the
command line, which come before any frame is read."""
import math

import numpy as np
import pytest

from solex_ser_recon_en_amd import prominence
from tests import emission_ref as er


def test_ring_of_a_circle():
    assert prominence.ring_of((200.5, 198.25, 175.0), 3, 1.4) == (200.5, 198.25, 178.0, 175.0 * 1.4)
    assert prominence.ring_of((200.5, 198.25, 175.0), 0, math.inf) == (200.5, 198.25, 175.0, math.inf)
    assert prominence.ring_of((200.5, 198.25, 175.0), 3, 1.4, on_disk=True) == (200.5, 198.25, -1.0, 175.0 * 1.4)
    assert prominence.ring_of((200.5, 198.25, 175.0), -500, 1.0) == (200.5, 198.25, 0.0, 175.0)          # r_in never below 0
    assert prominence.ring_of((10.0, 10.0, 100.0), 40, 1.4) == (10.0, 10.0, 140.0, 100.0 * 1.4)           # r_in = r_out: accepted
    for none in (None, (-1, -1, -1), [-1, -1, -1]):                 # ratio_fixe / slant_fix: no limb fit, no ring
        assert prominence.ring_of(none, 3, 1.4) is None
    with pytest.raises(ValueError, match='empty'):
        prominence.ring_of((10.0, 10.0, 100.0), 41, 1.4)
    for ring in (prominence.ring_of((20.0, 12.0, 5.0), 0, 2.0), prominence.ring_of((20.0, 12.0, 5.0), 2, math.inf)):
        assert er.check_ring(ring) == ring                          # what shg_line_emission_finish accepts


RINGS = [(20.0, 12.0, 5.0, 10.0),                                   # 3-4-5 and 6-8-10 pixels lie on the radii exactly
         (20.0, 12.0, math.nextafter(5.0, 0.0), math.nextafter(10.0, 0.0)), (20.0, 12.0, math.nextafter(5.0, 6.0), math.nextafter(10.0, 11.0)),
         (20.0, 12.0, -1.0, 10.0), (20.0, 12.0, 0.0, 0.0), (20.0, 12.0, 5.0, math.inf), (19.7, 11.3, 4.45, 9.55), None]


def test_ring_mask_is_the_finish_test():
    for ring in RINGS:
        keep = prominence.ring_mask((24, 41), ring)
        assert keep.dtype == bool and np.array_equal(keep, er.ring_keep(24, 41, ring)), ring
    keep = prominence.ring_mask((24, 41), RINGS[0])
    assert not keep[12, 25] and not keep[16, 23] and keep[12, 26]               # on r_in: masked; just outside it: kept
    assert keep[12, 30] and keep[20, 26] and not keep[12, 31]                   # on r_out: kept; just outside it: masked
    assert prominence.ring_mask((24, 41), RINGS[1])[12, 25] and not prominence.ring_mask((24, 41), RINGS[1])[12, 30]
    assert prominence.ring_mask((24, 41), RINGS[3])[12, 20] and not prominence.ring_mask((24, 41), RINGS[4])[12, 20]
    assert prominence.ring_mask((3, 5), None).all()


def test_ring_stats_count_the_ring():
    ring = RINGS[0]
    keep = prominence.ring_mask((24, 41), ring)
    m = np.full((24, 41), np.nan, dtype=np.float32)
    m[~keep] = 1e6                                                  # values outside the ring do not count
    on = np.flatnonzero(keep.ravel())
    m.ravel()[on[:101]] = np.arange(101, dtype=np.float32)
    stats = prominence.ring_stats(m, ring)
    assert stats == {'valid_fraction': 101 / on.size, 'median': 50.0, 'p1': 1.0, 'p99': 99.0}
    assert prominence.ring_stats(np.full((24, 41), np.nan, dtype=np.float32), ring) == {
        'valid_fraction': 0.0, 'median': None, 'p1': None, 'p99': None}
    assert prominence.ring_stats(np.ones((4, 4), dtype=np.float32), None)['valid_fraction'] == 1.0


def test_emission_maps_refuses_before_reading():
    for kw in (dict(min_excess=-1.0), dict(min_excess=math.nan), dict(min_excess=math.inf), dict(outer=0.9), dict(outer=math.nan),
               dict(inner=math.inf), dict(inner=math.nan)):
        with pytest.raises(ValueError):
            prominence.emission_maps(None, **kw)                    # (no reader: the refusal comes first)


def test_command_line_refusals(monkeypatch, capsys):
    for argv in (['x.ser', '--min-excess', '-1'], ['x.ser', '--min-excess', 'nan'], ['x.ser', '--min-excess', 'inf'],
                 ['x.ser', '--outer', '0.5'], ['x.ser', '--outer', 'nan'], ['x.ser', '--inner', 'inf'], ['x.ser', '--half-width', '33'],
                 ['x.ser', '-w', '1,2'], ['x.ser', '--shift', '1', '--line', '6562.8']):
        with pytest.raises(SystemExit) as e:
            prominence.main(argv)
        assert e.value.code == 2, argv
    assert 'not an emission-map flag' in capsys.readouterr().err
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit):
        prominence.main(['x.ser'])
    assert 'without torchrun' in capsys.readouterr().err
    assert prominence.PLANES == er.PLANES and prominence.DEFAULT_OUTER == 1.4
