"""Derotation without a GPU: the host steps of derotate.py (the orientation matrix, the rotation law, a SER file's time), the
restatement of shg_derotate_u16 on planted cases and on the rotating scene (tests/derotate_ref.py) with the accuracy DESIGN.md
section 25 records, the C entry point's refusals, and every refusal of the two command lines that needs no device."""
import ctypes
import datetime
import math
import struct

import numpy as np
import pytest

from solex_ser_recon_en_amd import derotate, stack
from tests import derotate_ref as rr
from tests import flatten_ref as fr


def test_orientation_is_orthonormal_and_starts_at_the_identity():
    assert np.array_equal(derotate.orientation(0.0, 0.0), np.eye(3))
    assert np.array_equal(derotate.orientation(0.0, 0.0, True), np.diag([-1.0, 1.0, 1.0]))
    for north, b0, mirror in ((17.0, -5.2, False), (-123.0, 7.25, True), (90.0, 0.0, False), (360.0 + 45.0, 90.0, True)):
        m = derotate.orientation(north, b0, mirror)
        assert np.abs(m @ m.T - np.eye(3)).max() < 4e-16 and abs(np.linalg.det(m) - (-1.0 if mirror else 1.0)) < 1e-15
        assert np.abs(m - rr.orientation(north, b0, mirror)).max() < 4e-16
    # solar north, 17 degrees counterclockwise from image-up, is the pole; the disk's centre has the latitude b0
    m = derotate.orientation(17.0, -5.2)
    north_in_image = np.array([-math.sin(math.radians(17.0)), math.cos(math.radians(17.0)), 0.0])
    assert np.allclose(m @ north_in_image, [0.0, math.cos(math.radians(-5.2)), -math.sin(math.radians(-5.2))], atol=1e-15)
    assert abs(math.degrees(math.asin((m @ [0.0, 0.0, 1.0])[1])) - (-5.2)) < 1e-13
    # north is the counterclockwise angle in the image AS GIVEN, mirrored or not: that direction is the pole's, and west lies a
    # quarter turn clockwise of it in the sky, counterclockwise in an east-west flipped image
    for north, b0, mirror in ((17.0, 0.0, True), (17.0, -5.2, True), (-123.0, 7.25, True), (200.0, 3.0, False), (90.0, 0.0, True)):
        m, p, b = derotate.orientation(north, b0, mirror), math.radians(north), math.radians(b0)
        n = np.array([-math.sin(p), math.cos(p), 0.0])
        west = np.array([-n[1], n[0], 0.0]) if mirror else np.array([n[1], -n[0], 0.0])
        assert np.allclose(m @ n, [0.0, math.cos(b), -math.sin(b)], atol=1e-15), (north, b0, mirror)
        assert np.allclose(m @ west, [1.0, 0.0, 0.0], atol=1e-15), (north, b0, mirror)
    # the same for a scan: the angle is given in the written product, which is the scan's disk turned counterclockwise by img_rotate
    for rotate in (0, 90, 180, 270):
        for mirror in (False, True):
            p = math.radians(17.0)
            written = np.array([-math.sin(p), math.cos(p), 0.0])
            in_scan = written.copy()
            for _ in range(rotate // 90):
                in_scan = np.array([in_scan[1], -in_scan[0], 0.0])               # a quarter turn back, clockwise
            m = derotate.orientation(derotate.north_in_scan(17.0, {'img_rotate': rotate}), -5.2, mirror)
            assert np.allclose(m @ in_scan, [0.0, math.cos(math.radians(-5.2)), -math.sin(math.radians(-5.2))], atol=1e-15), (rotate, mirror)
    # west is to the right of north, to the left in a mirrored image
    assert (derotate.orientation(0.0, 0.0) @ [1.0, 0.0, 0.0])[0] == 1.0 and (derotate.orientation(0.0, 0.0, True) @ [1.0, 0.0, 0.0])[0] == -1.0
    for bad in ((np.nan, 0.0), (0.0, np.inf), (0.0, 91.0)):
        with pytest.raises(ValueError):
            derotate.orientation(*bad)


def test_rotation_law():
    a, b, c = derotate.rotation_law()
    assert (a, b, c) == (math.radians(14.71 - 0.9856), math.radians(-2.39), math.radians(-1.78))
    assert derotate.rotation_law('snodgrass', synodic=False)[0] == math.radians(14.71)
    assert derotate.rotation_law((13.0, -2.0, -1.5), synodic=False) == tuple(math.radians(v) for v in (13.0, -2.0, -1.5))
    assert derotate.rates(0.25) == rr.rates(0.25) and derotate.rates(-0.5, (13.0, -2.0, -1.5)) == rr.rates(-0.5, (13.0, -2.0, -1.5))
    assert derotate.rates(0.0) == (0.0, -0.0, -0.0)
    for bad in ('carrington', (1.0, 2.0), (1.0, np.nan, 0.0)):
        with pytest.raises(ValueError):
            derotate.rotation_law(bad)
    # the range: |k0| + |k1| + |k2| <= 0.5 rad is about 1.9 days at the default law
    limit = 0.5 / sum(abs(v) for v in derotate.rotation_law())
    assert 1.5 < limit < 2.0
    derotate.rates(0.999 * limit)
    for bad in (1.001 * limit, -1.001 * limit, np.nan, np.inf):
        with pytest.raises(ValueError):
            derotate.rates(bad)


def ser_with(local, utc, path):
    head = bytearray(178)
    head[0:14] = b'LUCAM-RECORDER'
    struct.pack_into('<qq', head, 162, local, utc)
    path.write_bytes(bytes(head) + b'\0' * 64)
    return str(path)


def test_ser_time(tmp_path):
    epoch = datetime.datetime(1, 1, 1)
    utc = datetime.datetime(2024, 5, 1, 10, 15, 30, 250000)
    local = utc + datetime.timedelta(hours=2)

    def ticks(t):
        return ((t - epoch) // datetime.timedelta(microseconds=1)) * 10

    assert derotate.ser_time(ser_with(ticks(local), ticks(utc), tmp_path / 'both.ser')) == utc
    assert derotate.ser_time(ser_with(ticks(local), 0, tmp_path / 'local.ser')) == local
    assert derotate.ser_time(ser_with(0, 0, tmp_path / 'none.ser')) is None
    (tmp_path / 'short.ser').write_bytes(b'LUCAM-RECORDER')
    with pytest.raises(ValueError):
        derotate.ser_time(str(tmp_path / 'short.ser'))
    with pytest.raises(ValueError, match='late.ser holds a time stamp beyond'):
        derotate.ser_time(ser_with(0, 2 ** 62, tmp_path / 'late.ser'))
    assert derotate.days_between('2024-05-01T09:00:00', '2024-05-01T12:00:00Z') == 0.125
    assert derotate.days_between(utc, '2024-05-01T12:15:30.250+02:00') == 0.0
    with pytest.raises(ValueError):
        derotate.parse_time('noon')


def test_the_header_constants_and_the_polynomials():
    assert rr.coefficients_are_the_nearest_doubles()
    a = np.linspace(-0.5, 0.5, 20001)
    sa, ca = rr.sin_cos(a)
    assert np.abs(sa - np.sin(a)).max() <= 2.0 ** -53 and np.abs(ca - np.cos(a)).max() <= 2.0 ** -52
    assert rr.keys_q14(np.array([0.0, 0.5])).tolist() == [[0, 16384, 0, 0], [-1024, 9216, 9216, -1024]]
    t = np.random.default_rng(0).uniform(0.0, 1.0, 1000)
    from solex_ser_recon_en_amd import dejitter
    assert np.array_equal(rr.keys_q14(t), dejitter.weights(t)[1]) and (rr.keys_q14(t).sum(axis=1) == 16384).all()


def test_zero_rates_return_the_input_bit_for_bit():
    img = np.random.default_rng(1).integers(0, 65536, (60, 70)).astype(np.uint16)
    circle = (33.3, 29.6, 25.4)
    for clv in (None, np.random.default_rng(2).uniform(1.0, 9.0, fr.n_rings(circle))):
        out, parts = rr.derotate(img, circle, rr.orientation(17.0, -5.2, True), (0.0, 0.0, 0.0), clv, parts=True)
        assert np.array_equal(out, img) and not parts['moved'].any() and not parts['behind'].any()
    # off the disk nothing moves either, whatever the rates
    out, parts = rr.derotate(img, circle, rr.orientation(17.0, -5.2), (0.3, -0.05, -0.05), None, parts=True)
    on = fr.rings(60, 70, circle)[2] < np.float64(circle[2]) ** 2
    assert np.array_equal(out[~on], img[~on]) and not parts['moved'][~on].any() and parts['moved'].any()


def test_a_planted_point_moves_by_the_analytic_angle():
    """Rigid rotation (B = C = 0), B0 = 0, north up: a small blob at the disk's centre moves west -- to the right, to the left in a
    mirrored image, a quarter turn clockwise of north in the sky and counterclockwise in a mirrored image whatever the angle of north
    -- by R sin(a).  The blob has sigma = 2 px on R = 100.4: the curvature of x -> R sin(asin(x / R)
    + a) moves its centroid by about sigma^2 sin(a) / (2 R) = 0.006 px, and the Q14 cubic by less: 0.03 px is the bound."""
    h, w, circle = 250, 260, (131.0, 122.0, 100.4)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    blob = np.exp(-0.5 * ((xx - circle[0]) ** 2 + (yy - circle[1]) ** 2) / 4.0)
    img = np.where(fr.rings(h, w, circle)[0], 20000.0 + 10000.0 * blob, 300.0).astype(np.uint16)

    def centroid(a):
        wgt = np.clip(a.astype(np.float64) - 20000.0, 0.0, None) * fr.rings(h, w, (circle[0], circle[1], 60.0))[0]
        return (wgt * xx).sum() / wgt.sum(), (wgt * yy).sum() / wgt.sum()

    x0, y0 = centroid(img)
    for days in (0.25, -0.5, 1.0):
        angle = math.radians(13.0) * days
        move = circle[2] * math.sin(angle)
        for north, mirror in ((0.0, False), (0.0, True), (90.0, False), (180.0, False), (90.0, True), (30.0, True), (-50.0, True), (30.0, False)):
            p = math.radians(north)
            n = (-math.sin(p), math.cos(p))                                      # north in the image, (right, up)
            west = (-n[1], n[0]) if mirror else (n[1], -n[0])
            want = (move * west[0], -move * west[1])                             # (columns, rows): rows run down
            out = rr.derotate(img, circle, derotate.orientation(north, 0.0, mirror), derotate.rates(days, (13.0, 0.0, 0.0)))
            x1, y1 = centroid(out)
            assert abs((x1 - x0) - want[0]) < 0.03 and abs((y1 - y0) - want[1]) < 0.03, (days, north, mirror, x1 - x0, y1 - y0, want)


def test_the_host_statistics_against_the_restatement():
    """behind_limb restates the header's steps 1 to 5 operation for operation, so its count is the restatement's (and the kernel's)
    exactly; largest_displacement is a bound that the equator all but reaches."""
    for shape, circle, north, b0, mirror, rate3 in (((250, 260), (131.3, 122.6, 100.4), 17.0, -5.2, False, (0.45, -0.03, -0.015)),
                                                    ((250, 260), (131.3, 122.6, 100.4), -40.0, 6.0, True, rr.rates(-0.5)),
                                                    ((250, 260), (40.7, 30.2, 100.4), 200.0, 3.0, False, (-0.45, 0.03, 0.015)),
                                                    ((64, 130), (60.5, 30.5, 150.2), 5.0, 1.0, True, rr.rates(0.25)),
                                                    ((20, 22), (10.3, 9.6, 0.0), 5.0, 1.0, False, rr.rates(0.25))):
        matrix = rr.orientation(north, b0, mirror)
        parts = rr.derotate(np.zeros(shape, np.uint16), circle, matrix, rate3, None, parts=True)[1]
        assert derotate.behind_limb(shape, circle, matrix, rate3) == int(parts['behind'].sum()), (circle, rate3)
        assert derotate.behind_limb(shape, circle, matrix, rate3, rows=7) == int(parts['behind'].sum())
        bound = derotate.largest_displacement(circle, rate3)
        assert parts['shift'].max() <= bound
        if shape == (250, 260) and circle[0] > 100:
            assert parts['shift'].max() >= 0.98 * bound
    assert derotate.largest_angle((0.2, -0.03, -0.02)) == 0.2 and derotate.largest_angle((0.0, 0.4, -0.4)) == pytest.approx(0.1)
    assert derotate.largest_angle((-0.1, 0.0, 0.3)) == pytest.approx(0.2) and derotate.largest_displacement((0, 0, 100.0), (0.0, 0.0, 0.0)) == 0.0
    assert derotate.behind_limb((50, 50), (25.0, 25.0, 20.0), np.eye(3), (0.0, 0.0, 0.0)) == 0


def test_the_spots_are_a_minority_of_every_ring():
    for days in (0.0, 1.0 / 24.0, 0.25):
        assert rr.spot_share_of_rings(days) < 0.5


@pytest.mark.parametrize('hours', sorted(rr.TOLERANCE))
def test_accuracy_on_the_rotating_scene(hours):
    got = rr.accuracy(hours)
    print('%g h: before %.2f, geometry only %.2f, measured profile %.3f, there and back %.3f counts rms; %d pixels from behind the limb'
          % (hours, got['before'], got['geometry'], got['measured'], got['round_trip'], got['behind']))
    assert got['measured'] < got['geometry'] < got['before']
    for key, bound in rr.TOLERANCE[hours].items():
        assert got[key] <= bound, key
    assert 0 < got['behind'] < 100


def test_measured_clv_fills_an_empty_innermost_ring():
    """A disk whose centre lies off the image: ring 0 (and more) holds no pixel and takes its nearest neighbour's value."""
    img = rr.scene(0.0, with_spots=False)[:, 140:]
    circle = (131.3 - 140.0, 122.6, 100.4)
    count = fr.ring_medians(img, circle)[0]
    table = rr.measured_clv(img, circle)
    first = int(np.flatnonzero(count > 0)[0])
    assert first > 5 and (table[:first] == table[first]).all() and (table > 0).all() and np.isfinite(table).all()
    out = rr.derotate(img, circle, rr.orientation(17.0, -5.2), rr.rates(0.25), table)
    assert out.shape == img.shape


def test_the_c_entry_point_refuses_without_a_gpu():
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    img, out = ctypes.c_void_p(4096), ctypes.c_void_p(65536)
    circle, matrix, rate = np.array([4.0, 4.0, 3.5]), np.ascontiguousarray(rr.orientation(17.0, -5.2)), np.array([0.1, -0.01, -0.01])

    def call(img=img, h=8, w=8, pitch=8, circle=circle, matrix=matrix, rate=rate, n_rings=4, out=out, out_pitch=8):
        return lib.shg_derotate_u16(img, h, w, pitch, *(None if a is None else a.ctypes.data for a in (circle, matrix, rate)), None, n_rings, out,
                                    out_pitch, None)

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        assert call(**over) == -3, over
        assert 'shg_derotate_u16' in _lib.last_error()
    scaled, holed = matrix * (1.0 + 1e-9), matrix.copy()
    holed[1, 1] = np.inf
    for over in (dict(img=None), dict(out=None), dict(circle=None), dict(matrix=None), dict(rate=None), dict(pitch=7), dict(out_pitch=7),
                 dict(n_rings=3), dict(n_rings=5), dict(circle=np.array([4.0, np.nan, 3.5])), dict(circle=np.array([4.0, 4.0, -1.0])),
                 dict(circle=np.array([4.0, 4.0, 16384.0]), n_rings=16385), dict(circle=np.array([65536.0, 4.0, 3.5])), dict(matrix=scaled),
                 dict(matrix=holed), dict(matrix=np.zeros((3, 3))), dict(rate=np.array([0.4, 0.06, -0.05])), dict(rate=np.array([np.nan, 0.0, 0.0])),
                 dict(out=img), dict(out=ctypes.c_void_p(4096 + 2 * 63)), dict(out=ctypes.c_void_p(4096 - 2 * 63))):
        assert call(**over) == -1, over
        assert 'shg_derotate_u16' in _lib.last_error()
    assert 'overlaps' in _lib.last_error()


def test_command_line_refusals(capsys):
    need = ['--north', '10', '--b0', '2']
    for argv, message in ((['x.ser', '--dt-minutes', '30'], 'needs --north and --b0'), (['x.ser', '--north', '10', '--dt-minutes', '30'], 'needs --north and --b0'),
                          (['x.ser', '--north', '10', '--b0', '95', '--dt-minutes', '30'], '|b0| <= 90'),
                          (['x.ser'] + need, 'give one of --dt-minutes and --to'),
                          (['x.ser', '--dt-minutes', '30', '--to', '2024-05-01T10:00:00'] + need, 'give one of --dt-minutes and --to'),
                          (['x.ser', '--dt-minutes', '30', '--time', '2024-05-01T10:00:00'] + need, '--time goes with --to'),
                          (['x.ser', '--to', 'noon'] + need, 'a time is ISO 8601'),
                          (['x.ser', '--to', '2024-05-01T10:00:00', '--time', 'then'] + need, 'a time is ISO 8601'),
                          (['x.ser', '--dt-minutes', '4000'] + need, 'the limit is 0.5'),
                          (['x.ser', '--dt-minutes', '30', '--rotation', '13,2'] + need, '--rotation is A,B,C'),
                          (['x.ser', '--dt-minutes', '30', '--circle', '1,2'] + need, '--circle is cx,cy,rad'),
                          (['x.ser', '--dt-minutes', '30', '--circle', '1,2,0'] + need, '--circle is cx,cy,rad'),
                          (['x.ser', '--dt-minutes', '30', '--circle', '100,100,80'] + need, '--circle goes with a PNG'),
                          (['x.png', '--dt-minutes', '30'] + need, 'a PNG needs --circle'),
                          (['x.png', '--circle', '100,100,80', '--to', '2024-05-01T10:00:00'] + need, 'a PNG holds no time'),
                          (['x.ser', 'y.ser', '--dt-minutes', '30'] + need, 'exactly one'),
                          (['no_such_file.ser', '--dt-minutes', '30'] + need, 'no such file')):
        with pytest.raises(SystemExit) as exit_:
            derotate.main(argv)
        said = capsys.readouterr()
        assert exit_.value.code == 2 and said.out == '' and message in said.err, (argv, said.err)


def test_stack_derotate_refusals(capsys, tmp_path):
    two = ['x.ser', 'y.ser']
    on = ['--derotate', '--north', '10', '--b0', '2']
    for argv, message in ((two + ['--north', '10'], '--north needs --derotate'), (two + ['--b0', '2'], '--b0 needs --derotate'),
                          (two + ['--mirror'], '--mirror needs --derotate'), (two + ['--times', 'a,b'], '--times needs --derotate'),
                          (two + ['--interval', '60'], '--interval needs --derotate'), (two + ['--rotation', '13,-2,-1'], '--rotation needs --derotate'),
                          (two + ['--no-clv'], '--no-clv needs --derotate'), (two + ['--derotate'], 'needs --north and --b0'),
                          (two + ['--derotate', '--north', '10'], 'needs --north and --b0'),
                          (two + on + ['--times', '2024-05-01T10:00:00,2024-05-01T10:10:00', '--interval', '600'], 'exclude each other'),
                          (two + on + ['--times', '2024-05-01T10:00:00,soon'], 'a time is ISO 8601'),
                          (two + on + ['--times', '2024-05-01T10:00:00'], '--times names 1 times for 2 scans'),
                          (two + on + ['--rotation', '13'], '--rotation is A,B,C'), (two + on + ['--interval', 'nan'], '--interval is a finite'),
                          (two + ['--derotate', '--north', '10', '--b0', '-91'], '|b0| <= 90')):
        with pytest.raises(SystemExit) as exit_:
            stack.main(argv)
        said = capsys.readouterr()
        assert exit_.value.code == 2 and said.out == '' and message in said.err, (argv, said.err)
    # the library: checked before a scan is read (these files hold a header and nothing else)
    stamped, bare = ser_with(0, 638501000000000000, tmp_path / 'stamped.ser'), ser_with(0, 0, tmp_path / 'bare.ser')
    for bad, message in ((dict(north=10.0), 'needs north and b0'), (dict(north=10.0, b0=2.0, colour='red'), 'derotate knows'),
                         (dict(north=10.0, b0=2.0), 'bare.ser holds no time stamp'), (dict(north=10.0, b0=2.0, times=['2024-05-01T10:00:00']), '1 times for 2 scans'),
                         (dict(north=10.0, b0=2.0, times=['a', 'b']), 'a time is ISO 8601'), (dict(north=10.0, b0=2.0, interval=60.0, times=['a', 'b']), 'not both'),
                         (dict(north=10.0, b0=2.0, interval=np.inf), 'finite number of seconds'), (dict(north=10.0, b0=200.0, interval=60.0), '|b0| <= 90'),
                         (dict(north=10.0, b0=2.0, interval=60.0, law='carrington'), 'rotation law is one of'),
                         (dict(north=10.0, b0=2.0, interval=60.0, clv=np.ones(4)), 'clv is')):
        with pytest.raises(ValueError, match=message.replace('|', r'\|')):
            stack.stack_scans([stamped, bare], derotate=bad)
    plan = derotate.series_plan([stamped, stamped], north=10.0, b0=2.0, mirror=True)
    assert plan['times'] == [derotate.ser_time(stamped)] * 2 and plan['north'] == 10.0 and plan['mirror'] is True
    plan = derotate.series_plan(['a', 'b', 'c'], dict(img_rotate=90), north=10.0, b0=2.0, interval=90.0)
    assert [derotate.days_between(plan['times'][0], t) * 86400.0 for t in plan['times']] == [0.0, 90.0, 180.0] and plan['north'] == -80.0
    # a series that spans more than the range: refused by derotate_series before any kernel
    plan = derotate.series_plan(['a', 'b'], north=0.0, b0=0.0, interval=3.0 * 86400.0)
    with pytest.raises(ValueError, match='the limit is 0.5'):
        derotate.derotate_series([None, None], [(5.0, 5.0, 4.0)] * 2, plan, 0)
