"""Derotation on the GPU: shg_derotate_u16 against the restatement written from the header (tests/derotate_ref.py) with zero
differing pixels -- centred and off-centre circles that are no integers, a disk that leaves the image on two sides, a width that is no
multiple of 8, pitched inputs and outputs on and off 16 bytes with the padding planted and checked, every orientation, both signs of
the time difference, with and without the limb-darkening table, the behind-limb branch, the identity, a 1 x 1 and an 8 x 3 image --,
every refusal with the output untouched, the Python layer, and three scans of a rotating scene stacked with and without --derotate."""
import math

import numpy as np
import pytest

from solex_ser_recon_en_amd import derotate as _derotate  # noqa: F401  (no feature: no tests)
from tests import derotate_ref as rr
from tests import flatten_ref as fr
from tests.linemaps_util import run_json, write_scan
from tests.test_dejitter_gpu import FILL, PAD, Planes, down16, up16

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import derotate, disk, ops, stack
    from solex_ser_recon_en_amd._lib import lib
    return {'derotate': derotate, 'disk': disk, 'ops': ops, 'stack': stack, 'lib': lib}


def run(lib, img, circle, matrix, rate3, clv, in_aligned, out_aligned, **over):
    """shg_derotate_u16 on the image in a padded buffer into a planted one -> (status, the image or None, whether the input, both
    paddings -- and after a refusal the whole output -- are as they were)."""
    h, w = img.shape
    src, dst = Planes(1, h, w, in_aligned, PAD, img), Planes(1, h, w, out_aligned, FILL)
    c3 = np.ascontiguousarray(circle, dtype=np.float64)
    m9 = np.ascontiguousarray(matrix, dtype=np.float64).reshape(-1)
    k3 = np.ascontiguousarray(rate3, dtype=np.float64)
    table = None if clv is None else torch.from_numpy(np.ascontiguousarray(clv, dtype=np.float64)).cuda()
    keep = {'circle': c3.ctypes.data, 'matrix': m9.ctypes.data, 'rate': k3.ctypes.data}
    st = lib.shg_derotate_u16(over.get('img_ptr', src.ptr), over.get('h', h), over.get('w', w), over.get('pitch', src.pitch),
                              over.get('circle_ptr', keep['circle']), over.get('matrix_ptr', keep['matrix']), over.get('rate_ptr', keep['rate']),
                              None if table is None else table.data_ptr(), over['n_rings'] if 'n_rings' in over else fr.n_rings(circle),
                              over.get('out', dst.ptr), over.get('out_pitch', dst.pitch), None)
    torch.cuda.synchronize()
    back, intact = src.read()
    intact = intact and np.array_equal(back[0], img)
    if st != 0:
        return st, None, bool(intact and dst.untouched())
    got, around = dst.read()
    return st, got[0], bool(intact and around)


def same_image(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, '%s: %d pixels differ, first at %s: %d vs %d' % (what, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def textured(h, w, seed):
    """Half the columns the whole range at random (the cubic leaves the range both ways), half a smooth ramp with noise."""
    rng = np.random.default_rng([h, w, seed])
    img = rng.integers(0, 65536, (h, w))
    smooth = 20000.0 + 60.0 * np.arange(w)[None, :] + 40.0 * np.arange(h)[:, None] + rng.normal(0.0, 300.0, (h, w))
    img[:, w // 2:] = np.clip(np.rint(smooth), 0, 65535)[:, w // 2:]
    return img.astype(np.uint16)


def random_table(circle, seed):
    """A limb-darkening table that no profile would give: every ratio between a quarter and four."""
    return np.random.default_rng(seed).uniform(500.0, 2000.0, fr.n_rings(circle))


# (name, shape, circle, north, b0, mirror, hours)
CASES = [('centred', (250, 260), (129.5 + 0.3, 124.6, 100.4), 0.0, 0.0, False, 6.0),
         ('off_centre_tilted', (250, 260), (141.3, 112.6, 93.7), 17.0, -5.2, False, -6.0),
         ('mirrored', (250, 260), (131.3, 122.6, 100.4), -123.0, 7.1, True, 9.0),
         ('leaves_two_sides', (250, 260), (40.7, 30.2, 100.4), 200.0, 3.0, False, -12.0),
         ('odd_width', (203, 251), (120.2, 99.9, 88.8), 45.0, -7.2, True, 4.0),
         ('larger_than_the_image', (64, 130), (60.5, 30.5, 150.2), 5.0, 1.0, False, 20.0)]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_matches_the_restatement(mods, case):
    lib = mods['lib']
    name, (h, w), circle, north, b0, mirror, hours = case
    matrix = rr.orientation(north, b0, mirror)
    rate3 = rr.rates(hours / 24.0)
    img = textured(h, w, 1)
    moved = 0
    for clv in (None, random_table(circle, 2)):
        ref, parts = rr.derotate(img, circle, matrix, rate3, clv, parts=True)
        moved += int(parts['moved'].sum())
        assert not np.array_equal(ref, img)
        for in_aligned, out_aligned in ((False, False), (True, True), (False, True), (True, False)):
            what = '%s, clv %s, input aligned %s, output aligned %s' % (name, clv is not None, in_aligned, out_aligned)
            st, got, intact = run(lib, img, circle, matrix, rate3, clv, in_aligned, out_aligned)
            assert st == 0 and intact, what
            same_image(got, ref, what)
    assert moved > 0


def test_behind_the_limb_near_the_range_limit(mods):
    lib = mods['lib']
    circle, matrix = (131.3, 122.6, 100.4), rr.orientation(17.0, -5.2)
    img = rr.scene(0.0)
    for sign in (1.0, -1.0):
        rate3 = (sign * 0.45, sign * -0.03, sign * -0.015)                        # |k0| + |k1| + |k2| = 0.495
        for clv in (None, rr.measured_clv(img, circle)):
            ref, parts = rr.derotate(img, circle, matrix, rate3, clv, parts=True)
            assert int(parts['behind'].sum()) > 1000 and np.abs(parts['a']).max() > 0.44, 'the behind-limb branch did not run'
            assert np.array_equal(ref[parts['behind']], img[parts['behind']])
            for aligned in (False, True):
                st, got, intact = run(lib, img, circle, matrix, rate3, clv, aligned, aligned)
                assert st == 0 and intact
                same_image(got, ref, 'a = %+.2f, clv %s, aligned %s' % (rate3[0], clv is not None, aligned))


def test_identity_and_tiny_images(mods):
    lib = mods['lib']
    circle, matrix = (131.3, 122.6, 100.4), rr.orientation(17.0, -5.2, True)
    img = textured(250, 260, 3)
    for clv in (None, random_table(circle, 4)):
        for aligned in (False, True):
            st, got, intact = run(lib, img, circle, matrix, (0.0, 0.0, 0.0), clv, aligned, not aligned)
            assert st == 0 and intact
            same_image(got, img, 'rate3 = 0')
    # k0 alone cancelled at one latitude only: a != 0 almost everywhere
    for shape, circle in (((1, 1), (0.2, 0.1, 3.5)), ((3, 8), (3.6, 1.2, 2.9)), ((3, 8), (3.6, 1.2, 0.0)), ((8, 3), (1.1, 4.2, 9.7)), ((9, 17), (8.0, 4.0, 4.0))):
        img = textured(shape[0], shape[1], 5)
        for clv in (None, random_table(circle, 6)):
            ref = rr.derotate(img, circle, matrix, (0.2, -0.03, -0.02), clv)
            for aligned in (False, True):
                st, got, intact = run(lib, img, circle, matrix, (0.2, -0.03, -0.02), clv, aligned, aligned)
                assert st == 0 and intact, (shape, circle)
                same_image(got, ref, '%r with circle %r' % (shape, circle))


def test_refusals_leave_the_output_untouched(mods):
    lib, ops = mods['lib'], mods['ops']
    h, w = 20, 22
    circle, matrix, rate3 = (10.3, 9.6, 7.5), rr.orientation(10.0, 2.0), (0.1, -0.01, -0.01)
    img = textured(h, w, 7)

    def refused(code, clv=None, circle=circle, matrix=matrix, rate3=rate3, **over):
        if 'n_rings' not in over:
            over['n_rings'] = fr.n_rings((0.0, 0.0, circle[2])) if np.isfinite(circle[2]) and 0 <= circle[2] < 16384 else 8
        st, _, intact = run(lib, img, circle, matrix, rate3, clv, False, False, **over)
        assert st == code and intact, (circle, rate3, over)

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        refused(E_UNSUPPORTED, **over)
    for over in (dict(img_ptr=None), dict(out=None), dict(circle_ptr=None), dict(matrix_ptr=None), dict(rate_ptr=None), dict(pitch=21),
                 dict(out_pitch=21), dict(n_rings=7), dict(n_rings=9), dict(n_rings=0)):
        refused(E_ARG, **over)
    refused(E_ARG, clv=np.ones(9), n_rings=9)
    for bad in ((np.nan, 9.6, 7.5), (10.3, np.inf, 7.5), (10.3, 9.6, np.nan), (10.3, 9.6, -1.0), (10.3, 9.6, 16384.0), (65536.0, 9.6, 7.5),
                (10.3, -65536.0, 7.5)):
        refused(E_ARG, circle=bad)
    skewed, scaled, holed = matrix.copy(), matrix * (1.0 + 1e-9), matrix.copy()
    skewed[0, 1] += 1e-9
    holed[2, 2] = np.nan
    for bad in (skewed, scaled, holed, np.zeros((3, 3))):
        refused(E_ARG, matrix=bad)
    for bad in ((0.4, -0.06, -0.05), (-0.51, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        refused(E_ARG, rate3=bad)
    # (a matrix and rates right at the limits pass)
    st, got, intact = run(lib, img, circle, matrix * (1.0 + 1e-13), (0.25, -0.125, -0.125), None, False, False)
    assert st == 0 and intact
    a = Planes(1, h, w, False, FILL)
    c3, m9, k3 = np.array(circle), np.ascontiguousarray(matrix).reshape(-1), np.array(rate3)
    last = 2 * (19 * a.pitch + 21)
    for out in (a.ptr, a.ptr + last, a.ptr - last):
        assert lib.shg_derotate_u16(a.ptr, h, w, a.pitch, c3.ctypes.data, m9.ctypes.data, k3.ctypes.data, None, 8, out, a.pitch, None) == E_ARG
    torch.cuda.synchronize()
    assert a.untouched()
    dev = up16(img)
    for bad in (dict(matrix=np.eye(4)), dict(rate3=(0.5, 0.1, 0.0)), dict(rate3=(np.nan, 0.0, 0.0)), dict(clv=torch.ones(7, dtype=torch.float64, device='cuda')),
                dict(clv=torch.ones(8, dtype=torch.float32, device='cuda')), dict(out=torch.empty((h, w + 1), dtype=torch.uint16, device='cuda')),
                dict(circle=(1.0, 2.0))):
        with pytest.raises(ValueError):
            ops.derotate_u16(dev, bad.pop('circle', circle), bad.pop('matrix', matrix), bad.pop('rate3', rate3), **bad)
    with pytest.raises(RuntimeError, match='overlaps'):
        ops.derotate_u16(dev, circle, matrix, rate3, out=dev)
    with pytest.raises(RuntimeError):
        ops.derotate_u16(torch.zeros((4, 4), dtype=torch.uint16), (2.0, 2.0, 1.0), matrix, rate3)
    with pytest.raises(RuntimeError):
        ops.derotate_u16(dev, circle, matrix, rate3, clv=torch.ones(8, dtype=torch.float64))
    assert np.array_equal(down16(dev), img)
    mine = ops.pitched_u16(h, w, 'cuda', 8)
    assert ops.derotate_u16(dev, circle, matrix, rate3, out=mine) is mine
    same_image(down16(mine), rr.derotate(img, circle, matrix, rate3), 'the caller\'s output')


# ---- the Python layer ----
def test_derotate_disk_is_the_restatement(mods):
    derotate = mods['derotate']
    circle = rr.SCENE['circle']
    img = rr.scene(0.0)
    dev = up16(img)
    assert np.array_equal(derotate.measured_clv(dev, circle), rr.measured_clv(img, circle))
    assert np.array_equal(derotate.measured_clv(dev, circle, 5), rr.measured_clv(img, circle, 5))
    for dt, north, b0, mirror in ((0.25, 17.0, -5.2, False), (-0.5, -40.0, 6.0, True)):
        matrix, rate3 = rr.orientation(north, b0, mirror), rr.rates(dt)
        for clv, table in (('measure', rr.measured_clv(img, circle)), (None, None), (random_table(circle, 8), random_table(circle, 8))):
            out, record = derotate.derotate_disk(dev, circle, dt, north, b0, mirror, clv=clv)
            ref, parts = rr.derotate(img, circle, matrix, rate3, table, parts=True)
            same_image(down16(out), ref, 'derotate_disk, dt %g' % dt)
            assert record['rings'] == fr.n_rings(circle) and record['a_equator'] == rate3[0] and record['dt_days'] == dt
            assert record['behind_limb'] == int(parts['behind'].sum()) and 0.98 * record['max_px'] <= parts['shift'].max() <= record['max_px']
    out, record = derotate.derotate_disk(dev, circle, 0.0, 17.0, -5.2)
    same_image(down16(out), img, 'dt = 0')
    assert record['max_px'] == 0.0 and record['behind_limb'] == 0
    for bad in (dict(dt_days=2.5), dict(clv='guess'), dict(clv=np.ones(5)), dict(clv=np.zeros(fr.n_rings(circle))), dict(b0=95.0),
                dict(law='carrington'), dict(law=(1.0, 2.0))):
        args = dict(dict(dt_days=0.1, north=0.0, b0=0.0), **bad)
        with pytest.raises(ValueError):
            derotate.derotate_disk(dev, circle, **args)


def test_accuracy_on_the_gpu_is_the_restatements(mods):
    ops = mods['ops']

    def on_gpu(img, circle, matrix, rate3, clv):
        return down16(ops.derotate_u16(up16(img), circle, matrix, rate3, None if clv is None else torch.from_numpy(clv).cuda()))

    for hours, bounds in rr.TOLERANCE.items():
        got = rr.accuracy(hours, on_gpu)
        print('%g h: before %.2f, geometry only %.2f, measured profile %.3f, there and back %.3f counts rms' % (
            hours, got['before'], got['geometry'], got['measured'], got['round_trip']))
        assert got == rr.accuracy(hours)
        assert got['measured'] < got['geometry'] < got['before']
        for key, bound in bounds.items():
            assert got[key] <= bound, (hours, key)


# ---- end to end: three scans of a rotating scene ----
HOURS = (-6.0, 0.0, 6.0)                     # the scans' epochs; the middle one is the reference
TIMES = ['2024-05-01T06:00:00', '2024-05-01T12:00:00Z', '2024-05-01T18:00:00+00:00']
# (latitude, longitude at the reference epoch, radius, depth), radians: spread from limb to limb, so that the spots move by
# different amounts -- 7.6 frames at the centre, 4 at a longitude of one radian -- and no single offset registers them all
SPOTS = [(0.10, -1.0, 0.035, 0.5), (-0.25, -0.6, 0.03, 0.45), (0.30, -0.25, 0.04, 0.4), (-0.05, 0.1, 0.03, 0.5), (0.22, 0.5, 0.035, 0.4),
         (-0.35, 0.95, 0.04, 0.45), (0.45, 0.75, 0.03, 0.5), (-0.5, -0.15, 0.035, 0.4)]


def rotating_scan(hours, seed):
    """synth's scan (300 frames of 400 slit rows) with SPOTS carried along by the default law: north up, B0 = 0, so a point of the
    sphere (west, north, observer) = (cos lat sin lon, sin lat, cos lat cos lon) shows at frame cx + ax west, row cy - ay north."""
    from solex_ser_recon_en_amd import synth
    n, ih, iw = 300, 400, 32
    base = synth.scene_params(n, ih, iw)
    k = rr.rates(hours / 24.0)
    spots = []
    for lat, lon0, rad, depth in SPOTS:
        s2 = math.sin(lat) ** 2
        lon = lon0 + (k[2] * s2 + k[1]) * s2 + k[0]
        spots.append((base['cx'] + base['ax'] * math.cos(lat) * math.sin(lon), base['cy'] - base['ay'] * math.sin(lat), rad * base['ax'],
                      rad * base['ay'], depth))
    return synth.synth_frames_numpy(n, ih, iw, 16, seed=seed, scene={'noise': 0.0005, 'spots': spots})


@pytest.fixture(scope='module')
def series(mods, tmp_path_factory):
    return [write_scan(tmp_path_factory, 'derotate_%d' % i, rotating_scan(hours, 31 + i)) for i, hours in enumerate(HOURS)]


def test_stack_derotate_end_to_end(mods, series, capsys):
    """Three scans six hours apart, eight spots from limb to limb, the default registration, mode mean.  Measured on an MI355X: the rms
    difference between the stack and the reference scan's disk over the inner 0.9 R is 40.36 counts without --derotate and 27.17
    with it, a ratio of 0.673; the test holds the order, not the figures."""
    stack, disk = mods['stack'], mods['disk']
    plain = stack.stack_scans(series, reference=1, mode='mean')
    fixed = stack.stack_scans(series, reference=1, mode='mean', derotate={'north': 0.0, 'b0': 0.0, 'times': TIMES})
    # without the flag: what the pieces that were there before give, bit for bit, and no new key
    disks = [disk.scan_disk(f, None, 0, 'stacking') for f in series]
    images, circles = [d['image'] for d in disks], [d['circle'] for d in disks]
    records = stack.register_disks(images, circles, 1, 8, 0.9)
    by_hand, count = stack.stack_disks(images, records, 'mean', 2.5, 2, tuple(images[1].shape))
    assert np.array_equal(down16(plain['stack']), down16(by_hand)) and np.array_equal(plain['count'].cpu().numpy(), count.cpu().numpy())
    assert 'derotate' not in plain and sorted(set(fixed) - set(plain)) == ['derotate']
    assert all(np.array_equal(down16(a), down16(b)) for a, b in zip(plain['images'], images))
    # with it: the reference is not resampled, the others are, by the analytic angle
    assert np.array_equal(down16(fixed['images'][1]), down16(images[1]))
    assert not np.array_equal(down16(fixed['images'][0]), down16(images[0])) and not np.array_equal(down16(fixed['images'][2]), down16(images[2]))
    recs = fixed['derotate']
    assert recs[1]['dt_days'] == 0.0 and recs[1]['max_px'] == 0.0 and sorted(recs[1]) == sorted(recs[0]) and recs[0]['behind_limb'] is None
    assert recs[0]['dt_days'] == 0.25 and recs[2]['dt_days'] == -0.25 and recs[0]['a_equator'] == rr.rates(0.25)[0]
    rad = circles[0][2]
    assert abs(recs[0]['max_px'] - rad * math.sin(rr.rates(0.25)[0])) < 0.05 * recs[0]['max_px']
    circle = plain['circle']
    mask = rr.inner(images[1].shape, circle)
    reference = down16(images[1])
    before, after = rr.rms(down16(plain['stack']), reference, mask), rr.rms(down16(fixed['stack']), reference, mask)
    with capsys.disabled():
        print('three scans 6 h apart, R = %.1f px, centre moves %.2f px: rms against the reference scan %.2f counts without --derotate, %.2f with '
              '(ratio %.3f)' % (rad, recs[0]['max_px'], before, after, after / before))
    assert after < before
    # the command line: the same stack, and the frames' new key
    out = run_json(stack.main, capsys, series + ['--reference', '1', '--mode', 'mean', '--derotate', '--north', '0', '--b0', '0', '--times', ','.join(TIMES)])
    from solex_ser_recon_en_amd.png_io import read_png_gray
    assert np.array_equal(read_png_gray(out['png']), down16(fixed['stack']))
    for frame, rec in zip(out['frames'], recs):
        assert frame['derotate'] == {'dt_minutes': rec['dt_days'] * 1440.0, 'a_equator': rec['a_equator'], 'max_px': rec['max_px']}
    out = run_json(stack.main, capsys, series + ['--reference', '1', '--mode', 'mean'])
    assert all('derotate' not in frame for frame in out['frames'])
    assert np.array_equal(read_png_gray(out['png']), down16(plain['stack']))
    with pytest.raises(ValueError, match='holds no time stamp'):
        stack.stack_scans(series, derotate={'north': 0.0, 'b0': 0.0})


def test_derotate_command_line(mods, series, tmp_path, capsys):
    import shutil
    from solex_ser_recon_en_amd.png_io import read_png_gray
    derotate = mods['derotate']
    work = str(tmp_path / 'scan.ser')
    shutil.copy(series[0], work)
    out = run_json(derotate.main, capsys, [work, '--north', '0', '--b0', '0', '--dt-minutes', '360'])
    want = derotate.derotate_scan(work, dt_days=0.25, north=0.0, b0=0.0)
    assert out['png'] == work[:-4] + '_shift=0_derot.png' and np.array_equal(read_png_gray(out['png']), down16(want['derotated']))
    assert out['dt_minutes'] == 360.0 and out['a_equator'] == rr.rates(0.25)[0] and out['rings'] == want['derotate']['rings']
    assert out['max_px'] == want['derotate']['max_px'] and out['circle'] == list(want['circle'])
    # a PNG this package wrote, with its circle and both times
    again = run_json(derotate.main, capsys, [out['png'], '--north', '0', '--b0', '0', '--circle', ','.join(repr(v) for v in out['circle']),
                                            '--to', TIMES[0], '--time', TIMES[1], '--no-clv'])
    assert again['png'] == work[:-4] + '_shift=0_derot_derot.png' and again['dt_minutes'] == -360.0 and again['clv'] is False
    back, _ = derotate.derotate_disk(want['derotated'], want['circle'], -0.25, 0.0, 0.0, clv=None)
    assert np.array_equal(read_png_gray(again['png']), down16(back))
    # a scan without a time stamp and no --time
    capsys.readouterr()
    assert derotate.main([work, '--north', '0', '--b0', '0', '--to', TIMES[0]]) == 1
    assert 'holds no time stamp' in capsys.readouterr().err
