"""Measuring the blur from the limb, on the CPU: the restatement of the tables against the header's own words
and against an arctangent, the recovery of planted widths within psf_ref.TOLERANCE, the sectors that are dropped and why, what the
estimate is worth to the deconvolution, the refusals of the C entry points that need no device, and the command lines with the
kernels stubbed."""
import ctypes
import json

import numpy as np
import pytest

from solex_ser_recon_en_amd import deconvolve, psf
from tests import deconvolve_ref as dr
from tests import psf_ref as pr


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the restatement says what the header says ----
def test_sectors_follow_the_header_on_every_boundary():
    from solex_ser_recon_en_amd import ops
    circle, reach, sub, sectors = (50.0, 50.0, 30.0), 5, 4, 32
    s, b, counts = pr.sector_and_bin(101, 101, circle, reach, sub, sectors, pr.thresholds(sectors))
    # (column, row) -> sector: dy = 0 in octants 0 and 3, dx = 0 in 1 and 6, |dx| = |dy| in 0, 3, 4 and 7
    for (c, r), want in {(80, 50): 0, (50, 80): 7, (20, 50): 15, (50, 20): 24, (71, 71): 3, (29, 71): 12, (29, 29): 19, (71, 29): 28}.items():
        assert counts[r, c] and s[r, c] == want, ((c, r), s[r, c], want)
    # rho = 30 exactly is v = reach * sub exactly: the bin above the boundary; rho = 25 is bin 0 and rho = 35 counts no more
    assert b[50, 80] == reach * sub and b[50, 75] == 0 and counts[50, 75] and not counts[50, 85] and counts[50, 84]
    assert b[50 + 24, 50 + 18] == reach * sub                                  # 18^2 + 24^2 = 30^2
    # away from the boundaries the fold is the arctangent's sector, counted from +column towards +row
    dx = np.arange(101.0)[None, :] - 50.0
    dy = np.arange(101.0)[:, None] - 50.0
    turn = np.mod(np.arctan2(dy, dx), 2.0 * np.pi) / (2.0 * np.pi / sectors)
    clear = counts & (np.abs(turn - np.rint(turn)) > 1e-6)
    assert clear.sum() > 1500 and np.array_equal(s[clear], np.floor(turn[clear]).astype(np.int64))
    for n in (8, 16, 64):
        t = pr.thresholds(n)
        assert t.size == n // 8 - 1 and (np.diff(t) > 0).all() and ((t > 0) & (t < 1)).all()
        assert np.array_equal(t, ops.sector_thresholds(n))                     # the same doubles
    count, total, sumsq = pr.limb_profile(np.full((101, 101), 65535, np.uint16), circle, reach, sub, sectors)
    assert count.sum() == counts.sum() and total.sum() == 65535 * int(counts.sum()) and sumsq.sum() == 65535 ** 2 * int(counts.sum())


def test_equal_taps_and_padding_in_the_xy_restatement():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 65536, (23, 31)).astype(np.uint16)
    k = dr.gaussian(1.3, 4)
    assert np.array_equal(bits(pr.deconvolve_xy(img, k, k, 3)[1]), bits(dr.deconvolve(img, k, 3)[1]))
    kx, ky = dr.gaussian(0.8, 2), dr.gaussian(2.1, 7)
    got = pr.deconvolve_xy(img, kx, ky, 2)[1]
    assert np.array_equal(bits(got), bits(pr.deconvolve_xy(img, dr.pad_taps(kx, 7), ky, 2)[1]))          # property (c)
    assert not np.array_equal(got, pr.deconvolve_xy(img, ky, kx, 2)[1])                                  # the axes are told apart
    # the transposed image with the sets swapped: the transposed estimate, up to the order of the two passes
    one = pr.deconvolve_xy(img, kx, ky, 1)[1]
    other = pr.deconvolve_xy(np.ascontiguousarray(img.T), ky, kx, 1)[1].T
    assert (np.abs(one.astype(np.float64) - other) <= pr.transpose_bound(kx, ky) * np.maximum(one, other)).all()


# ---- recovery ----
CASES = [p + (0.0,) for p in pr.PLANTED] + [(1.0, 2.0, pr.NOISE)]


@pytest.fixture(scope='module')
def recovered():
    got = {}
    for sx, sy, noise in CASES:
        est = pr.estimate(pr.limb_scene(sx, sy, noise, seed=1))
        got[(sx, sy, noise)] = est
        print('planted (%g, %g), noise %g: sigma_x %.4f (%+.4f), sigma_y %.4f (%+.4f), %d sectors, fit %.3f s'
              % (sx, sy, noise, est['sigma_x'], est['sigma_x'] - pr.expected(sx), est['sigma_y'], est['sigma_y'] - pr.expected(sy),
                 est['n_used'], est['fit_seconds']))
    return got


@pytest.mark.parametrize('case', CASES)
def test_planted_widths_are_recovered(recovered, case):
    sx, sy, _ = case
    est = recovered[case]
    assert abs(est['sigma_x'] - pr.expected(sx)) <= pr.TOLERANCE['recovery']
    assert abs(est['sigma_y'] - pr.expected(sy)) <= pr.TOLERANCE['recovery']
    assert est['isotropic'] is False and est['n_used'] >= 28 and len(est['sectors']) == 32
    assert est['fit_seconds'] < 2.0                                           # the naive prototype's time for 32 sectors


def test_the_recovery_bound_is_the_measured_error_plus_two_hundredths(recovered):
    worst = max(max(abs(est['sigma_x'] - pr.expected(sx)), abs(est['sigma_y'] - pr.expected(sy))) for (sx, sy, _), est in recovered.items())
    print('the largest error over the four cases: %.4f px' % worst)
    assert pr.TOLERANCE['recovery'] < 0.1
    assert worst + 0.0195 <= pr.TOLERANCE['recovery'] <= worst + 0.0205


def test_fit_edge_is_one_row_of_fit_edges():
    img = pr.limb_scene(1.0, 2.0)
    count, total, _ = pr.limb_profile(img, pr.CIRCLE, 12, 4, 32)
    t = psf.bin_centres(12, 4)
    mean = total / np.maximum(count, 1)
    sigma, t0, residual, on_edge = psf.fit_edges(t, mean, count)
    one = psf.fit_edge(t, mean[5], count[5])
    assert one[:3] == pytest.approx((sigma[5], t0[5], residual[5]), rel=1e-8, abs=1e-8) and one[3] is bool(on_edge[5])      # (BLAS sums differ in the last bits)
    assert not on_edge.any() and (np.abs(t0) < 0.3).all()
    # a flat sector has no edge: the minimum runs to the grid's edge
    assert psf.fit_edge(t, np.full(t.size, 700.0) + 0.01 * t, np.full(t.size, 9))[3] is True


# ---- sector rejection ----
def unused(est):
    return {i: s['why_not'] for i, s in enumerate(est['sectors']) if not s['used']}


def sectors_leaving(shape, circle, reach=12, sub=4, sectors=32):
    """By geometry, not by binning pixels: the sectors in which more than a tenth of the radial bins have none of their arc inside
    the image's area."""
    h, w = shape
    theta = (np.arange(sectors)[:, None] + np.linspace(0.0, 1.0, 401)[None, :]) * (2.0 * np.pi / sectors)
    gone = []
    for s in range(sectors):
        empty = 0
        for t in psf.bin_centres(reach, sub):
            x = circle[0] + (circle[2] + t) * np.cos(theta[s])
            y = circle[1] + (circle[2] + t) * np.sin(theta[s])
            empty += not ((x >= -0.5) & (x <= w - 0.5) & (y >= -0.5) & (y <= h - 0.5)).any()
        if empty > 0.1 * 2 * reach * sub:
            gone.append(s)
    return gone


def test_a_disk_cut_by_the_left_border_drops_the_sectors_that_leave():
    circle = (70.3, 131.7, 100.4)
    est = pr.estimate(pr.limb_scene(1.0, 2.0, circle=circle), circle)
    gone = sectors_leaving(pr.SHAPE, circle)
    assert gone == list(range(12, 20))
    assert unused(est) == {s: 'leaves the image' for s in gone}
    assert est['n_used'] == 24 and not est['isotropic']
    print('24 of 32 sectors: sigma_x %+.4f, sigma_y %+.4f off' % (est['sigma_x'] - pr.expected(1.0), est['sigma_y'] - pr.expected(2.0)))
    assert abs(est['sigma_x'] - pr.expected(1.0)) <= pr.TOLERANCE['recovery']
    assert abs(est['sigma_y'] - pr.expected(2.0)) <= pr.TOLERANCE['recovery']


def test_a_blob_on_the_limb_drops_its_sector():
    est = pr.estimate(pr.limb_scene(1.0, 2.0, blob=(psf.sector_angles(32)[5], 8000.0)))
    assert unused(est) == {5: 'beyond 3 robust sigma of the regression'}
    assert abs(est['sigma_x'] - pr.expected(1.0)) <= pr.TOLERANCE['recovery']
    assert abs(est['sigma_y'] - pr.expected(2.0)) <= pr.TOLERANCE['recovery']


def test_sectors_along_one_axis_give_one_width():
    shape, circle = (60, 250), (124.3, 30.2, 100.4)
    est = pr.estimate(pr.limb_scene(1.5, 1.5, shape=shape, circle=circle), circle)
    assert [i for i, s in enumerate(est['sectors']) if s['used']] == [0, 1, 14, 15, 16, 17, 30, 31]
    assert est['isotropic'] is True and est['sigma_x'] == est['sigma_y']
    assert abs(est['sigma_x'] - pr.expected(1.5)) <= pr.TOLERANCE['recovery']


def test_two_sectors_are_too_few():
    count, total, _ = pr.limb_profile(pr.limb_scene(1.5, 1.5), pr.CIRCLE, 12, 4, 32)
    keep = np.zeros(32, bool)
    keep[[3, 20]] = True
    with pytest.raises(ValueError, match='2 usable sectors of 32'):
        psf.estimate_from_profiles(count * keep[:, None].astype(np.uint32), total * keep[:, None].astype(np.uint64), psf.bin_centres(12, 4))


def test_a_circle_that_is_off_moves_t0_and_not_sigma(recovered):
    good = recovered[(1.0, 2.0, 0.0)]
    cx, cy, rad = pr.CIRCLE
    est = pr.estimate(pr.limb_scene(1.0, 2.0, seed=1), (cx + 0.4, cy - 0.3, rad + 0.5))
    assert abs(est['sigma_x'] - pr.expected(1.0)) <= pr.TOLERANCE['recovery']
    assert abs(est['sigma_y'] - pr.expected(2.0)) <= pr.TOLERANCE['recovery']
    t0 = np.array([s['t0'] for s in est['sectors']])
    before = np.array([s['t0'] for s in good['sectors']])
    theta = psf.sector_angles(32)
    # the edge sits at rho = rad seen from the true centre: t0 = -0.5 - 0.4 cos theta + 0.3 sin theta from the circle that is off
    assert np.abs(before).max() < 0.1
    assert np.abs(t0 - (-0.5 - 0.4 * np.cos(theta) + 0.3 * np.sin(theta))).max() < 0.1


# ---- why it pays ----
def test_the_estimated_pair_deconvolves_better_than_the_default():
    img, model, circle, region = pr.pays_scene()
    est = pr.estimate(img, circle)
    kx, ky = deconvolve.gaussian_taps(est['sigma_x']), deconvolve.gaussian_taps(est['sigma_y'])
    with_pair = dr.rms(pr.deconvolve_xy(img, kx, ky, 10)[0], model, region)
    with_default = dr.rms(dr.deconvolve(img, deconvolve.gaussian_taps(deconvolve.DEFAULT_SIGMA), 10)[0], model, region)
    ratio = with_pair / with_default
    print('estimated (%.3f, %.3f): %.3f counts rms inside rad - 20; the default 1.2: %.3f; the blurred image: %.3f; ratio %.5f'
          % (est['sigma_x'], est['sigma_y'], with_pair, with_default, dr.rms(img, model, region), ratio))
    assert ratio < 1.0 and ratio <= pr.TOLERANCE['pays'] < 1.0
    assert abs(pr.TOLERANCE['pays'] - (ratio + 0.25 * (1.0 - ratio))) < 0.002, 'the bound is the ratio plus a quarter of its distance to 1'


# ---- the C entry points refuse before they touch a device ----
E_ARG, E_UNSUPPORTED = -1, -3


def test_limb_profile_refusals_need_no_gpu():
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    img, count, total, sumsq = (ctypes.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 4 << 20))
    table = pr.thresholds(32)

    def call(img=img, h=97, w=83, pitch=103, circle=(40.0, 50.0, 30.4), reach=12, sub=4, sectors=32, thresholds=table, count=count,
             total=total, sumsq=sumsq):
        c3 = None if circle is None else np.array(circle, np.float64)
        return lib.shg_limb_profile_u16(img, h, w, pitch, None if c3 is None else c3.ctypes.data, reach, sub, sectors,
                                        None if thresholds is None else np.ascontiguousarray(thresholds, np.float64).ctypes.data,
                                        count, total, sumsq, None)

    nan, inf = float('nan'), float('inf')
    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        assert call(**over) == E_UNSUPPORTED, over
    for over in (dict(img=None), dict(circle=None), dict(thresholds=None), dict(count=None), dict(total=None), dict(sumsq=None), dict(pitch=82),
                 dict(circle=(nan, 50.0, 30.4)), dict(circle=(40.0, inf, 30.4)), dict(circle=(40.0, 50.0, nan)), dict(circle=(40.0, 50.0, -1.0)),
                 dict(circle=(40.0, 50.0, 16384.0)), dict(circle=(65536.0, 50.0, 30.4)), dict(circle=(40.0, -65536.0, 30.4)),
                 dict(reach=0), dict(reach=65), dict(reach=30), dict(circle=(40.0, 50.0, 12.9)), dict(sub=0), dict(sub=9),
                 dict(sectors=0), dict(sectors=4), dict(sectors=12), dict(sectors=72), dict(sectors=-8),
                 dict(thresholds=[0.2, nan, 0.7]), dict(thresholds=[0.2, 0.2, 0.7]), dict(thresholds=[0.5, 0.4, 0.7]), dict(thresholds=[0.0, 0.4, 0.7]),
                 dict(thresholds=[0.2, 0.4, 1.0]), dict(thresholds=[0.2, 0.4, inf]), dict(thresholds=[-0.1, 0.4, 0.7]),
                 dict(count=img), dict(total=ctypes.c_void_p((1 << 20) + 2 * (96 * 103 + 82))), dict(sumsq=ctypes.c_void_p((1 << 20) - 8)),
                 dict(total=count), dict(sumsq=ctypes.c_void_p((2 << 20) + 4 * 32 * 96 - 4)), dict(sumsq=ctypes.c_void_p((3 << 20) + 8 * 32 * 96 - 8)),
                 dict(total=ctypes.c_void_p((4 << 20) - 8))):
        assert call(**over) == E_ARG, over
        assert 'shg_limb_profile_u16' in _lib.last_error()
    assert call(sectors=8, thresholds=None, count=None) == E_ARG                 # (8 sectors need no table; the null table is the fault)
    assert 'null pointer' in _lib.last_error()


def test_deconvolve_xy_refusals_need_no_gpu():
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(4096)
    taps = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
    five = (ctypes.c_float * 5)(0.1, 0.2, 0.4, 0.2, 0.1)

    def call(img=one, h=8, w=8, pitch=8, kx=taps, rx=1, ky=five, ry=2, iterations=3, out=ctypes.c_void_p(8192), out_pitch=8, ws=ctypes.c_void_p(1 << 16),
             ws_bytes=1 << 20):
        return lib.shg_rl_deconvolve_xy_u16(img, h, w, pitch, kx, rx, ky, ry, iterations, out, out_pitch, None, ws, ws_bytes, None)

    for over in (dict(img=None), dict(kx=None), dict(ky=None), dict(out=None), dict(ws=None), dict(pitch=7), dict(out_pitch=7), dict(rx=-1), dict(rx=17),
                 dict(ry=-1), dict(ry=17), dict(iterations=0), dict(iterations=201), dict(ws_bytes=0), dict(out=one),
                 dict(ky=(ctypes.c_float * 5)(0.1, 0.2, float('nan'), 0.2, 0.1)), dict(ky=(ctypes.c_float * 5)(0.1, 0.2, 0.5, 0.2, 0.1)),
                 dict(kx=(ctypes.c_float * 3)(-0.25, 1.0, 0.25)), dict(kx=(ctypes.c_float * 3)(0.25, 0.5, 0.2))):
        assert call(**over) == E_ARG, over
        assert 'shg_rl_deconvolve_xy_u16' in _lib.last_error()
    for over in (dict(h=0), dict(w=16385)):
        assert call(**over) == E_UNSUPPORTED, over
    assert lib.shg_abi_version() == 16


# ---- the command lines, with the kernels stubbed ----
def test_psf_sigma_parses():
    assert deconvolve.psf_sigma_argument('1.5') == 1.5 and isinstance(deconvolve.psf_sigma_argument('2'), float)
    assert deconvolve.psf_sigma_argument('auto') == 'auto' and deconvolve.psf_sigma_argument('AUTO') == 'auto'
    assert deconvolve.psf_sigma_argument('1.0,2.25') == (1.0, 2.25)
    for bad in ('wide', '1,2,3', '1,', ',', ''):
        with pytest.raises(Exception, match='invalid float value'):
            deconvolve.psf_sigma_argument(bad)


def test_deconvolve_command_line_refusals(monkeypatch, capsys, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, message in ((['x.png', '--psf-sigma', 'auto'], '--psf-sigma auto on a PNG needs --circle cx,cy,rad'),
                          (['x.ser', '--psf-sigma', 'wide'], 'argument --psf-sigma: invalid float value: \'wide\''),
                          (['x.ser', '--psf-sigma', '1,2,3'], 'argument --psf-sigma: invalid float value: \'1,2,3\''),
                          (['x.ser', '--psf-sigma', '1.0,5'], 'sigma lies in'), (['x.ser', '--psf-sigma', '0.1,2'], 'sigma lies in'),
                          (['x.ser', '--psf-sigma', '1,2', '--radius', '17'], 'radius is an integer'),
                          (['x.ser', '--psf-sigma', 'auto', '--iterations', '0'], 'iterations is an integer'),
                          (['no_such_file.ser', '--psf-sigma', 'auto'], 'no such file')):
        with pytest.raises(SystemExit) as exit_info:
            deconvolve.main(argv)
        assert exit_info.value.code == 2
        captured = capsys.readouterr()
        assert message in captured.err and captured.out == '', argv


def test_psf_command_line_refusals(monkeypatch, capsys, tmp_path):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, message in ((['x.png'], 'a PNG needs --circle cx,cy,rad'), (['x.ser', '--reach', '0'], '--reach is 1 to 64'),
                          (['x.ser', '--reach', '65'], '--reach is 1 to 64'), (['x.ser', '--sub', '9'], '--sub is 1 to 8'),
                          (['x.ser', '--sectors', '12'], '--sectors is a multiple of 8 from 8 to 64'),
                          (['x.ser', '--circle', '1,2'], '--circle is cx,cy,rad'), (['x.ser', '-w', '1'], '-w is not a psf flag'),
                          (['no_such_file.ser'], 'no such file'), ([], 'exactly one SER, AVI or PNG file')):
        with pytest.raises(SystemExit) as exit_info:
            psf.main(argv)
        assert exit_info.value.code == 2
        captured = capsys.readouterr()
        assert message in captured.err and captured.out == '', argv
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit):
        psf.main(['x.ser'])
    assert 'measuring the blur is single-process: run it without torchrun' in capsys.readouterr().err


@pytest.fixture
def stubbed(monkeypatch, tmp_path):
    """A PNG that is the (1.0, 2.0) scene, the tables from the restatement, the deconvolution recorded and not run."""
    from solex_ser_recon_en_amd import device, disk, ops
    img = pr.limb_scene(1.0, 2.0, seed=1)
    path = str(tmp_path / 'scene.png')
    open(path, 'wb').close()
    calls = []
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(disk, 'png_input', lambda p, opts: (img, None, p[:-4]))
    monkeypatch.setattr(disk, 'write_image', lambda image, stem, opts, src: (np.asarray(image), stem + '.png', None))
    monkeypatch.setattr(device, 'to_device_u16', lambda image: image)
    monkeypatch.setattr(psf, 'limb_profiles',
                        lambda image, circle, reach=12, sub=4, sectors=32: pr.limb_profile(image, circle, reach, sub, sectors) + (psf.bin_centres(reach, sub),))
    monkeypatch.setattr(ops, 'rl_deconvolve_u16', lambda image, k, n: calls.append(('one', k, n)) or (image, None))
    monkeypatch.setattr(ops, 'rl_deconvolve_xy_u16', lambda image, kx, ky, n: calls.append(('xy', kx, ky, n)) or (image, None))
    return path, calls


def json_line(capsys):
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_deconvolve_auto_reports_what_it_measured(stubbed, capsys):
    path, calls = stubbed
    circle = '%r,%r,%r' % pr.CIRCLE
    assert deconvolve.main([path, '--psf-sigma', 'auto', '--circle', circle, '--iterations', '4']) == 0
    out = json_line(capsys)
    assert set(out['psf']) == {'sigma_x', 'sigma_y', 'isotropic', 'n_used', 'rms'}
    assert abs(out['psf']['sigma_x'] - pr.expected(1.0)) <= pr.TOLERANCE['recovery']
    assert abs(out['psf']['sigma_y'] - pr.expected(2.0)) <= pr.TOLERANCE['recovery']
    assert out['psf_sigma'] == [out['psf']['sigma_x'], out['psf']['sigma_y']] and out['radius'] == [5, 9] and out['iterations'] == 4
    (kind, kx, ky, n), = calls
    assert kind == 'xy' and n == 4 and np.array_equal(kx, deconvolve.gaussian_taps(out['psf']['sigma_x']))
    assert np.array_equal(ky, deconvolve.gaussian_taps(out['psf']['sigma_y'])) and out['taps'] == [[float(v) for v in kx], [float(v) for v in ky]]
    for key in ('input', 'shape', 'flux', 'shift', 'circle', 'ratio', 'png', 'fits', 'contrast'):
        assert key in out


def test_a_pair_goes_the_xy_way_only_when_it_differs(stubbed, capsys):
    path, calls = stubbed
    assert deconvolve.main([path, '--psf-sigma', '1.0,2.0', '--radius', '6']) == 0
    out = json_line(capsys)
    assert 'psf' not in out and out['psf_sigma'] == [1.0, 2.0] and out['radius'] == [6, 6]
    assert calls.pop()[0] == 'xy'
    assert deconvolve.main([path, '--psf-sigma', '1.5,1.5']) == 0
    out = json_line(capsys)
    assert out['psf_sigma'] == [1.5, 1.5] and out['radius'] == 6 and len(out['taps']) == 13
    kind, k, n = calls.pop()
    assert kind == 'one' and np.array_equal(k, deconvolve.gaussian_taps(1.5))
    assert deconvolve.main([path, '--psf-sigma', '1.5']) == 0                # a float: today's line
    out = json_line(capsys)
    assert 'psf' not in out and out['psf_sigma'] == 1.5 and out['radius'] == 6 and calls.pop()[0] == 'one' and not calls
    # the library the same way
    img = pr.limb_scene(1.0, 2.0, seed=1)
    _, rec = deconvolve.deconvolve_disk(img, taps=(dr.gaussian(1.0, 3), dr.gaussian(2.0, 7)), iterations=2)
    assert rec['radius'] == [3, 7] and rec['sigma'] is None and calls.pop()[0] == 'xy'
    _, rec = deconvolve.deconvolve_disk(img, taps=(dr.gaussian(1.0, 3), dr.gaussian(1.0, 3)), iterations=2)
    assert rec['radius'] == 3 and calls.pop()[0] == 'one'
    with pytest.raises(ValueError, match='taps come without sigma and radius'):
        deconvolve.deconvolve_disk(img, sigma=(1.0, 2.0), taps=(dr.gaussian(1.0, 3), dr.gaussian(2.0, 7)))
    with pytest.raises(ValueError, match='sigma lies in'):
        deconvolve.deconvolve_disk(img, sigma=(1.0, 4.5))


def test_psf_command_line_writes_the_profiles(stubbed, capsys):
    path, _ = stubbed
    assert psf.main([path, '--circle', '%r,%r,%r' % pr.CIRCLE, '--sectors', '16']) == 0
    out = json_line(capsys)
    for key in ('input', 'shape', 'shift', 'reach', 'sub', 'sigma_x', 'sigma_y', 'isotropic', 'n_used', 'n_sectors', 'rms', 'fit_seconds',
                'sectors', 'esf', 'circle', 'ratio', 'phi', 'crop'):
        assert key in out, key
    assert out['n_sectors'] == 16 and len(out['sectors']) == 16 and out['circle'] == list(pr.CIRCLE) and out['shift'] is None
    assert set(out['sectors'][0]) == {'theta', 'sigma', 't0', 'residual', 'used', 'why_not'}
    assert abs(out['sigma_x'] - pr.expected(1.0)) <= pr.TOLERANCE['recovery'] and abs(out['sigma_y'] - pr.expected(2.0)) <= pr.TOLERANCE['recovery']
    assert out['esf'] == path[:-4] + '_esf.txt'
    rows = np.loadtxt(out['esf'])
    assert rows.shape == (16 * 96, 6) and np.array_equal(np.unique(rows[:, 0]), np.arange(16.0))
    count, total, _ = pr.limb_profile(pr.limb_scene(1.0, 2.0, seed=1), pr.CIRCLE, 12, 4, 16)
    assert np.array_equal(rows[:, 3].reshape(16, 96), count)
    assert np.abs(rows[:, 5] - rows[:, 4]).max() < 0.02 * pr.DISK            # the model follows the means
