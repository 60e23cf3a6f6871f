"""Sharpening on the GPU: shg_wavelet_sharpen_u16 and shg_wavelet_noise_u16 bit for bit against the restatement written from the
header (tests/sharpen_ref.py) -- images in buffers whose pitch exceeds the width with the padding planted and checked, outputs on
and off 16 bytes, one pixel, one row, one column, images narrower than a hole (repeated reflection), several workgroups on both
axes, every level count (hence every fused form and every carried plane); random, constant, chequerboard and impulse images; gains
0, 1, 16 and mixed, gates 0, mixed and 2^22, clipping both ways; with and without the planes; the noise's empty, one-pixel, odd and
even sets, circles partly off the image, medians on the first and the last value of a coarse bin; every refused argument; and a
scan and a PNG through sharpen_scan and the command line."""
import os
import shutil

import numpy as np
import pytest

from tests import flatten_ref as fr
from tests import sharpen_ref as sr
from tests.linemaps_util import run_json, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
PAD, OUT_FILL, PLANE_FILL, WS_FILL, NOISE_FILL = 0xBEEF, 0x5A5A, 0x7A7A7A7A, 0xA5, 0x7EADBEEF7EADBEEF
GUARD = 5                                   # planted elements around the planes, behind the noise result and the workspace
SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (33, 257), (70, 130), (300, 520)]
MIXED_GAIN = [0, 461, 4096, 256, 100, 700]
MIXED_THR = [50000, 0, 1 << 22, 3000, 64, 1]


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops, sharpen
    from solex_ser_recon_en_amd._lib import lib
    return sharpen, ops, lib


def up16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.uint16)


def down16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def padded(img, extra, fill=PAD):
    h, w = img.shape
    buf = np.full((h, w + extra), fill, np.uint16)
    buf[:, :w] = img
    return up16(buf)


def i32(values):
    return np.ascontiguousarray(values, dtype=np.int32)


def call_sharpen(lib, img, gain_q8, thr_q6, planes=False, extra=3, out_extra=1, skew=0, **over):
    """shg_wavelet_sharpen_u16 on the image in a padded buffer into planted outputs; skew: the output starts that many elements into
    its buffer -> (status, out [h, w], planes [L + 1, h, w] or None, everything else intact)."""
    h, w = img.shape
    levels = over.pop('levels', len(gain_q8))
    buf = padded(img, extra)
    out_pitch = w + out_extra
    out = up16(np.full(h * out_pitch + skew + 8, OUT_FILL))
    n_planes = (max(levels, 0) + 1) * h * w
    pl = torch.full((n_planes + 2 * GUARD,), PLANE_FILL, dtype=torch.int32, device='cuda')
    need = lib.shg_wavelet_workspace_bytes(h, w, levels) or lib.shg_wavelet_workspace_bytes(h, w, 1)
    ws = torch.full((need + GUARD,), WS_FILL, dtype=torch.uint8, device='cuda')
    g, t = i32(gain_q8), i32(thr_q6)
    st = lib.shg_wavelet_sharpen_u16(over.get('img_ptr', buf.data_ptr()), over.get('h', h), over.get('w', w), over.get('pitch', w + extra), levels,
                                     over.get('gain', g.ctypes.data), over.get('thr', t.ctypes.data), over.get('out', out.data_ptr() + 2 * skew),
                                     over.get('out_pitch', out_pitch), over.get('planes', pl.data_ptr() + 4 * GUARD if planes else None),
                                     over.get('ws', ws.data_ptr()), over.get('ws_bytes', need), None)
    torch.cuda.synchronize()
    got, got_p, got_ws = down16(out), pl.cpu().numpy(), ws.cpu().numpy()
    plane = got[skew:skew + h * out_pitch].reshape(h, out_pitch)
    intact = (got[:skew] == OUT_FILL).all() and (got[skew + (h - 1) * out_pitch + w:] == OUT_FILL).all() and (plane[:, w:][:-1] == OUT_FILL).all()
    intact = intact and (got_p[:GUARD] == PLANE_FILL).all() and (got_p[GUARD + n_planes:] == PLANE_FILL).all() and (got_ws[need:] == WS_FILL).all()
    if st != 0 or not planes:
        intact = intact and (got_p == PLANE_FILL).all()
    if st != 0:
        intact = intact and (got == OUT_FILL).all() and (got_ws == WS_FILL).all()
    back = down16(buf)
    assert np.array_equal(back[:, :w], img) and (back[:, w:] == PAD).all(), 'the image changed'
    got_planes = got_p[GUARD:GUARD + n_planes].reshape(levels + 1, h, w).copy() if planes and st == 0 else None
    return st, plane[:, :w].copy(), got_planes, bool(intact)


def check(lib, img, ref_planes, gain_q8, thr_q6, **how):
    want = sr.recombine(ref_planes, gain_q8, thr_q6)
    st, got, got_planes, intact = call_sharpen(lib, img, gain_q8, thr_q6, **how)
    assert st == 0 and intact
    bad = np.argwhere(got != want)
    assert bad.size == 0, '%d pixels differ, first at %s: %d vs %d' % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    if got_planes is not None:
        bad = np.argwhere(got_planes != ref_planes)
        assert bad.size == 0, '%d plane values differ, first at %s: %d vs %d' % (len(bad), bad[0], got_planes[tuple(bad[0])], ref_planes[tuple(bad[0])])
    return want


def images(h, w):
    rng = np.random.default_rng([h, w])
    impulse = np.zeros((h, w), np.uint16)
    impulse[h // 2, w // 3] = 65535
    return {'random': rng.integers(0, 65536, (h, w)).astype(np.uint16), 'zeros': np.zeros((h, w), np.uint16),
            'full': np.full((h, w), 65535, np.uint16), 'board': ((np.add.outer(np.arange(h), np.arange(w)) % 2) * 65535).astype(np.uint16),
            'impulse': impulse}


# ---- sharpen ----
@pytest.mark.parametrize('levels', [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_sharpen_matches_the_restatement(mods, shape, levels):
    _, _, lib = mods
    h, w = shape
    unity, zero = [256] * levels, [0] * levels
    for k, (name, img) in enumerate(images(h, w).items()):
        ref = sr.wavelet_planes(img, levels)
        lay = dict(skew=k % 2, out_extra=7 - k, extra=1 + k)
        assert np.array_equal(check(lib, img, ref, unity, zero, planes=True, **lay), img), name      # the identity, and the planes
        check(lib, img, ref, MIXED_GAIN[:levels], MIXED_THR[:levels], **lay)
        check(lib, img, ref, [4096] * levels, zero, planes=k % 2 == 0, **lay)
        if name == 'random':
            check(lib, img, ref, [0] * levels, zero, **lay)
            gated = check(lib, img, ref, MIXED_GAIN[:levels], [1 << 22] * levels, **lay)
            assert np.array_equal(gated, ((ref[levels].astype(np.int64) + 32) >> 6).astype(np.uint16))
            check(lib, img, ref, MIXED_GAIN[::-1][:levels], MIXED_THR[::-1][:levels], planes=True, skew=1 - k % 2)
            if h * w >= 35:                                              # sixteen times the detail clips both ways
                loud = sr.recombine(ref, [4096] * levels, zero)
                assert (loud == 0).any() and (loud == 65535).any()
                acc = 256 * ref[levels].astype(np.int64) + 4096 * ref[:levels].astype(np.int64).sum(axis=0)
                assert acc.min() < -8192 and acc.max() > 65535 << 14
        if name == 'board' and min(h, w) > 1:
            assert (np.abs(ref[0]) == 32 * 65535).all()


def test_aligned_rows_and_shared_workspace(mods):
    """Rows on 16 bytes in and out, and one workspace of the largest size serving every level count and the noise call in turn."""
    _, ops, lib = mods
    img = images(70, 130)['random']
    ws = torch.empty(lib.shg_wavelet_workspace_bytes(70, 130, 6), dtype=torch.uint8, device='cuda')
    view = padded(img, 6)[:, :130]
    assert view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0
    for levels in (6, 3, 4, 1, 5, 2):
        out = ops.pitched_u16(70, 130, 'cuda', 8)
        got, planes = ops.wavelet_sharpen_u16(view, MIXED_GAIN[:levels], MIXED_THR[:levels], out=out, want_planes=True, workspace=ws)
        ref = sr.wavelet_planes(img, levels)
        assert got is out and np.array_equal(down16(got), sr.recombine(ref, MIXED_GAIN[:levels], MIXED_THR[:levels]))
        assert planes.dtype == torch.int32 and np.array_equal(planes.cpu().numpy(), ref)
        assert tuple(ops.wavelet_noise_u16(view, (60.0, 30.0, 25.0), workspace=ws).cpu().tolist()) == sr.noise(img, (60.0, 30.0, 25.0))


def test_sharpen_refusals_leave_everything_untouched(mods):
    _, _, lib = mods
    img = images(20, 22)['random']
    gains, thr = [256, 300, 200, 256], [0, 10, 0, 0]

    def refused(code, g=gains, t=thr, **over):
        st, _, _, intact = call_sharpen(lib, img, g, t, planes=over.pop('with_planes', True), **over)
        assert st == code and intact, over

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        refused(E_UNSUPPORTED, **over)
    need = lib.shg_wavelet_workspace_bytes(20, 22, 4)
    for over in (dict(img_ptr=None), dict(gain=None), dict(thr=None), dict(out=None), dict(ws=None), dict(pitch=21), dict(out_pitch=21),
                 dict(levels=0), dict(levels=7), dict(levels=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        refused(E_ARG, **over)
    for j in range(4):
        for bad_g, bad_t in ((-1, 0), (4097, 0), (256, -1), (256, (1 << 22) + 1)):
            g, t = list(gains), list(thr)
            g[j], t[j] = bad_g, bad_t
            refused(E_ARG, g, t)
    # an output or planes on the image, on its last element, and on each other
    buf = padded(img, 1)
    last = buf.data_ptr() + 2 * (19 * 23 + 21)
    out = up16(np.full(20 * 23, OUT_FILL))
    pl = torch.full((5 * 20 * 22,), PLANE_FILL, dtype=torch.int32, device='cuda')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    g, t = i32(gains), i32(thr)
    for o, p in ((buf.data_ptr(), None), (last, None), (out.data_ptr(), last - 2), (out.data_ptr(), buf.data_ptr() - 4 * 5 * 20 * 22 + 4),
                 (out.data_ptr(), out.data_ptr()), (pl.data_ptr() + 4 * (5 * 20 * 22 - 1), pl.data_ptr())):
        assert lib.shg_wavelet_sharpen_u16(buf.data_ptr(), 20, 22, 23, 4, g.ctypes.data, t.ctypes.data, o, 23, p, ws.data_ptr(), need, None) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(down16(buf)[:, :22], img) and (down16(out) == OUT_FILL).all() and (pl.cpu().numpy() == PLANE_FILL).all()


# ---- noise ----
def call_noise(lib, img, circle='none', extra=3, **over):
    """-> (status, (median, n), the guard behind the result, the padding and, on an error, the result itself intact)."""
    h, w = img.shape
    buf = padded(img, extra)
    res = torch.from_numpy(np.full(2 + GUARD, NOISE_FILL, np.uint64).view(np.int64)).cuda()
    need = lib.shg_wavelet_workspace_bytes(h, w, 1)
    ws = torch.full((need + GUARD,), WS_FILL, dtype=torch.uint8, device='cuda')
    c3 = None if circle == 'none' else np.ascontiguousarray([float(v) for v in circle], dtype=np.float64)
    st = lib.shg_wavelet_noise_u16(over.get('img_ptr', buf.data_ptr()), over.get('h', h), over.get('w', w), over.get('pitch', w + extra),
                                   None if c3 is None else c3.ctypes.data, over.get('out2', res.data_ptr()), over.get('ws', ws.data_ptr()),
                                   over.get('ws_bytes', need), None)
    torch.cuda.synchronize()
    got, got_ws = res.cpu().numpy().view(np.uint64), ws.cpu().numpy()
    intact = (got[2 if st == 0 else 0:] == NOISE_FILL).all() and (got_ws[need:] == WS_FILL).all() and (st == 0 or (got_ws == WS_FILL).all())
    back = down16(buf)
    assert np.array_equal(back[:, :w], img) and (back[:, w:] == PAD).all()
    return st, (int(got[0]), int(got[1])), bool(intact)


def check_noise(lib, img, circle='none'):
    want = sr.noise(img, None if circle == 'none' else circle)
    st, got, intact = call_noise(lib, img, circle)
    assert st == 0 and intact and got == want, (got, want)
    return want


NOISE_CASES = [  # (name, h, w, circle, pixels or None)
    ('1x1', 1, 1, 'none', 1), ('1x9', 1, 9, 'none', 9), ('9x1', 9, 1, (-1, -1, -1), 9), ('even', 6, 7, 'none', 42), ('odd', 5, 7, 'none', 35),
    ('off_image', 40, 37, (200.0, 200.0, 20.0), 0), ('one_pixel', 40, 37, (20.0, 15.0, 0.0), 1), ('between_pixels', 40, 37, (20.5, 15.5, 0.5), 0),
    ('five', 40, 37, (20.0, 15.0, 1.0), 5), ('two', 40, 37, (20.5, 15.0, 0.5), 2), ('partly_off', 70, 130, (-10.0, 30.5, 40.0), None),
    ('corner', 70, 130, (129.0, 69.0, 12.3), None), ('tiles', 300, 520, 'none', 300 * 520), ('tiles_disk', 300, 520, (250.3, 140.6, 133.3), None),
    ('covers_all', 33, 257, (128.0, 16.0, 1000.0), 33 * 257),
]


@pytest.mark.parametrize('case', NOISE_CASES, ids=[c[0] for c in NOISE_CASES])
def test_noise_matches_the_restatement(mods, case):
    _, _, lib = mods
    name, h, w, circle, pixels = case
    for kind in ('random', 'quiet'):
        rng = np.random.default_rng([h, w, len(kind)])
        img = (rng.integers(0, 65536, (h, w)) if kind == 'random' else 30000 + rng.integers(-40, 41, (h, w))).astype(np.uint16)
        median, n = check_noise(lib, img, circle)
        assert pixels is None or n == pixels
    if name == 'partly_off':
        assert 0 < n < 70 * 130


def test_noise_of_constant_images_and_bin_edges(mods):
    _, _, lib = mods
    for value in (0, 777, 65535):
        assert check_noise(lib, np.full((20, 31), value, np.uint16), (15.0, 10.0, 8.0))[0] == 0
    # one impulse v on zero: w_1 = 55 v under it, so a one-pixel set reads 55 v: the first and the last value of a coarse bin of 2048
    for v, low in ((2048, 0), ((-pow(55, -1, 2048)) % 2048 + 2048, 2047), (65535, None)):
        img = np.zeros((20, 31), np.uint16)
        img[10, 15] = v
        median, n = check_noise(lib, img, (15.0, 10.0, 0.0))
        assert n == 1 and median == 55 * v and (low is None or median % 2048 == low)
    # and whole images whose median of 90 values is the first value of a coarse bin, and the last of the one before
    for seed, want in ((25, 2048), (5308, 2047)):
        img = np.random.default_rng([77, seed]).integers(0, 200, (9, 10)).astype(np.uint16)
        assert check_noise(lib, img) == (want, 90)
    # the largest |w_1|
    board = images(12, 14)['board']
    assert check_noise(lib, board) == (32 * 65535, 12 * 14)


def test_noise_refusals_leave_everything_untouched(mods):
    _, _, lib = mods
    img = images(20, 22)['random']
    need = lib.shg_wavelet_workspace_bytes(20, 22, 1)
    for over, code in ((dict(h=0), E_UNSUPPORTED), (dict(w=16385), E_UNSUPPORTED), (dict(img_ptr=None), E_ARG), (dict(out2=None), E_ARG),
                       (dict(ws=None), E_ARG), (dict(pitch=21), E_ARG), (dict(ws_bytes=need - 1), E_ARG)):
        st, _, intact = call_noise(lib, img, **over)
        assert st == code and intact, over
    for circle in ((float('nan'), 1.0, 5.0), (1.0, float('inf'), 5.0), (1.0, 1.0, float('nan')), (1.0, 1.0, float('-inf'))):
        st, _, intact = call_noise(lib, img, circle)
        assert st == E_ARG and intact


# ---- the Python layer ----
def test_sharpen_disk_and_planes(mods):
    sharpen, ops, _ = mods
    img, _, circle, sigma, _ = sr.scene()
    dev = up16(img)
    est, median, pixels = sharpen.estimate_sigma(dev, circle)
    want_median, want_pixels = sr.noise(img, (circle[0], circle[1], circle[2] * 0.9))
    assert (median, pixels) == (want_median, want_pixels) and est == sharpen.sigma_from_median(want_median)
    print('sigma %.3f for %.3f planted' % (est, sigma))
    assert abs(est / sigma - 1.0) <= sr.TOLERANCE['sigma']
    out, rec = sharpen.sharpen_disk(dev, sharpen.DEFAULT_GAINS, sharpen.DEFAULT_DENOISE, circle=circle)
    thr = sharpen.thresholds(est, sharpen.DEFAULT_DENOISE, 4)
    assert rec['gain_q8'] == [256, 461, 358, 256] and rec['threshold_q6'] == thr.tolist() and rec['sigma'] == est and rec['pixels'] == pixels
    assert rec['levels'] == 4 and rec['median_q6'] == median and rec['thresholds'] == (thr / 64.0).tolist() and thr[0] > thr[1] > 0 == thr[2]
    assert np.array_equal(down16(out), sr.sharpen(img, rec['gain_q8'], thr)[0])
    out, rec = sharpen.sharpen_disk(dev, [1, 2], (1,), sigma=100.0)
    assert rec['pixels'] is None and rec['median_q6'] is None and rec['denoise'] == [1.0, 0.0]
    assert np.array_equal(down16(out), sr.sharpen(img, [256, 512], sharpen.thresholds(100.0, (1,), 2))[0])
    planes = sharpen.wavelet_planes(dev, 5)
    assert np.array_equal(planes.cpu().numpy(), sr.wavelet_planes(img, 5))
    measures = sr.scene_measures(lambda im, c: sharpen.estimate_sigma(up16(im), c)[0],
                                 lambda im, c: down16(sharpen.sharpen_disk(up16(im), [1] * 4, sharpen.DEFAULT_DENOISE, circle=c)[0]))
    assert measures['sigma'] <= sr.TOLERANCE['sigma'] and measures['residual'] <= sr.TOLERANCE['residual']
    with pytest.raises(ValueError):
        ops.wavelet_sharpen_u16(dev, [256] * 7)
    with pytest.raises(ValueError):
        ops.wavelet_sharpen_u16(dev, [256, 5000])
    with pytest.raises(ValueError):
        ops.wavelet_sharpen_u16(dev, [256], out=dev[:-1])
    with pytest.raises(RuntimeError, match='overlaps'):
        ops.wavelet_sharpen_u16(dev, [256], out=dev)
    with pytest.raises(RuntimeError):
        ops.wavelet_noise_u16(torch.zeros((4, 4), dtype=torch.uint16))


# ---- end to end: a scan, and a PNG ----
@pytest.fixture(scope='module')
def scan(mods, tmp_path_factory):
    sharpen = mods[0]
    path = write_scan(tmp_path_factory, 'sharpen', fr.pipeline_scan())
    return {'path': path, 'res': sharpen.sharpen_scan(path)}


def test_sharpen_scan_is_the_restatement_of_its_disk(mods, scan):
    from solex_ser_recon_en_amd import SHG_MAIN, stack
    sharpen = mods[0]
    res = scan['res']
    disk = stack.scan_disk(scan['path'])
    image = down16(disk['image'])
    assert np.array_equal(down16(res['image']), image) and res['circle'] == disk['circle']
    rec = res['record']
    cx, cy, rad = res['circle']
    median, pixels = sr.noise(image, (cx, cy, rad * 0.9))
    assert (rec['median_q6'], rec['pixels']) == (median, pixels) and pixels > 1000
    thr = sharpen.thresholds(sharpen.sigma_from_median(median), sharpen.DEFAULT_DENOISE, 4)
    assert rec['threshold_q6'] == thr.tolist() and rec['gain_q8'] == [256, 461, 358, 256]
    assert np.array_equal(down16(res['sharp']), sr.sharpen(image, rec['gain_q8'], thr)[0])
    assert (down16(res['sharp']) != image).any()
    with pytest.raises(ValueError, match='circle'):
        sharpen.sharpen_scan(scan['path'], dict(SHG_MAIN.default_options(), ratio_fixe=1.0))


def test_command_line(mods, scan, tmp_path, capsys):
    from solex_ser_recon_en_amd import SHG_MAIN
    from solex_ser_recon_en_amd.fits_io import read_fits_u16
    from solex_ser_recon_en_amd.png_io import read_png_gray
    sharpen = mods[0]
    work = str(tmp_path / 'scan.ser')
    shutil.copy(scan['path'], work)
    res = scan['res']
    k = SHG_MAIN.default_options()['img_rotate'] // 90
    want = np.rot90(down16(res['sharp']), k)
    out = run_json(sharpen.main, capsys, [work, '--contrast', '-f'])
    base = work[:-4] + '_shift=0_sharp'
    assert out['png'] == base + '.png' and out['fits'] == base + '.fits' and out['contrast'] == base and out['input'] == work
    assert np.array_equal(read_png_gray(out['png']), want) and np.array_equal(read_fits_u16(out['fits'])[0], want)
    for suffix in ('_clahe.png', '_protus.png', '_uncontrasted.png', '_high_contrast.png', '_clahe.fits'):
        assert os.path.exists(base + suffix), suffix
    assert np.array_equal(read_png_gray(base + '_uncontrasted.png'), want)
    rec = res['record']
    assert out['shape'] == list(want.shape) and out['levels'] == 4 and out['gains'] == rec['gains'] == [1.0, 461 / 256.0, 358 / 256.0, 1.0]
    assert out['sigma'] == rec['sigma'] and out['median'] == rec['median_q6'] / 64.0 and out['pixels'] == rec['pixels']
    assert out['thresholds'] == rec['thresholds'] and out['denoise'] == [3.0, 1.0, 0.0, 0.0] and out['shift'] == 0
    assert out['circle'] == list(res['circle']) and out['ratio'] == res['ratio']
    # a PNG the package wrote, other layers, a given sigma, the noise circle; shorter lists are padded
    png = str(tmp_path / 'disk_uncontrasted.png')
    shutil.copy(base + '_uncontrasted.png', png)
    out = run_json(sharpen.main, capsys, [png, '--levels', '5', '--gains', '1,2.5', '--denoise', '2', '--sigma', '150'])
    assert out['png'] == png[:-4] + '_sharp.png' and out['fits'] is None and out['contrast'] is None and out['shift'] is None
    assert out['levels'] == 5 and out['gains'] == [1.0, 2.5, 1.0, 1.0, 1.0] and out['denoise'] == [2.0, 0.0, 0.0, 0.0, 0.0]
    assert out['sigma'] == 150.0 and out['median'] is None and out['pixels'] is None and out['circle'] == [-1, -1, -1]
    thr = sharpen.thresholds(150.0, (2,), 5)
    assert out['thresholds'] == (thr / 64.0).tolist()
    assert np.array_equal(read_png_gray(out['png']), sr.sharpen(want, [256, 640, 256, 256, 256], thr)[0])
    out = run_json(sharpen.main, capsys, [png, '--circle', '150,200,100', '--region', '0.5', '--contrast'])
    median, pixels = sr.noise(want, (150.0, 200.0, 50.0))
    assert out['median'] == median / 64.0 and out['pixels'] == pixels and out['sigma'] == sharpen.sigma_from_median(median)
    assert out['circle'] == [150.0, 200.0, 100.0] and os.path.exists(png[:-4] + '_sharp_clahe.png')
    whole = run_json(sharpen.main, capsys, [png])
    assert whole['pixels'] == want.size and whole['sigma'] == sharpen.sigma_from_median(sr.noise(want)[0]) > 0
    assert sharpen.main([work, '-x']) == 1                                         # no limb fit, no circle
    assert 'circle' in capsys.readouterr().err
    assert sharpen.main([work, '--circle', '1,2,3']) == 1
    assert 'PNG' in capsys.readouterr().err
