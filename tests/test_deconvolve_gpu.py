"""Deconvolution on the GPU: shg_rl_deconvolve_u16 bit for bit against the restatement written from the header
(tests/deconvolve_ref.py) -- the uint16 output and the float32 estimate compared as integers --: images in buffers whose pitch
exceeds the width with the padding planted and checked, outputs on and off 16 bytes, guards around the estimate and behind the
workspace, one pixel, one row, one column, an image narrower than the radius (repeated reflection), several workgroups on both axes;
radii 0, 1, 3, 6 and 16 (every padded radius the kernel is built for), 1, 2, 3 and 7 iterations; random, zero, full, chequerboard and
impulse images and a disk on a sky of exactly 0 (the flush); Gaussian, asymmetric and zero-padded taps; every refused argument; and a
scan and a PNG through deconvolve_scan and the command line."""
import os
import shutil

import numpy as np
import pytest

from solex_ser_recon_en_amd import deconvolve as _deconvolve  # noqa: F401  (no feature: no tests)
from tests import deconvolve_ref as dr
from tests import flatten_ref as fr
from tests.linemaps_util import run_json, write_scan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

E_ARG, E_UNSUPPORTED = -1, -3
PAD, OUT_FILL, EST_FILL, WS_FILL = 0xBEEF, 0x5A5A, 0x7A7A7A7A, 0xA5
GUARD = 5                                   # planted elements around the estimate and behind the workspace
SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (33, 257), (70, 130), (300, 520)]
RADII = [0, 1, 3, 6, 16]
ITERATIONS = [1, 2, 3, 7]
SIGMA_OF = {0: 1.0, 1: 0.6, 3: 1.0, 6: 1.5, 16: 4.0}


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import deconvolve, ops
    from solex_ser_recon_en_amd._lib import lib
    return deconvolve, ops, lib


def up16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda().view(torch.uint16)


def down16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def padded(img, extra, fill=PAD):
    h, w = img.shape
    buf = np.full((h, w + extra), fill, np.uint16)
    buf[:, :w] = img
    return up16(buf)


def f32(values):
    return np.ascontiguousarray(values, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def asymmetric(radius):
    """Taps that are not their own reverse: a Gaussian times a ramp, normalised in float64."""
    if radius == 0:
        return f32([1.0])
    k = dr.gaussian(SIGMA_OF[radius], radius).astype(np.float64) * np.linspace(0.5, 1.5, 2 * radius + 1)
    k = (k / k.sum()).astype(np.float32)
    assert not np.array_equal(k, k[::-1])
    return k


def call_rl(lib, img, taps, iterations, estimate=True, extra=3, out_extra=1, skew=0, **over):
    """shg_rl_deconvolve_u16 on the image in a padded buffer into planted outputs; skew: the output starts that many elements into
    its buffer -> (status, out [h, w], estimate [h, w] or None, everything else intact)."""
    h, w = img.shape
    k = f32(taps)
    buf = padded(img, extra)
    out_pitch = w + out_extra
    out = up16(np.full(h * out_pitch + skew + 8, OUT_FILL))
    est = torch.full((h * w + 2 * GUARD,), EST_FILL, dtype=torch.int32, device='cuda')
    need = lib.shg_rl_workspace_bytes(h, w)
    ws = torch.full((need + GUARD,), WS_FILL, dtype=torch.uint8, device='cuda')
    st = lib.shg_rl_deconvolve_u16(over.get('img_ptr', buf.data_ptr()), over.get('h', h), over.get('w', w), over.get('pitch', w + extra),
                                   over.get('taps_ptr', k.ctypes.data), over.get('radius', k.size // 2), iterations,
                                   over.get('out', out.data_ptr() + 2 * skew), over.get('out_pitch', out_pitch),
                                   over.get('estimate', est.data_ptr() + 4 * GUARD if estimate else None), over.get('ws', ws.data_ptr()),
                                   over.get('ws_bytes', need), None)
    torch.cuda.synchronize()
    got, got_e, got_ws = down16(out), est.cpu().numpy(), ws.cpu().numpy()
    plane = got[skew:skew + h * out_pitch].reshape(h, out_pitch)
    intact = (got[:skew] == OUT_FILL).all() and (got[skew + (h - 1) * out_pitch + w:] == OUT_FILL).all() and (plane[:, w:][:-1] == OUT_FILL).all()
    intact = intact and (got_e[:GUARD] == EST_FILL).all() and (got_e[GUARD + h * w:] == EST_FILL).all() and (got_ws[need:] == WS_FILL).all()
    if st != 0 or not estimate:
        intact = intact and (got_e == EST_FILL).all()
    if st != 0:
        intact = intact and (got == OUT_FILL).all() and (got_ws == WS_FILL).all()
    back = down16(buf)
    assert np.array_equal(back[:, :w], img) and (back[:, w:] == PAD).all(), 'the image changed'
    got_est = got_e[GUARD:GUARD + h * w].reshape(h, w).copy() if estimate and st == 0 else None
    return st, plane[:, :w].copy(), got_est, bool(intact)


def check(lib, img, taps, iterations, want=None, **how):
    """The call against the restatement (want: e_N of the restatement when the caller has it already) -> e_N."""
    e = dr.iterate(img, taps, iterations) if want is None else want
    st, got, got_est, intact = call_rl(lib, img, taps, iterations, **how)
    assert st == 0 and intact
    ref = dr.finish(e)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, '%d pixels differ, first at %s: %d vs %d' % (len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
    if got_est is not None:
        bad = np.argwhere(got_est != bits(e))
        assert bad.size == 0, '%d estimates differ, first at %s: %r vs %r' % (len(bad), bad[0], got_est.view(np.float32)[tuple(bad[0])],
                                                                              e[tuple(bad[0])])
    return e


def images(h, w):
    rng = np.random.default_rng([h, w])
    impulse = np.zeros((h, w), np.uint16)
    impulse[h // 2, w // 3] = 65535
    return {'random': rng.integers(0, 65536, (h, w)).astype(np.uint16), 'zeros': np.zeros((h, w), np.uint16),
            'full': np.full((h, w), 65535, np.uint16), 'board': ((np.add.outer(np.arange(h), np.arange(w)) % 2) * 65535).astype(np.uint16),
            'impulse': impulse, 'disk': dr.zero_sky_disk(h, w)}


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_deconvolve_matches_the_restatement(mods, shape):
    """Small images: every image with every radius.  The three that span several workgroups: the random image with every radius, the
    others with one radius each, the radii and the iteration counts taking turns."""
    _, _, lib = mods
    h, w = shape
    small = h * w < 1000
    turn = SHAPES.index(shape)
    for k, (name, img) in enumerate(images(h, w).items()):
        radii = RADII if small or name == 'random' else [RADII[(k + turn) % len(RADII)]]
        for j, radius in enumerate(radii):
            n = ITERATIONS[(k + j + turn) % len(ITERATIONS)]
            lay = dict(skew=(k + j) % 2, out_extra=7 - k, extra=1 + k, estimate=(k + j) % 3 != 2)
            e = check(lib, img, dr.gaussian(SIGMA_OF[radius], radius), n, **lay)
            if name in ('zeros', 'full') and radius == 0:
                assert np.array_equal(e, img.astype(np.float32))
            if name == 'zeros':
                assert (bits(e) == 0).all()
            if small or name in ('random', 'disk'):
                check(lib, img, asymmetric(radius), n, **lay)


@pytest.mark.parametrize('case', [(90, 100, 20), (300, 520, 7)], ids=['90x100', '300x520'])
def test_the_flush_is_on_the_path(mods, case):
    """A disk whose sky is exactly 0 and whose faint rim dies beside the limb: estimates are flushed to 0, none is left below 2^-20."""
    _, _, lib = mods
    h, w, n = case
    disk = dr.zero_sky_disk(h, w)
    e = dr.iterate(disk, dr.gaussian(1.5, 6), n)
    assert ((disk > 0) & (e == 0)).any() and not ((e > 0) & (e < dr.FLUSH)).any() and (e[disk == 0] == 0).all()
    check(lib, disk, dr.gaussian(1.5, 6), n, want=e)


@pytest.mark.parametrize('shape', [(7, 5), (70, 130)], ids=['7x5', '70x130'])
def test_zero_padded_taps_change_no_bit(mods, shape):
    """Taps of radius 1 and 3 padded with zeros to every larger radius -- hence through every padded radius the kernel is built for --
    against the restatement of the unpadded taps."""
    _, _, lib = mods
    img = images(*shape)['random']
    for taps in (asymmetric(1), dr.gaussian(1.0, 3)):
        want = dr.iterate(img, taps, 3)
        for radius in (2, 3, 5, 6, 7, 10, 11, 16):
            if radius >= taps.size // 2:
                check(lib, img, dr.pad_taps(taps, radius), 3, want=want, skew=radius % 2)


def test_tap_and_value_extremes(mods):
    """The smallest tap, a tap of exactly 1 off centre (a shift), taps whose sum is near either end of the range, and 200 iterations."""
    _, _, lib = mods
    img = images(33, 257)['random']
    tiny = f32([2.0 ** -30, 1.0 - 2.0 ** -24, 2.0 ** -30])
    check(lib, img, tiny, 3)
    check(lib, img, f32([0, 0, 0, 1, 0]), 2)
    for scale in (1.0 - 0.9 * 2.0 ** -10, 1.0 + 0.9 * 2.0 ** -10):
        k = f32(dr.gaussian(1.0, 3).astype(np.float64) * scale)
        assert 0.8 * 2.0 ** -10 < abs(float(k.astype(np.float64).sum()) - 1.0) <= 2.0 ** -10
        check(lib, img, k, 3)
    small = images(20, 22)['disk']
    check(lib, small, dr.gaussian(1.0, 3), 200)


def test_aligned_rows_and_shared_workspace(mods):
    """Rows on 16 bytes in and out through ops.rl_deconvolve_u16 with the caller's out, and one workspace of the largest size
    serving every shape in turn."""
    _, ops, lib = mods
    ws = torch.full((lib.shg_rl_workspace_bytes(300, 520) + GUARD,), WS_FILL, dtype=torch.uint8, device='cuda')
    taps = asymmetric(3)
    for h, w in ((300, 520), (7, 5), (70, 130), (1, 9), (33, 257)):
        img = images(h, w)['random']
        view = padded(img, (-w) % 8 + 8)[:, :w]
        assert view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0
        out = ops.pitched_u16(h, w, 'cuda', 8)
        got, est = ops.rl_deconvolve_u16(view, taps, 2, out=out, want_estimate=True, workspace=ws)
        want, e = dr.deconvolve(img, taps, 2)
        assert got is out and np.array_equal(down16(got), want)
        assert est.dtype == torch.float32 and tuple(est.shape) == (h, w) and np.array_equal(bits(est.cpu().numpy()), bits(e))
        assert np.array_equal(down16(view), img)
    assert (ws.cpu().numpy()[-GUARD:] == WS_FILL).all()
    got, est = ops.rl_deconvolve_u16(up16(img), taps, 2)
    assert est is None and np.array_equal(down16(got), want)


def test_refusals_leave_everything_untouched(mods):
    _, ops, lib = mods
    img = images(20, 22)['random']
    taps = dr.gaussian(1.0, 3)

    def refused(code, k=taps, n=3, **over):
        st, _, _, intact = call_rl(lib, img, k, n, **over)
        assert st == code and intact, over

    for over in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385)):
        refused(E_UNSUPPORTED, **over)
    need = lib.shg_rl_workspace_bytes(20, 22)
    for over in (dict(img_ptr=None), dict(taps_ptr=None), dict(out=None), dict(ws=None), dict(pitch=21), dict(out_pitch=21), dict(radius=-1),
                 dict(radius=17), dict(n=0), dict(n=201), dict(n=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        refused(E_ARG, **over)
    for j, bad in ((0, float('nan')), (3, float('inf')), (2, -0.25), (1, 2.0 ** -31), (3, 1.5), (3, 0.2), (6, 0.3)):
        k = taps.copy()
        k[j] = bad
        refused(E_ARG, k)
    refused(E_ARG, np.zeros(7, np.float32))
    # an output, an estimate or a workspace on the image, on its last element, and on each other
    buf = padded(img, 1)
    last = buf.data_ptr() + 2 * (19 * 23 + 21)
    out = up16(np.full(20 * 23, OUT_FILL))
    est = torch.full((20 * 22,), EST_FILL, dtype=torch.int32, device='cuda')
    ws = torch.full((need,), WS_FILL, dtype=torch.uint8, device='cuda')
    o, e, s = out.data_ptr(), est.data_ptr(), ws.data_ptr()
    for oo, ee, ss in ((buf.data_ptr(), e, s), (last, e, s), (o, last - 2, s), (o, buf.data_ptr() - 4 * 20 * 22 + 4, s), (o, e, last),
                       (o, e, buf.data_ptr() - need + 2), (o, o, s), (o, o + 2 * (19 * 23 + 21), s),
                       (o, e, o), (o, e, e), (o, e, e + 4 * (20 * 22 - 1)), (o, s + need - 4, s)):
        assert lib.shg_rl_deconvolve_u16(buf.data_ptr(), 20, 22, 23, taps.ctypes.data, 3, 3, oo, 23, ee, ss, need, None) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(down16(buf)[:, :22], img) and (down16(out) == OUT_FILL).all() and (est.cpu().numpy() == EST_FILL).all()
    assert (ws.cpu().numpy() == WS_FILL).all()
    dev = up16(img)
    for bad in (dict(taps=[0.5, 0.5]), dict(taps=np.full(35, 1.0 / 35)), dict(taps=[0.2, 0.5, 0.2]), dict(taps=[-0.5, 1.0, 0.5]), dict(n=0),
                dict(n=201), dict(n=2.5), dict(out=dev[:-1])):
        with pytest.raises(ValueError):
            ops.rl_deconvolve_u16(dev, bad.get('taps', taps), bad.get('n', 3), out=bad.get('out'))
    with pytest.raises(RuntimeError, match='overlaps'):
        ops.rl_deconvolve_u16(dev, taps, 3, out=dev)
    with pytest.raises(RuntimeError):
        ops.rl_deconvolve_u16(torch.zeros((4, 4), dtype=torch.uint16), taps, 3)


# ---- the Python layer ----
def test_deconvolve_disk_and_the_accuracy(mods):
    deconvolve = mods[0]
    img, _, _ = dr.scene()
    dev = up16(img)
    out, rec = deconvolve.deconvolve_disk(dev, 1.5, 10, radius=6)
    assert rec == {'sigma': 1.5, 'radius': 6, 'taps': [float(v) for v in dr.gaussian(1.5, 6)], 'iterations': 10}
    assert np.array_equal(down16(out), dr.deconvolve(img, dr.gaussian(1.5, 6), 10)[0])
    out, rec = deconvolve.deconvolve_disk(dev)
    assert rec['sigma'] == 1.2 and rec['radius'] == 5 and rec['iterations'] == 10
    assert np.array_equal(down16(out), dr.deconvolve(img, deconvolve.gaussian_taps(1.2), 10)[0])
    out, rec = deconvolve.deconvolve_disk(dev, taps=[0.5, 0.3, 0.2], iterations=2)
    assert rec['sigma'] is None and rec['radius'] == 1 and np.array_equal(down16(out), dr.deconvolve(img, [0.5, 0.3, 0.2], 2)[0])
    got = dr.scene_measures(lambda im, taps, n: down16(deconvolve.deconvolve_disk(up16(im), taps=taps, iterations=n)[0]))
    print('clean %.6f, flux %.3e, noisy %.6f' % (got['clean'], got['flux'], got['noisy']))
    for key in ('clean', 'flux', 'noisy'):
        assert got[key] <= dr.TOLERANCE[key], key
    for bad in (dict(sigma=0.1), dict(sigma=5.0), dict(iterations=0), dict(radius=17), dict(sigma=1.0, taps=[1.0])):
        with pytest.raises(ValueError):
            deconvolve.deconvolve_disk(dev, **bad)


# ---- end to end: a scan, and a PNG ----
@pytest.fixture(scope='module')
def scan(mods, tmp_path_factory):
    deconvolve = mods[0]
    path = write_scan(tmp_path_factory, 'deconvolve', fr.pipeline_scan())
    return {'path': path, 'res': deconvolve.deconvolve_scan(path)}


def test_deconvolve_scan_is_the_restatement_of_its_disk(mods, scan):
    from solex_ser_recon_en_amd import SHG_MAIN, disk
    deconvolve = mods[0]
    res = scan['res']
    own = disk.scan_disk(scan['path'])
    image = down16(own['image'])
    assert np.array_equal(down16(res['image']), image) and res['circle'] == own['circle'] and res['shift'] == 0
    rec = res['record']
    assert rec['sigma'] == 1.2 and rec['radius'] == 5 and rec['iterations'] == 10 and rec['taps'] == [float(v) for v in deconvolve.gaussian_taps(1.2)]
    assert np.array_equal(down16(res['deconv']), dr.deconvolve(image, deconvolve.gaussian_taps(1.2), 10)[0])
    assert (down16(res['deconv']) != image).any()
    with pytest.raises(ValueError, match='circle'):
        deconvolve.deconvolve_scan(scan['path'], dict(SHG_MAIN.default_options(), ratio_fixe=1.0))


def test_command_line(mods, scan, tmp_path, capsys):
    from solex_ser_recon_en_amd import SHG_MAIN, sharpen
    from solex_ser_recon_en_amd.fits_io import read_fits_u16
    from solex_ser_recon_en_amd.png_io import read_png_gray
    deconvolve = mods[0]
    work = str(tmp_path / 'scan.ser')
    shutil.copy(scan['path'], work)
    res = scan['res']
    k = SHG_MAIN.default_options()['img_rotate'] // 90
    want = np.rot90(down16(res['deconv']), k)
    out = run_json(deconvolve.main, capsys, [work, '--contrast', '-f'])
    base = work[:-4] + '_shift=0_deconv'
    assert out['png'] == base + '.png' and out['fits'] == base + '.fits' and out['contrast'] == base and out['input'] == work
    assert np.array_equal(read_png_gray(out['png']), want) and np.array_equal(read_fits_u16(out['fits'])[0], want)
    for suffix in ('_clahe.png', '_protus.png', '_uncontrasted.png', '_high_contrast.png', '_clahe.fits'):
        assert os.path.exists(base + suffix), suffix
    assert np.array_equal(read_png_gray(base + '_uncontrasted.png'), want)
    rec = res['record']
    for key in ('input', 'shape', 'psf_sigma', 'radius', 'taps', 'iterations', 'flux', 'shift', 'circle', 'ratio', 'png', 'fits', 'contrast'):
        assert key in out, key
    assert out['shape'] == list(want.shape) and out['psf_sigma'] == 1.2 and out['radius'] == 5 and out['taps'] == rec['taps']
    assert out['iterations'] == 10 and out['shift'] == 0 and out['circle'] == list(res['circle']) and out['ratio'] == res['ratio']
    flux = float(want.astype(np.float64).sum()) / float(down16(res['image']).astype(np.float64).sum())
    assert out['flux'] == flux and abs(flux - 1.0) < 1e-3
    # a PNG the package wrote, another blur
    png = str(tmp_path / 'disk_stack.png')
    shutil.copy(base + '_uncontrasted.png', png)
    out = run_json(deconvolve.main, capsys, [png, '--psf-sigma', '1.5', '--iterations', '3', '--radius', '4'])
    assert out['png'] == png[:-4] + '_deconv.png' and out['fits'] is None and out['contrast'] is None and out['shift'] is None
    assert out['psf_sigma'] == 1.5 and out['radius'] == 4 and out['iterations'] == 3 and out['circle'] == [-1, -1, -1] and out['ratio'] is None
    again = dr.deconvolve(want, deconvolve.gaussian_taps(1.5, 4), 3)[0]
    assert np.array_equal(read_png_gray(out['png']), again) and out['shape'] == list(want.shape)
    assert out['flux'] == float(again.astype(np.float64).sum()) / float(want.astype(np.float64).sum())
    # stack -> deconvolve -> sharpen chains through files
    sharp = run_json(sharpen.main, capsys, [out['png'], '--sigma', '100'])
    assert sharp['png'] == png[:-4] + '_deconv_sharp.png' and os.path.exists(sharp['png']) and sharp['shape'] == list(want.shape)
    assert deconvolve.main([work, '-x']) == 1                                      # no limb fit, no circle
    assert 'circle' in capsys.readouterr().err
    eight = str(tmp_path / 'eight.png')
    from solex_ser_recon_en_amd.png_io import write_png
    write_png(eight, (want >> 8).astype(np.uint8), 0)
    assert deconvolve.main([eight]) == 1
    assert '16-bit' in capsys.readouterr().err
