"""k_lin_row_sums and k_lin_apply (csrc/linfilter.hip) past one 512-column segment, each against the NumPy statement of its
contract (tests/linfilter_ref.py) on the seeded cases that tests/test_linfilter_cpu.py holds to the kernels' preconditions:
stage 1 the two sum planes (bit for bit for a uint16 image), stage 2 the apply kernel alone on the reference's planes, stage 3
ops.lin_filter_u16 end to end, stage 4 the product route on a frame wider than two segments."""
import numpy as np
import pytest

from tests import linfilter_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

IDS = ['%s-%s' % (n, p) for n, p in ref.case_ids()]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def orc():
    from oracle import shg_oracle
    return shg_oracle


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # np.array: the cases are read-only, torch wants a writable array


def host(t):
    return t.cpu().numpy()


def _case(name):
    return next(c for c in ref.cases() if c['name'] == name)


def _device_image(c):
    """-> (the uint16 image as the case wants it handed over, the whole tensor it is a view of or None)."""
    if c['view'] is None:
        return dev(c['img']), None
    off, width, sentinel = c['view']
    wide = np.full((c['h'], width), sentinel, dtype=np.uint16)
    wide[:, off:off + c['w']] = c['img']
    base = dev(wide)
    return base[:, off:off + c['w']], base


def _check_view_untouched(c, base):
    if base is not None:
        off, width, sentinel = c['view']
        b = host(base)
        assert (b[:, :off] == sentinel).all() and (b[:, off + c['w']:] == sentinel).all()
        np.testing.assert_array_equal(b[:, off:off + c['w']], c['img'])


def _row_sums(ops, c, path):
    """shg_lin_filter_row_sums as ops.lin_filter_u16 calls it -> (hl, hf) on the host."""
    from solex_ser_recon_en_amd import _lib
    img, base = _device_image(c)
    ptr, h, w, pitch = ops._img(img, 'img', torch.uint16)
    assert pitch >= w and (c['view'] is None or (pitch > w and ptr % 16))
    rf = dev(c['row_factor']) if path == 'f64' else None
    flagged, up, dn = dev(c['flagged'].astype(np.uint8)), dev(c['up'].astype(np.int32)), dev(c['dn'].astype(np.int32))
    hl = torch.full((h, w), 12345.0, dtype=torch.float64, device='cuda')
    hf = torch.full((h, w), 12345.0, dtype=torch.float64, device='cuda')
    _lib.check(_lib.lib.shg_lin_filter_row_sums(ptr, h, w, pitch, rf.data_ptr() if rf is not None else None,
                                                ops._log_lut(img.device).data_ptr(), flagged.data_ptr(), up.data_ptr(), dn.data_ptr(),
                                                int(c['linlen']), hl.data_ptr(), hf.data_ptr(), ops._stream()), 'shg_lin_filter_row_sums')
    torch.cuda.synchronize()
    _check_view_untouched(c, base)
    return host(hl), host(hf)


def _apply(ops, c, path, hl, hf):
    """shg_lin_filter_apply on given host planes -> uint16 image on the host, written through a pitched destination."""
    from solex_ser_recon_en_amd import _lib
    img, base = _device_image(c)
    ptr, h, w, pitch = ops._img(img, 'img', torch.uint16)
    rf = dev(c['row_factor']) if path == 'f64' else None
    hl_d, hf_d = dev(hl), dev(hf)
    taper, xa, xb, edge = dev(c['taper']), dev(c['xa'].astype(np.int32)), dev(c['xb'].astype(np.int32)), dev(c['edge'].astype(np.uint8))
    out = ops.pitched_u16(h, w, img.device)
    _lib.check(_lib.lib.shg_lin_filter_apply(ptr, h, w, pitch, rf.data_ptr() if rf is not None else None, hl_d.data_ptr(),
                                             hf_d.data_ptr(), int(c['linlen']), int(c['half_width']), taper.data_ptr(), xa.data_ptr(),
                                             xb.data_ptr(), edge.data_ptr(), int(c['edge_half']), out.data_ptr(), out.stride(0),
                                             ops._stream()), 'shg_lin_filter_apply')
    torch.cuda.synchronize()
    _check_view_untouched(c, base)
    return host(out.contiguous())


@pytest.mark.parametrize('name,path', ref.case_ids(), ids=IDS)
def test_stage1_row_sums(ops, name, path):
    """uint16 image: the same float32 table and the same order of float64 additions, so hl and hf are the reference's bit for
    bit, -inf and NaN included.  float64 image: the device's float64 log against NumPy's, each within an ulp or so of the true
    value, through linlen additions: atol = linlen * 4 * spacing(max |log|), rtol = 0."""
    c = _case(name)
    hl, hf = _row_sums(ops, c, path)
    want_hl, want_hf = ref.reference(c, path)[:2]
    if path == 'u16':
        np.testing.assert_array_equal(hl, want_hl, err_msg='%s hl' % name)
        np.testing.assert_array_equal(hf, want_hf, err_msg='%s hf' % name)
        return
    src, _ = ref.source(c, path)
    atol = c['linlen'] * 4 * np.spacing(np.abs(np.log(src)).max())
    d_hl, d_hf = np.abs(hl - want_hl).max(), np.abs(hf - want_hf).max()
    print('LINFILTER stage 1 %-12s f64  max |hl - ref| %.3e  max |hf - ref| %.3e  atol %.3e' % (name, d_hl, d_hf, atol))
    assert np.isfinite(hl).all() and np.isfinite(hf).all()
    assert d_hl <= atol and d_hf <= atol, '%s: max |hl - ref| %.3e, max |hf - ref| %.3e, atol %.3e' % (name, d_hl, d_hf, atol)
    unflagged = ~c['flagged']
    np.testing.assert_array_equal(hf[unflagged], hl[unflagged])                     # one sum, stored twice


@pytest.mark.parametrize('name,path', ref.case_ids(), ids=IDS)
def test_stage2_apply_on_the_reference_planes(ops, name, path):
    """The apply kernel alone, fed the reference's hl and hf: exactly the source where the exponent is exactly 0, exactly the
    header's rule on the reference wherever the reference is further than 1e-6 from a truncation step, at most 1 LSB elsewhere."""
    c = _case(name)
    hl, hf, pre, expo = ref.reference(c, path)
    got = _apply(ops, c, path, hl, hf)
    src, _ = ref.source(c, path)
    n = ref.check_output(got, pre, expo, np.asarray(src, dtype=np.float64), name)
    print('LINFILTER stage 2 %-12s %s  in band %d' % (name, path, n))
    if name == 'saturation':
        over = pre > 65535
        assert over.mean() >= 0.05 and (got[over] == 65535).all()


@pytest.mark.parametrize('name,path', ref.case_ids(), ids=IDS)
def test_stage3_ops_end_to_end(ops, name, path):
    """ops.lin_filter_u16 (both kernels, the device's own planes) under the stage-2 criterion; the source view's surroundings
    stay as they were."""
    c = _case(name)
    img, base = _device_image(c)
    rows = [np.array(c[k]) for k in ('flagged', 'up', 'dn', 'taper', 'xa', 'xb', 'edge')]            # writable copies for torch
    out = ops.lin_filter_u16(img, *rows, c['edge_half'], c['linlen'], c['half_width'], dev(c['row_factor']) if path == 'f64' else None)
    assert out.shape == (c['h'], c['w']) and out.dtype == torch.uint16
    hl, hf, pre, expo = ref.reference(c, path)
    src, _ = ref.source(c, path)
    n = ref.check_output(host(out.contiguous()), pre, expo, np.asarray(src, dtype=np.float64), name)
    print('LINFILTER stage 3 %-12s %s  in band %d' % (name, path, n))
    _check_view_untouched(c, base)


@pytest.mark.parametrize('path', ['u16', 'f64'])
def test_stage4_product_route_on_a_wide_frame(ops, orc, path):
    """su.correct_transversalium2 (stubborn branch) on a 160 x 1100 disk frame against the oracle, under the criterion of
    test_lin_filter_vs_oracle_and_reference_shim: the host's float32 log table and the Savitzky-Golay trend enter as well, so at
    most 1 LSB on at most 8 pixels."""
    from solex_ser_recon_en_amd import solex_util as su
    from solex_ser_recon_en_amd.device import DeviceImage
    img, rf, circle, borders = ref.disk_frame()
    opts = {'stubborn_transversalium': True, 'trans_strength': 301, '_nolog': True, 'clahe_only': True, 'protus_only': False}
    frame = DeviceImage(dev(img), row_factor=dev(rf)) if path == 'f64' else dev(img)
    got = np.asarray(su.correct_transversalium2(frame, circle, borders, opts, 0, 'x'))
    with np.errstate(all='ignore'):
        want, flag = orc.correct_transversalium2_stubborn(img * rf[:, None] if path == 'f64' else img, circle, borders, 301)
    assert flag.sum() >= 3 and got.dtype == np.uint16 and got.shape == want.shape == (160, 1100)
    assert np.count_nonzero(want != np.minimum(img * (rf[:, None] if path == 'f64' else 1), 65535).astype(np.uint16)) > 5000
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print('LINFILTER stage 4 %s  %d pixels differ, max %d LSB' % (path, np.count_nonzero(d), d.max()))
    assert d.max() <= 1 and np.count_nonzero(d) <= 8, (int(d.max()), int(np.count_nonzero(d)))
