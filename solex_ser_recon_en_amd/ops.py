"""Thin tensor-level wrappers over the C ABI (include/shg_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
computation below happens in libshg_hip.so.  All tensors must live on the GPU; a
CPU tensor raises (there is no CPU path).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib


def _stream():
    # raw hipStream_t of torch's current stream (the public accessor builds a Stream object: ~1 us per call)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _dev(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s must be a GPU tensor: the SHG hot path has no CPU fallback' % what)
    return t


def _img(t, what, dtype=None):
    """(ptr, h, w, pitch) of a 2-D image view with unit column stride."""
    _dev(t, what)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError('%s must be a 2-D image with contiguous rows' % what)
    if dtype is not None and t.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (what, dtype, t.dtype))
    return t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)


def _out_like(out, h, w, dtype, device, what='out'):
    """(the tensor, ptr, pitch) of an [h, w] output view of `dtype`: the caller's `out`, or a new one when it is None."""
    if out is None:
        out = torch.empty((h, w), dtype=dtype, device=device)
    ptr, oh, ow, pitch = _img(out, what, dtype)
    if (oh, ow) != (h, w):
        raise ValueError('%s must be a %s [%d, %d] view' % (what, str(dtype).split('.')[-1], h, w))
    return out, ptr, pitch


def _int64_out(out, shape, device):
    """A contiguous int64 output of `shape`: the caller's `out`, or a new one when it is None."""
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=device)
    if _dev(out, 'out').dtype != torch.int64 or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError('out must be a contiguous int64 [%s] tensor' % ', '.join('%d' % v for v in shape))
    return out


def _points(points, device):
    """(the points as a contiguous int32 [n, 2] tensor on `device` -- a host array is uploaded --, n)."""
    if not isinstance(points, torch.Tensor):
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)).to(device)
    if _dev(points, 'points').dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 2 or not points.is_contiguous():
        raise ValueError('points must be a contiguous int32 [n, 2] tensor of (row, col)')
    if points.shape[0] < 1:
        raise ValueError('at least one point is needed')
    return points, int(points.shape[0])


def _workspace(workspace, need, device):
    """(the tensor, its bytes): the caller's workspace, or a new uint8 one of `need` bytes when it is None."""
    ws = torch.empty(need, dtype=torch.uint8, device=device) if workspace is None else _dev(workspace, 'workspace')
    return ws, ws.numel() * ws.element_size()


def pitched_u16(h, w, device, align=64):
    """uint16 image whose row pitch is a multiple of `align` elements (128 B rows)."""
    pitch = (w + align - 1) // align * align
    return torch.empty((h, pitch), dtype=torch.uint16, device=device)[:, :w]


def padded_stack(n, h, w, dtype, device):
    """An [n, h, w] frame stack whose frame pitch is shg_frame_pitch_bytes (frame size rounded up to 8 KiB):
    the layout video_reader.device_stack() uploads into and the frame-walking kernels read fastest."""
    item = torch.empty((), dtype=dtype).element_size()
    pitch = lib.shg_frame_pitch_bytes(h * w * item) // item
    store = torch.empty(n * pitch, dtype=dtype, device=device)
    return torch.as_strided(store, (n, h, w), (pitch, w, 1))


def stack_to_host(stack):
    """Dense NumPy copy [n, H, W] of a (possibly pitched) frame stack."""
    if stack.dtype == torch.uint16:
        return stack.view(torch.int16).contiguous().cpu().numpy().view(np.uint16)
    return stack.contiguous().cpu().numpy()


def frame_stride(stack):
    return stack.stride(0) if stack.shape[0] > 1 else stack.shape[1] * stack.shape[2]


def stack_geometry(stack):
    """(n, H, W, bytes_per_px) of a frame stack in file layout (frames dense, frame pitch >= H*W)."""
    _dev(stack, 'stack')
    if stack.dim() != 3 or stack.stride(2) != 1 or stack.stride(1) != stack.shape[2] or (
            stack.shape[0] > 1 and stack.stride(0) < stack.shape[1] * stack.shape[2]):
        raise ValueError('stack must be an [N, Height, Width] tensor with dense frames')
    if stack.dtype == torch.uint8:
        bpp = 1
    elif stack.dtype in (torch.uint16, torch.int16):
        bpp = 2
    else:
        raise TypeError('stack must be uint8 or uint16, got %s' % stack.dtype)
    n, h, w = stack.shape
    return n, h, w, bpp


# ---- pass A ---------------------------------------------------------------
def accumulate_sum_max(stack, workspace=None):
    """-> (sum int64 [H*W], max uint16 [H*W]) in file layout, raw sample units."""
    n, h, w, bpp = stack_geometry(stack)
    dev = stack.device
    need = lib.shg_accumulate_workspace_bytes(n, h, w, bpp)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    total = torch.empty(h * w, dtype=torch.int64, device=dev)
    mx = torch.empty(h * w, dtype=torch.uint16, device=dev)
    _lib.check(lib.shg_accumulate_sum_max(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), total.data_ptr(), mx.data_ptr(),
                                          workspace.data_ptr(), workspace.numel(), _stream()),
               'shg_accumulate_sum_max')
    return total, mx


def accumulate_mean_max(stack, workspace=None):
    """compute_mean_max for a stack that is whole on this GPU -> (mean uint16 [ih, iw], max uint16 [ih, iw]):
    pass A and the division / rotation straight from its per-slab partials."""
    n, h, w, bpp = stack_geometry(stack)
    dev = stack.device
    need = lib.shg_accumulate_workspace_bytes(n, h, w, bpp)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    ih, iw = (w, h) if w > h else (h, w)
    mean = torch.empty((ih, iw), dtype=torch.uint16, device=dev)
    mout = torch.empty((ih, iw), dtype=torch.uint16, device=dev)
    _lib.check(lib.shg_accumulate_mean_max(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), mean.data_ptr(), mout.data_ptr(),
                                           workspace.data_ptr(), workspace.numel(), _stream()), 'shg_accumulate_mean_max')
    return mean, mout


def pass_a_prelaunch(stack, workspace):
    """Start pass A of `stack` on the device's frame-pass lane now, behind what the current stream holds (shg_pass_a_prelaunch);
    accumulate_mean_max(stack, workspace) later finds it there.  -> False when the device has no lane (nothing was launched)."""
    n, h, w, bpp = stack_geometry(stack)
    need = lib.shg_accumulate_workspace_bytes(n, h, w, bpp)
    if workspace.numel() < need:
        raise ValueError('pass_a_prelaunch: workspace of %d bytes, %d needed' % (workspace.numel(), need))
    launched = ctypes.c_int()
    _lib.check(lib.shg_pass_a_prelaunch(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), workspace.data_ptr(), workspace.numel(),
                                        _stream(), ctypes.byref(launched)), 'shg_pass_a_prelaunch')
    return bool(launched.value)


def finalize_mean_max(total, mx, n_total, height, width, bpp):
    """-> (mean uint16 [ih, iw], max uint16 [ih, iw]) in the reference's orientation."""
    _dev(total, 'sum')
    ih, iw = (width, height) if width > height else (height, width)
    mean = torch.empty((ih, iw), dtype=torch.uint16, device=total.device)
    mout = torch.empty((ih, iw), dtype=torch.uint16, device=total.device)
    _lib.check(lib.shg_finalize_mean_max(total.data_ptr(), mx.data_ptr(), int(n_total), height, width, bpp,
                                         mean.data_ptr(), mout.data_ptr(), _stream()), 'shg_finalize_mean_max')
    return mean, mout


def reduce_frame_stats(pieces, npix):
    """pieces: int32 GPU tensor [G, words], every row one rank's [npix sums as 32-bit words | npix maxima as 16-bit words | ...]
    (dist.exchange_frame_stats' all-gather) -> (int64 [npix] sums, uint16 [npix] maxima) over all ranks, one launch."""
    _dev(pieces, 'pieces')
    if pieces.dtype != torch.int32 or pieces.dim() != 2 or not pieces.is_contiguous():
        raise TypeError('pieces must be a contiguous int32 [G, words] tensor')
    total = torch.empty(int(npix), dtype=torch.int64, device=pieces.device)
    mx = torch.empty(int(npix), dtype=torch.uint16, device=pieces.device)
    _lib.check(lib.shg_reduce_frame_stats(pieces.data_ptr(), int(pieces.shape[0]), int(pieces.shape[1]), int(npix), total.data_ptr(),
                                          mx.data_ptr(), _stream()), 'shg_reduce_frame_stats')
    return total, mx


# ---- line detection helpers -------------------------------------------------
def box_blur_u16(img, kw, kh):
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    if pitch != w:
        raise ValueError('box_blur_u16 needs a dense image')
    out = torch.empty_like(img)
    tmp = torch.empty(h * w, dtype=torch.int32, device=img.device)
    _lib.check(lib.shg_box_blur_u16(ptr, h, w, int(kw), int(kh), out.data_ptr(), tmp.data_ptr(), _stream()),
               'shg_box_blur_u16')
    return out


def row_argmin_u16(img, x0, x1):
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    if pitch != w:
        raise ValueError('row_argmin_u16 needs a dense image')
    out = torch.empty(h, dtype=torch.int32, device=img.device)
    _lib.check(lib.shg_row_argmin_u16(ptr, h, w, int(x0), int(x1), out.data_ptr(), _stream()), 'shg_row_argmin_u16')
    return out


def row_mean_u16(img):
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    if pitch != w:
        raise ValueError('row_mean_u16 needs a dense image')
    out = torch.empty(h, dtype=torch.float64, device=img.device)
    _lib.check(lib.shg_row_mean_u16(ptr, h, w, out.data_ptr(), _stream()), 'shg_row_mean_u16')
    return out


def blur_row_mean_u16(img, kw, kh):
    """np.mean(cv2.blur(img, (kw, kh)), axis=1) without materialising the blurred image -> float64 [h]."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    if pitch != w:
        raise ValueError('blur_row_mean_u16 needs a dense image')
    out = torch.empty(h, dtype=torch.float64, device=img.device)
    _lib.check(lib.shg_blur_row_mean_u16(ptr, h, w, int(kw), int(kh), out.data_ptr(), _stream()), 'shg_blur_row_mean_u16')
    return out


def blur_argmin_u16(img, kw, kh, x0, x1):
    """(np.argmin(cv2.blur(img, (kw, kh))[:, x0:x1], axis=1), np.argmin(img, axis=1)) -> two int32 [h] tensors."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    if pitch != w:
        raise ValueError('blur_argmin_u16 needs a dense image')
    out = torch.empty((2, h), dtype=torch.int32, device=img.device)
    _lib.check(lib.shg_blur_argmin_u16(ptr, h, w, int(kw), int(kh), int(x0), int(x1), out[0].data_ptr(), out[1].data_ptr(), _stream()),
               'shg_blur_argmin_u16')
    return out[0], out[1]


# ---- pass B ---------------------------------------------------------------
def extract_columns(stack, ind_l, lw, rw, n_cols=None, k_offset=0, flip_x=False, out=None):
    """-> disks uint16 [S, ih, n_cols] (a view of a row-pitched buffer).

    ind_l int32 [S, ih] (clamped), lw/rw float64 [ih]: host arrays or GPU tensors."""
    n, h, w, bpp = stack_geometry(stack)
    dev = stack.device
    ih = max(h, w)
    ind_l = torch.as_tensor(np.ascontiguousarray(ind_l, dtype=np.int32) if not isinstance(ind_l, torch.Tensor) else ind_l).to(dev)
    if not isinstance(lw, torch.Tensor) and not isinstance(rw, torch.Tensor) and np.shape(lw) == np.shape(rw):
        both = torch.from_numpy(np.stack([np.asarray(lw, dtype=np.float64), np.asarray(rw, dtype=np.float64)])).to(dev)   # one upload
        lw, rw = both[0], both[1]
    else:
        lw = torch.as_tensor(np.ascontiguousarray(lw, dtype=np.float64) if not isinstance(lw, torch.Tensor) else lw).to(dev)
        rw = torch.as_tensor(np.ascontiguousarray(rw, dtype=np.float64) if not isinstance(rw, torch.Tensor) else rw).to(dev)
    if ind_l.dim() != 2 or ind_l.shape[1] != ih or lw.shape != (ih,) or rw.shape != (ih,):
        raise ValueError('ind_l must be [S, %d] and lw, rw [%d]' % (ih, ih))
    if ind_l.dtype != torch.int32 or lw.dtype != torch.float64 or rw.dtype != torch.float64:
        raise TypeError('ind_l must be int32 and lw, rw float64')
    s = ind_l.shape[0]
    n_cols = n if n_cols is None else int(n_cols)
    if out is None:
        pitch = (n_cols + 63) // 64 * 64
        # every column is written when this call covers the whole scan; a shard's call leaves the others' columns zero
        alloc = torch.empty if (n_cols == n and int(k_offset) == 0) else torch.zeros
        out = alloc((s, ih, pitch), dtype=torch.uint16, device=dev)[:, :, :n_cols]
    if out.shape != (s, ih, n_cols) or out.stride(2) != 1:
        raise ValueError('out must be a [S, ih, n_cols] view with unit column stride')
    _lib.check(lib.shg_extract_columns(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), ind_l.contiguous().data_ptr(),
                                       lw.contiguous().data_ptr(), rw.contiguous().data_ptr(), s, out.data_ptr(),
                                       out.stride(1), out.stride(0), n_cols, int(k_offset), int(bool(flip_x)),
                                       _stream()), 'shg_extract_columns')
    return out


def extract_columns_dense(stack, fit, shifts, flip_x=False, want_minmax=False):
    """shg_extract_columns_dense for consecutive shifts (any order, 3..24 of them): every distinct sample of a (row, frame) loaded
    once.  fit: host [ih, 4] as compute_mean_return_fit returns it.  -> disks uint16 [S, ih, n] (and the extrema int32 [S, 2])."""
    from . import hostmath
    n, h, w, bpp = stack_geometry(stack)
    dev = stack.device
    ih, iw = (w, h) if w > h else (h, w)
    sh = np.ascontiguousarray(shifts, dtype=np.int32)
    s = int(sh.size)
    if not lib.shg_extract_dense_fits(sh.ctypes.data, s):
        raise ValueError('extract_columns_dense needs 3..24 consecutive shifts')
    fit = np.ascontiguousarray(fit, dtype=np.float64)
    ind_l, lw, rw = hostmath.column_plan(fit, sh, ih, iw)
    base = (fit[:, 0] + 1.0 * float(sh.min())).astype(np.int64).astype(np.int32)
    ind_d = torch.from_numpy(ind_l).to(dev)
    w_d = torch.from_numpy(np.stack([lw, rw])).to(dev)
    base_d = torch.from_numpy(base).to(dev)
    pitch = (n + 63) // 64 * 64
    out = torch.empty((s, ih, pitch), dtype=torch.uint16, device=dev)[:, :, :n]
    mm = torch.empty(s * 130, dtype=torch.int32, device=dev) if want_minmax else None
    _lib.check(lib.shg_extract_columns_dense(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), ind_d.data_ptr(), base_d.data_ptr(),
                                             w_d[0].data_ptr(), w_d[1].data_ptr(), sh.ctypes.data, s, out.data_ptr(), out.stride(1), out.stride(0),
                                             n, 0, int(bool(flip_x)), None if mm is None else mm.data_ptr(), _stream()), 'shg_extract_columns_dense')
    return (out, mm[s * 128:].view(s, 2)) if want_minmax else out


# ---- post-processing ----------------------------------------------------------
def warp_rows_u16(img, h00, h01, h02, out_h, out_w, minmax=None):
    """minmax: the plane's extrema as shg_extract_columns_minmax left them (int32 [2] = {min, max}); None = found here."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    out = pitched_u16(out_h, out_w, img.device)
    if minmax is not None:
        _lib.check(lib.shg_warp_rows_minmax_u16(ptr, h, w, pitch, float(h00), float(h01), float(h02), out.data_ptr(), int(out_h),
                                                int(out_w), out.stride(0), minmax.data_ptr(), _stream()), 'shg_warp_rows_minmax_u16')
        return out
    mm = torch.empty(2, dtype=torch.int32, device=img.device)
    _lib.check(lib.shg_warp_rows_u16(ptr, h, w, pitch, float(h00), float(h01), float(h02), out.data_ptr(),
                                     int(out_h), int(out_w), out.stride(0), mm.data_ptr(), _stream()),
               'shg_warp_rows_u16')
    return out


def _row_factor_ptr(row_factor, h, device):
    if row_factor is None:
        return None, None
    rf = row_factor if isinstance(row_factor, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(row_factor, dtype=np.float64))
    rf = rf.to(device).contiguous()
    if rf.shape != (h,) or rf.dtype != torch.float64:
        raise ValueError('row_factor must be float64 [h]')
    return rf, rf.data_ptr()


def rowpair_logratio_stats(img, y1, y2, xa, xb, row_factor=None):
    """xa, xb: int32 host arrays [y2-y1] of NumPy-normalised slice bounds. -> float64 tensor [y2-y1]."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    if not isinstance(xa, torch.Tensor):
        xa = torch.as_tensor(np.ascontiguousarray(xa, dtype=np.int32)).to(img.device)
    if not isinstance(xb, torch.Tensor):
        xb = torch.as_tensor(np.ascontiguousarray(xb, dtype=np.int32)).to(img.device)
    if xa.numel() != y2 - y1 or xb.numel() != y2 - y1 or xa.dtype != torch.int32 or xb.dtype != torch.int32:
        raise ValueError('xa, xb must be int32 with y2 - y1 entries')
    rf, rf_ptr = _row_factor_ptr(row_factor, h, img.device)
    out = torch.empty(y2 - y1, dtype=torch.float64, device=img.device)
    _lib.check(lib.shg_rowpair_logratio_stats(ptr, h, w, pitch, int(y1), int(y2), xa.data_ptr(), xb.data_ptr(), rf_ptr,
                                              out.data_ptr(), _stream()), 'shg_rowpair_logratio_stats')
    return out


def scale_rows_u16(img, c, row_factor=None):
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    c = torch.as_tensor(np.ascontiguousarray(c, dtype=np.float64)).to(img.device) if not isinstance(c, torch.Tensor) else c
    if c.shape != (h,) or c.dtype != torch.float64:
        raise ValueError('c must be float64 [h]')
    rf, rf_ptr = _row_factor_ptr(row_factor, h, img.device)
    out = pitched_u16(h, w, img.device)
    _lib.check(lib.shg_scale_rows_u16(ptr, h, w, pitch, c.contiguous().data_ptr(), rf_ptr, out.data_ptr(), out.stride(0),
                                      _stream()), 'shg_scale_rows_u16')
    return out


_TAPS = {}


def correlate1d_rows_f64(rows, weights):
    """scipy.ndimage.correlate1d(rows, weights, axis=-1, mode='constant') for a float64 GPU tensor [k, n]; `weights`
    is a host array of odd length (as correlate1d takes them).  SciPy's symmetric-filter test is made here."""
    _dev(rows, 'rows')
    if rows.dim() != 2 or rows.dtype != torch.float64 or not rows.is_contiguous():
        raise ValueError('rows must be a contiguous float64 [k, n] tensor')
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or not w.size & 1:
        raise ValueError('weights must be 1-D of odd length')
    key = (str(rows.device), w.tobytes())
    if key not in _TAPS:
        r = w.size // 2
        eps = np.finfo(np.float64).eps                                                          # NI_Correlate1D's tests
        sym = 1 if all(abs(w[r + i] - w[r - i]) <= eps for i in range(1, r + 1)) else (
            -1 if all(abs(w[r + i] + w[r - i]) <= eps for i in range(1, r + 1)) else 0)
        if len(_TAPS) > 64:
            _TAPS.clear()
        _TAPS[key] = (torch.from_numpy(w).to(rows.device), r, int(sym))
    wd, r, sym = _TAPS[key]
    out = torch.empty_like(rows)
    _lib.check(lib.shg_correlate1d_rows_f64(rows.data_ptr(), rows.shape[0], rows.shape[1], wd.data_ptr(), r, sym, out.data_ptr(),
                                            _stream()), 'shg_correlate1d_rows_f64')
    return out


_LOG_LUT = {}


def _log_lut(device):
    """float32 log of every uint16 value exactly as NumPy computes np.log(uint16 image) on this host."""
    key = str(device)
    if key not in _LOG_LUT:
        with np.errstate(divide='ignore'):
            lut = np.log(np.arange(65536, dtype=np.uint16))
        assert lut.dtype == np.float32
        _LOG_LUT[key] = torch.from_numpy(lut).to(device)
    return _LOG_LUT[key]


def lin_filter_u16(img, flagged, up, dn, taper, xa, xb, edge, edge_half, linlen=101, half_width=5, row_factor=None):
    """apply_lin_filter + fix_edge_effect (solex_util.py:277-375) -> uint16 image (saturated, truncated).
    flagged / up / dn / taper / xa / xb / edge: per-row host arrays (see include/shg_hip.h)."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    dev = img.device

    def put(a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (h,):
            raise ValueError('per-row arrays must have shape (%d,)' % h)
        return torch.from_numpy(a).to(dev)
    flagged_d, up_d, dn_d = put(flagged, np.uint8), put(up, np.int32), put(dn, np.int32)
    taper_d, xa_d, xb_d, edge_d = put(taper, np.float64), put(xa, np.int32), put(xb, np.int32), put(edge, np.uint8)
    rf, rf_ptr = _row_factor_ptr(row_factor, h, dev)
    lut = _log_lut(dev)
    hl = torch.empty((h, w), dtype=torch.float64, device=dev)
    hf = torch.empty((h, w), dtype=torch.float64, device=dev)
    _lib.check(lib.shg_lin_filter_row_sums(ptr, h, w, pitch, rf_ptr, lut.data_ptr(), flagged_d.data_ptr(), up_d.data_ptr(),
                                           dn_d.data_ptr(), int(linlen), hl.data_ptr(), hf.data_ptr(), _stream()),
               'shg_lin_filter_row_sums')
    out = pitched_u16(h, w, dev)
    _lib.check(lib.shg_lin_filter_apply(ptr, h, w, pitch, rf_ptr, hl.data_ptr(), hf.data_ptr(), int(linlen), int(half_width),
                                        taper_d.data_ptr(), xa_d.data_ptr(), xb_d.data_ptr(), edge_d.data_ptr(), int(edge_half),
                                        out.data_ptr(), out.stride(0), _stream()), 'shg_lin_filter_apply')
    return out


def line_order_stats_u16(img, axis, rank_lo, rank_hi):
    """-> (lo, hi) uint16 GPU tensors: per column (axis 0) / row (axis 1) order statistics."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    lines = w if axis == 0 else h
    out = torch.empty((2, lines), dtype=torch.uint16, device=img.device)
    _lib.check(lib.shg_line_order_stats_u16(ptr, h, w, pitch, int(axis), int(rank_lo), int(rank_hi), out[0].data_ptr(),
                                            out[1].data_ptr(), _stream()), 'shg_line_order_stats_u16')
    return out[0], out[1]


def crop_pad_u16(img, nw, sx0, dx0, n, fill):
    """fill: 0..65535, or None for img[0, 0] (read on the device)."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    out = pitched_u16(h, nw, img.device)
    _lib.check(lib.shg_crop_pad_u16(ptr, h, w, pitch, out.data_ptr(), int(nw), out.stride(0), int(sx0), int(dx0),
                                    int(n), -1 if fill is None else int(fill), _stream()), 'shg_crop_pad_u16')
    return out


def clahe(img, clip_limit=0.8, tiles=2, small_workspace=False):
    """small_workspace: give shg_clahe only shg_clahe_workspace_bytes (it then builds the 16-bit tile histograms with
    global atomics); the default is the roomier shg_clahe_workspace_bytes_for."""
    _dev(img, 'img')
    if img.dtype == torch.uint16:
        bpp = 2
    elif img.dtype == torch.uint8:
        bpp = 1
    else:
        raise TypeError('clahe needs uint8 or uint16')
    ptr, h, w, pitch = _img(img, 'img')
    need = lib.shg_clahe_workspace_bytes(int(tiles), bpp) if small_workspace else lib.shg_clahe_workspace_bytes_for(h, w, int(tiles), bpp)
    if need == 0:
        raise ValueError('clahe: unsupported tile count %r' % (tiles,))
    ws = torch.empty(need, dtype=torch.uint8, device=img.device)
    out = pitched_u16(h, w, img.device) if bpp == 2 else torch.empty((h, w), dtype=torch.uint8, device=img.device)
    _lib.check(lib.shg_clahe(ptr, h, w, pitch, bpp, float(clip_limit), int(tiles), out.data_ptr(), out.stride(0),
                             ws.data_ptr(), need, _stream()), 'shg_clahe')
    return out


def contrast_stats_u16(frame, ranks_frame, ranks_cl1, out5, clip_limit=0.8, tiles=2, small_workspace=False):
    """cl1 = clahe(frame) plus the order statistics of frame (2 ranks) and cl1 (3 ranks) into out5 (float64 [5], GPU):
    one C call for the first half of image_process.  -> cl1"""
    import ctypes
    ptr, h, w, pitch = _img(frame, 'frame', torch.uint16)
    need = (lib.shg_contrast_stats_workspace_bytes(int(tiles)) if small_workspace
            else lib.shg_contrast_stats_workspace_bytes_for(h, w, int(tiles)))
    if need == 0:
        raise ValueError('contrast_stats: unsupported tile count %r' % (tiles,))
    ws = torch.empty(need, dtype=torch.uint8, device=frame.device)
    cl1 = pitched_u16(h, w, frame.device)
    rf = (ctypes.c_int64 * 2)(*[int(r) for r in ranks_frame])
    rc = (ctypes.c_int64 * 3)(*[int(r) for r in ranks_cl1])
    _lib.check(lib.shg_contrast_stats_u16(ptr, h, w, pitch, float(clip_limit), int(tiles), cl1.data_ptr(), cl1.stride(0), rf, rc,
                                          out5.data_ptr(), ws.data_ptr(), need, _stream()), 'shg_contrast_stats_u16')
    return cl1


def contrast_products_u16(frame, cl1, lo_hi6, disc=None):
    """-> (high_contrast, protus, cc): the three rescale_brightness calls of image_process and the protuberance disc
    (disc = (x0, y0, r) or None) in one C call."""
    import ctypes
    ptr, h, w, pitch = _img(frame, 'frame', torch.uint16)
    cptr, ch, cw, cpitch = _img(cl1, 'cl1', torch.uint16)
    if (ch, cw) != (h, w):
        raise ValueError('frame and cl1 must share one shape')
    store = torch.empty((3, h, (w + 63) // 64 * 64), dtype=torch.uint16, device=frame.device)
    hc, protus, cc = store[0, :, :w], store[1, :, :w], store[2, :, :w]
    bounds = (ctypes.c_double * 6)(*[float(v) for v in lo_hi6])
    x0, y0, r = (int(v) for v in disc) if disc is not None else (0, 0, 0)
    _lib.check(lib.shg_contrast_products_u16(ptr, pitch, cptr, cpitch, h, w, bounds, hc.data_ptr(), protus.data_ptr(), cc.data_ptr(),
                                             store.stride(1), x0, y0, r, _stream()), 'shg_contrast_products_u16')
    return hc, protus, cc


def histogram(img):
    """-> int32 tensor [65536] (uint16 images) or [256] (uint8)."""
    _dev(img, 'img')
    bpp = 2 if img.dtype == torch.uint16 else 1
    if img.dtype not in (torch.uint16, torch.uint8):
        raise TypeError('histogram needs uint8 or uint16')
    ptr, h, w, pitch = _img(img, 'img')
    hist = torch.empty(65536 if bpp == 2 else 256, dtype=torch.int32, device=img.device)
    _lib.check(lib.shg_hist(ptr, h, w, pitch, bpp, hist.data_ptr(), _stream()), 'shg_hist')
    return hist


def rescale_u8(img, lo, hi, alpha=1.0):
    ptr, h, w, pitch = _img(img, 'img', torch.uint8)
    out = torch.empty((h, w), dtype=torch.uint8, device=img.device)
    _lib.check(lib.shg_rescale_u8(ptr, h, w, pitch, float(lo), float(hi), float(alpha), out.data_ptr(), out.stride(0), _stream()),
               'shg_rescale_u8')
    return out


def rescale_u16(img, lo, hi, alpha=1.0):
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    out = pitched_u16(h, w, img.device)
    _lib.check(lib.shg_rescale_u16(ptr, h, w, pitch, float(lo), float(hi), float(alpha), out.data_ptr(),
                                   out.stride(0), _stream()), 'shg_rescale_u16')
    return out


def fill_disc_u16(img, x0, y0, r, value):
    """In place (cv2.circle returns its argument too)."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    _lib.check(lib.shg_fill_disc_u16(ptr, h, w, pitch, int(x0), int(y0), int(r), int(value), None, _stream()),
               'shg_fill_disc_u16')
    return img


def downscale_mean_u16(img, factor=4):
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    oh, ow = -(-h // factor), -(-w // factor)
    out = torch.empty((oh, ow), dtype=torch.float64, device=img.device)
    _lib.check(lib.shg_downscale_mean_u16(ptr, h, w, pitch, int(factor), out.data_ptr(), _stream()),
               'shg_downscale_mean_u16')
    return out


# ---- limb detection on the block-mean image -----------------------------------------
def box_blur_f64(img, k):
    _dev(img, 'img')
    if img.dtype != torch.float64 or img.dim() != 2 or not img.is_contiguous():
        raise TypeError('box_blur_f64 needs a dense float64 image')
    h, w = img.shape
    out = torch.empty_like(img)
    tmp = torch.empty_like(img)
    _lib.check(lib.shg_box_blur_f64(img.data_ptr(), h, w, int(k), out.data_ptr(), tmp.data_ptr(), _stream()),
               'shg_box_blur_f64')
    return out


def box_blur_key_f64(img, k):
    """cv2.blur of a block-mean image (whole numbers of 2^-20 below 1) -> (blurred float64, window sums uint32 in 2^-20 units)."""
    _dev(img, 'img')
    if img.dtype != torch.float64 or img.dim() != 2 or not img.is_contiguous():
        raise TypeError('box_blur_key_f64 needs a dense float64 image')
    h, w = img.shape
    out = torch.empty_like(img)
    tmp = torch.empty_like(img)
    keys = torch.empty((h, w), dtype=torch.int32, device=img.device)
    _lib.check(lib.shg_box_blur_key_f64(img.data_ptr(), h, w, int(k), out.data_ptr(), keys.data_ptr(), tmp.data_ptr(), _stream()),
               'shg_box_blur_key_f64')
    return out, keys


def select_keys_u32(keys, ranks, ks):
    """out[i] = the ranks[i]-th smallest window sum of keys[i], as the blurred value (key * 2^-20) / (ks[i] ** 2)."""
    import ctypes
    n = keys[0].numel()
    ptrs = (ctypes.c_void_p * len(keys))(*[k.data_ptr() for k in keys])
    rk = (ctypes.c_int64 * len(ranks))(*[int(r) for r in ranks])
    kk = (ctypes.c_int * len(ks))(*[int(v) for v in ks])
    need = lib.shg_select_keys_workspace_bytes(len(keys))
    ws = torch.empty(need, dtype=torch.uint8, device=keys[0].device)
    out = torch.empty(len(keys), dtype=torch.float64, device=keys[0].device)
    _lib.check(lib.shg_select_keys_u32(ptrs, n, rk, kk, len(keys), out.data_ptr(), ws.data_ptr(), need, _stream()), 'shg_select_keys_u32')
    return out


def gaussian_taps(sigma, truncate=4.0):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius): the taps gaussian_filter correlates with."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum(), radius


def canny_masks(blurred, flood_thresh, sigma, low, high):
    """-> (low_mask, high_mask) uint8 GPU tensors [h, w]."""
    _dev(blurred, 'blurred')
    if blurred.dtype != torch.float64 or blurred.dim() != 2 or not blurred.is_contiguous():
        raise TypeError('canny_masks needs a dense float64 image')
    h, w = blurred.shape
    taps, radius = gaussian_taps(sigma)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    need = lib.shg_canny_workspace_bytes(h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=blurred.device)
    masks = torch.empty((2, h, w), dtype=torch.uint8, device=blurred.device)
    import ctypes
    _lib.check(lib.shg_canny_masks_f64(blurred.data_ptr(), h, w, float(flood_thresh),
                                       taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), radius, float(low), float(high),
                                       masks[0].data_ptr(), masks[1].data_ptr(), ws.data_ptr(), need, _stream()),
               'shg_canny_masks_f64')
    return masks[0], masks[1]


def select_f64(values, ranks):
    """-> float64 GPU tensor: the ranks[i]-th smallest elements (0-based) of a dense float64 tensor."""
    import ctypes
    _dev(values, 'values')
    if values.dtype != torch.float64 or not values.is_contiguous():
        raise TypeError('select_f64 needs a dense float64 tensor')
    ranks = [int(r) for r in ranks]
    arr = (ctypes.c_int64 * len(ranks))(*ranks)
    need = lib.shg_select_workspace_bytes(len(ranks))
    if need == 0:
        raise ValueError('select_f64 takes 1..8 ranks')
    ws = torch.empty(need, dtype=torch.uint8, device=values.device)
    out = torch.empty(len(ranks), dtype=torch.float64, device=values.device)
    _lib.check(lib.shg_select_f64(values.data_ptr(), values.numel(), arr, len(ranks), out.data_ptr(), ws.data_ptr(), need,
                                  _stream()), 'shg_select_f64')
    return out


def select_multi_f64(arrays, ranks):
    """out[i] = the ranks[i]-th smallest element of arrays[i] (dense float64 GPU tensors of one size), one launch sequence."""
    import ctypes
    if len(arrays) != len(ranks) or not 1 <= len(ranks) <= 8:
        raise ValueError('select_multi_f64 takes 1..8 (array, rank) pairs')
    n = arrays[0].numel()
    for a in arrays:
        _dev(a, 'array')
        if a.dtype != torch.float64 or not a.is_contiguous() or a.numel() != n:
            raise TypeError('select_multi_f64 needs dense float64 tensors of one size')
    ptrs = (ctypes.c_void_p * len(arrays))(*[a.data_ptr() for a in arrays])
    rk = (ctypes.c_int64 * len(ranks))(*[int(r) for r in ranks])
    need = lib.shg_select_workspace_bytes(len(ranks))
    ws = torch.empty(need, dtype=torch.uint8, device=arrays[0].device)
    out = torch.empty(len(ranks), dtype=torch.float64, device=arrays[0].device)
    _lib.check(lib.shg_select_multi_f64(ptrs, n, rk, len(ranks), out.data_ptr(), ws.data_ptr(), need, _stream()),
               'shg_select_multi_f64')
    return out


def flood_stats(image, blurred, very_bright):
    """-> (stats float64 [3] = sum(image), min, max of blurred[blurred < very_bright]; counts int32 [20]) on the GPU."""
    _dev(image, 'image')
    _dev(blurred, 'blurred')
    if image.dtype != torch.float64 or blurred.dtype != torch.float64 or image.shape != blurred.shape:
        raise TypeError('flood_stats needs two dense float64 images of one shape')
    stats = torch.empty(3, dtype=torch.float64, device=image.device)
    counts = torch.empty(20, dtype=torch.int32, device=image.device)
    ws = torch.empty(32, dtype=torch.int64, device=image.device)
    _lib.check(lib.shg_flood_stats_f64(image.contiguous().data_ptr(), blurred.contiguous().data_ptr(), image.numel(),
                                       float(very_bright), stats.data_ptr(), counts.data_ptr(), ws.data_ptr(), _stream()),
               'shg_flood_stats_f64')
    return stats, counts


def flood_stats_lerp(image, blurred, order_stats, gamma):
    """flood_stats with very_bright = lerp of two device-resident order statistics (np.percentile's last step):
    the 99th percentile never travels to the host."""
    _dev(image, 'image')
    _dev(blurred, 'blurred')
    _dev(order_stats, 'order_stats')
    if image.dtype != torch.float64 or blurred.dtype != torch.float64 or image.shape != blurred.shape:
        raise TypeError('flood_stats needs two dense float64 images of one shape')
    if order_stats.dtype != torch.float64 or order_stats.numel() != 2 or not order_stats.is_contiguous():
        raise TypeError('order_stats must be two contiguous float64 values')
    stats = torch.empty(3, dtype=torch.float64, device=image.device)
    counts = torch.empty(20, dtype=torch.int32, device=image.device)
    ws = torch.empty(32, dtype=torch.int64, device=image.device)
    _lib.check(lib.shg_flood_stats_lerp_f64(image.contiguous().data_ptr(), blurred.contiguous().data_ptr(), image.numel(),
                                            order_stats.data_ptr(), float(gamma), stats.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                            _stream()), 'shg_flood_stats_lerp_f64')
    return stats, counts


def edge_components(low_mask, high_mask, prefetch=16384):
    """Hysteresis + labelling on the GPU.  -> (idx int32 [m], root int32 [m]) HOST arrays: the surviving edge
    pixels in raster order (idx = y*w + x) and the root (smallest linear index) of each pixel's component."""
    _dev(low_mask, 'low_mask')
    if low_mask.dtype != torch.uint8 or high_mask.dtype != torch.uint8 or low_mask.shape != high_mask.shape:
        raise TypeError('edge_components needs two uint8 masks of one shape')
    h, w = low_mask.shape
    n = h * w
    need = lib.shg_edge_components_workspace_bytes(h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=low_mask.device)
    out = torch.empty(2 * n + 1, dtype=torch.int32, device=low_mask.device)      # [count | idx[n] | root[n]]
    _lib.check(lib.shg_edge_components(low_mask.contiguous().data_ptr(), high_mask.contiguous().data_ptr(), h, w,
                                       out[1:].data_ptr(), out[1 + n:].data_ptr(), out.data_ptr(), ws.data_ptr(), need,
                                       _stream()), 'shg_edge_components')
    k = min(prefetch, n)
    head = torch.cat([out[:1 + k], out[1 + n:1 + n + k]]).cpu().numpy()          # one read covers the usual ~1500 points
    m = int(head[0])
    if m <= k:
        return head[1:1 + m], head[1 + k:1 + k + m]
    return out[1:1 + m].cpu().numpy(), out[1 + n:1 + n + m].cpu().numpy()


def limb_prepare(disk, k, ranks4, gamma99):
    """shg_limb_prepare (csrc/limb_fused.hip): the block mean of the uint16 disk, cv2.blur with windows k and 5, their order
    statistics and the flood statistics in five launches.  -> (packed float64 [32] on the GPU: [0..3] order statistics, [4] sum,
    [5] min, [6] max, 20 uint32 counts from packed[8]; keys int32 [sh, sw]: the window sums of blur k; the workspace that
    holds them)."""
    import ctypes
    ptr, h, w, pitch = _img(disk, 'disk', torch.uint16)
    sh, sw = -(-h // 4), -(-w // 4)
    need = lib.shg_limb_prepare_workspace_bytes(sh, sw, int(k))
    if need == 0:
        raise ValueError('limb_prepare: a %d x %d window is outside the fused path' % (k, k))
    ws = torch.empty(need, dtype=torch.uint8, device=disk.device)
    packed = torch.zeros(32, dtype=torch.float64, device=disk.device)
    rk = (ctypes.c_int64 * 4)(*[int(r) for r in ranks4])
    keys_ptr = ctypes.c_void_p()
    _lib.check(lib.shg_limb_prepare(ptr, h, w, pitch, int(k), rk, float(gamma99), packed.data_ptr(), ctypes.byref(keys_ptr), ws.data_ptr(),
                                    need, _stream()), 'shg_limb_prepare')
    off = keys_ptr.value - ws.data_ptr()
    keys = ws[off:off + sh * sw * 4].view(torch.int32).view(sh, sw)
    return packed, keys, ws


def limb_edges(keys, k, flood_thresh, sigma, low, high):
    """shg_limb_edges: canny and the labelling of its low mask from the window sums of the blurred image, three launches.
    -> (idx int32 [m], root int32 [m], high bool [m]) HOST arrays: the LOW-mask pixels in raster order, the smallest linear index
    of each pixel's component, and whether the pixel is in the HIGH mask."""
    import ctypes
    _dev(keys, 'keys')
    sh, sw = keys.shape
    n = sh * sw
    taps, radius = gaussian_taps(sigma)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    need = lib.shg_limb_edges_workspace_bytes(sh, sw)
    ws = torch.empty(need, dtype=torch.uint8, device=keys.device)
    comp = torch.zeros(2 * n + 1, dtype=torch.int32, device=keys.device)
    _lib.check(lib.shg_limb_edges(keys.data_ptr(), sh, sw, int(k), float(flood_thresh), taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                  radius, float(low), float(high), comp.data_ptr(), ws.data_ptr(), need, _stream()), 'shg_limb_edges')
    host = comp.cpu().numpy()
    m = int(host[0])
    idx, root = host[1:1 + m], host[1 + n:1 + n + m]
    return idx, root & 0x3fffffff, (root >> 30 & 1).astype(bool)


def select_u16(img, ranks, out=None):
    """-> float64 GPU tensor: the ranks[i]-th smallest pixels (0-based) of a uint16 image."""
    import ctypes
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    ranks = [int(r) for r in ranks]
    arr = (ctypes.c_int64 * len(ranks))(*ranks)
    need = lib.shg_select_u16_workspace_bytes(len(ranks))
    if need == 0:
        raise ValueError('select_u16 takes 1..8 ranks')
    ws = torch.empty(need, dtype=torch.uint8, device=img.device)
    if out is None:
        out = torch.empty(len(ranks), dtype=torch.float64, device=img.device)
    _lib.check(lib.shg_select_u16(ptr, h, w, pitch, arr, len(ranks), out.data_ptr(), ws.data_ptr(), need, _stream()),
               'shg_select_u16')
    return out


def stream_read_ceiling(buf, mode=0, vecs_per_frame=0, shapes=None, reps=5):
    """Measured HBM read ceiling in GB/s: best of a few launch shapes of a trivial read-only kernel over `buf`
    (a dense GPU tensor, ideally the frame stack itself).  mode 0: contiguous sweep (shapes = (workgroups, unroll));
    mode 2: pass A's frame-walking addresses (shapes = (frame splits, unroll)).  Returns (GB/s, best shape)."""
    _dev(buf, 'buf')
    if shapes is None:
        shapes = (((384, 4), (512, 4), (768, 4), (1024, 4), (768, 2), (1536, 2), (2048, 2), (512, 8)) if mode != 2
                  else ((1, 8), (2, 4), (1, 4), (2, 2), (3, 2), (4, 2), (2, 8), (3, 4)))
    nbytes = buf.numel() * buf.element_size()
    out = torch.zeros(1024, dtype=torch.int32, device=buf.device)
    best = (0.0, None)
    for blocks, unroll in shapes:
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(lib.shg_stream_read_probe(buf.data_ptr(), nbytes, int(mode), int(blocks), int(unroll), int(vecs_per_frame),
                                                 out.data_ptr(), _stream()), 'shg_stream_read_probe')
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        rate = nbytes / (min(times[1:]) * 1e-3) / 1e9
        if rate > best[0]:
            best = (rate, (blocks, unroll))
    return best


# ---- the spectral analyser (not on the SHG path) ------------------------------------------------
def atlas_correlate(atlas_y, first, step_d, anchor_wavelength, anchor_x, log_spectrum, fill_lo, fill_hi, scales, row_guesses=()):
    """The auto-dispersion loop of spectralAnalyserUI.py:271-300 (shg_atlas_correlate): atlas_y uint8 [n], log_spectrum float32 [w]
    (window filled), scales float64 [G], all on one GPU -> (corr float64 [G], run int32 [G, 2], rows float64 [len(row_guesses), w]
    holding the filled interpolated rows of those guesses, or None)."""
    _dev(atlas_y, 'atlas_y')
    _dev(log_spectrum, 'log_spectrum')
    _dev(scales, 'scales')
    for t, name, dt in ((atlas_y, 'atlas_y', torch.uint8), (log_spectrum, 'log_spectrum', torch.float32), (scales, 'scales', torch.float64)):
        if t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
            raise TypeError('%s must be a contiguous 1-D %s tensor' % (name, dt))
    dev = scales.device
    g, w = scales.shape[0], log_spectrum.shape[0]
    corr = torch.empty(g, dtype=torch.float64, device=dev)
    run = torch.empty((g, 2), dtype=torch.int32, device=dev)
    row_guesses = [int(i) for i in row_guesses]
    rows = slot = None
    if row_guesses:
        if min(row_guesses) < 0 or max(row_guesses) >= g or len(set(row_guesses)) != len(row_guesses):
            raise ValueError('row_guesses must be distinct guess indices below %d' % g)
        m = np.full(g, -1, dtype=np.int32)
        m[row_guesses] = np.arange(len(row_guesses), dtype=np.int32)
        slot = torch.from_numpy(m).to(dev)
        rows = torch.empty((len(row_guesses), w), dtype=torch.float64, device=dev)
    _lib.check(lib.shg_atlas_correlate(atlas_y.data_ptr(), atlas_y.shape[0], float(first), float(step_d), float(anchor_wavelength),
                                       float(anchor_x), log_spectrum.data_ptr(), w, int(fill_lo), int(fill_hi), scales.data_ptr(), g,
                                       corr.data_ptr(), run.data_ptr(), None if slot is None else slot.data_ptr(), len(row_guesses),
                                       None if rows is None else rows.data_ptr(), _stream()), 'shg_atlas_correlate')
    return corr, run, rows


# ---- the Dopplergram and the line-profile maps ------------------------------------------------------
LINE_PROFILE_PLANES = ('shift', 'core', 'width', 'cog', 'ew')


def _line_map_setup(stack, fit, n_cols, k_offset, out, planes=()):
    """What line_core_shift and line_profile share -> (n, h, w, bpp, fit as a contiguous float64 [ih, 4] tensor on the stack's device,
    n_cols, out float32 [*planes, ih, n_cols]: the caller's, or a view of a new row-pitched buffer, NaN when this call does not fill it)."""
    n, h, w, bpp = stack_geometry(stack)
    dev = stack.device
    ih = max(h, w)
    fit = torch.as_tensor(np.ascontiguousarray(fit, dtype=np.float64) if not isinstance(fit, torch.Tensor) else fit).to(dev)
    if fit.dtype != torch.float64 or tuple(fit.shape) != (ih, 4):
        raise ValueError('fit must be float64 [%d, 4]' % ih)
    n_cols = n if n_cols is None else int(n_cols)
    shape = tuple(planes) + (ih, n_cols)
    if out is None:
        pitch = (n_cols + 63) // 64 * 64
        out = torch.empty(shape[:-1] + (pitch,), dtype=torch.float32, device=dev)[..., :n_cols]
        if n_cols != n or int(k_offset) != 0:
            out.fill_(float('nan'))
    if tuple(out.shape) != shape or out.dtype != torch.float32 or out.stride(-1) != 1:
        raise ValueError('out must be a float32 [%s] view with unit column stride' % ', '.join(str(d) for d in shape))
    return n, h, w, bpp, fit.contiguous(), n_cols, out


def _finish_setup(out_w, circle, crop):
    """What doppler_finish and line_profile_finish share -> (nw: the output width after crop_plan's crop, circle as a host float64
    [3] array, crop as a host int64 [4] array; None where not given).  The caller keeps the arrays alive across the C call."""
    nw = int(out_w) if crop is None else int(crop[0])
    c3 = None if circle is None else np.ascontiguousarray([float(v) for v in circle], dtype=np.float64)
    c4 = None if crop is None else np.ascontiguousarray([int(v) for v in crop], dtype=np.int64)
    return nw, c3, c4


def _host_ptr(a):
    return None if a is None else a.ctypes.data


def line_core_shift(stack, fit, half_width, flip_x=False, n_cols=None, k_offset=0, out=None):
    """shg_line_core_shift: the line-core shift (pixels, float32) of every slit row and frame -> map [ih, n_cols] (a view of a
    row-pitched buffer; columns of frames this call does not hold stay NaN).  fit float64 [ih, 4] (host array or GPU tensor)."""
    n, h, w, bpp, fit, n_cols, out = _line_map_setup(stack, fit, n_cols, k_offset, out)
    _lib.check(lib.shg_line_core_shift(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), fit.data_ptr(), int(half_width),
                                       int(bool(flip_x)), out.data_ptr(), out.stride(0), n_cols, int(k_offset), _stream()),
               'shg_line_core_shift')
    return out


def doppler_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, display_range=None):
    """shg_doppler_finish: the raw map float32 [ih, N] resampled as the ellipse -> circle warp (mat3 row 0: h00 h01 h02) with NaN
    for taps outside, masked outside `circle` (cx, cy, r; None or (-1, -1, -1): no mask), cropped / padded by `crop` (crop_plan's
    (nw, lo, dx0, n), None: none) with NaN -> (map float32 [out_h, nw], png uint16 [out_h, nw] or None).  display_range R: also the
    16-bit display plane, 0 for NaN, clip(rint(32768 + d * 32767 / R), 1, 65535) elsewhere."""
    ptr, h, w, pitch = _img(raw, 'raw', torch.float32)
    nw, c3, c4 = _finish_setup(out_w, circle, crop)
    out = torch.empty((int(out_h), nw), dtype=torch.float32, device=raw.device)
    png = None if display_range is None else torch.empty(out.shape, dtype=torch.uint16, device=raw.device)
    _lib.check(lib.shg_doppler_finish(ptr, h, w, pitch, float(h00), float(h01), float(h02), int(out_h), int(out_w), _host_ptr(c3),
                                      _host_ptr(c4), out.data_ptr(), out.stride(0), None if png is None else png.data_ptr(), nw,
                                      0.0 if display_range is None else float(display_range), _stream()), 'shg_doppler_finish')
    return out, png


def line_profile(stack, fit, half_width, shift=0, flip_x=False, n_cols=None, k_offset=0, out=None):
    """shg_line_profile: the five planes (LINE_PROFILE_PLANES, float32) of every slit row and frame, measured around the line
    shifted by `shift` pixels -> planes [5, ih, n_cols] (a view of a row-pitched buffer; columns of frames this call does not hold
    stay NaN).  fit float64 [ih, 4] (host array or GPU tensor)."""
    n, h, w, bpp, fit, n_cols, out = _line_map_setup(stack, fit, n_cols, k_offset, out, (len(LINE_PROFILE_PLANES),))
    _lib.check(lib.shg_line_profile(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), fit.data_ptr(), int(half_width), int(shift),
                                    int(bool(flip_x)), out.data_ptr(), out.stride(0), out.stride(1), n_cols, int(k_offset), _stream()),
               'shg_line_profile')
    return out


def _planes_finish(fn, planes, dims, raw, h00, h01, h02, out_h, out_w, circle, crop, half_width, display_range, *levels):
    """What line_profile_finish and line_bisector_finish share: raw float32 [planes, h, w] (`dims` names the count in the message)
    through the C call `fn` (`levels`: its arguments after the raw plane stride) -> (maps float32 [planes, out_h, nw], png uint16
    [planes, out_h, nw] or None)."""
    _dev(raw, 'raw')
    if raw.dim() != 3 or raw.shape[0] != planes or raw.dtype != torch.float32 or raw.stride(2) != 1:
        raise ValueError('raw must be a float32 [%s, h, w] view with unit column stride' % dims)
    if (half_width is None) != (display_range is None):
        raise ValueError('the display planes need both half_width and display_range')
    _, h, w = raw.shape
    nw, c3, c4 = _finish_setup(out_w, circle, crop)
    out = torch.empty((planes, int(out_h), nw), dtype=torch.float32, device=raw.device)
    png = None if display_range is None else torch.empty(out.shape, dtype=torch.uint16, device=raw.device)
    _lib.check(getattr(lib, fn)(raw.data_ptr(), raw.stride(0), *levels, h, w, raw.stride(1), float(h00), float(h01), float(h02),
                                int(out_h), int(out_w), _host_ptr(c3), _host_ptr(c4), out.data_ptr(), out.stride(0), out.stride(1),
                                None if png is None else png.data_ptr(), out.stride(0), out.stride(1),
                                0 if half_width is None else int(half_width), 0.0 if display_range is None else float(display_range),
                                _stream()), fn)
    return out, png


def line_profile_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, half_width=None, display_range=None):
    """shg_line_profile_finish: the five raw planes float32 [5, ih, N] through doppler_finish's geometry, all in one launch ->
    (maps float32 [5, out_h, nw], png uint16 [5, out_h, nw] or None).  With half_width H and display_range R also the display
    planes: 0 for NaN; shift and cog as the Dopplergram's, core clip(rint(v), 1, 65535), width and ew
    clip(rint(1 + v * 65534 / (2H + 1)), 1, 65535)."""
    return _planes_finish('shg_line_profile_finish', len(LINE_PROFILE_PLANES), '5', raw, h00, h01, h02, out_h, out_w, circle, crop,
                          half_width, display_range)


def line_bisector(stack, fit, half_width, levels, shift=0, flip_x=False, n_cols=None, k_offset=0, out=None):
    """shg_line_bisector: the bisector (pixels from fit[y, 3] + shift) and the chord (pixels) at each of K = len(levels) depths of
    the line, for every slit row and frame, measured around the line shifted by `shift` pixels -> planes [2K, ih, n_cols], planes
    0 .. K-1 the bisectors and K .. 2K-1 the chords (a view of a row-pitched buffer; columns of frames this call does not hold stay
    NaN).  levels: fractions from the core (0) to the continuum (1), checked by the C call.  fit float64 [ih, 4]."""
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).reshape(-1))
    n, h, w, bpp, fit, n_cols, out = _line_map_setup(stack, fit, n_cols, k_offset, out, (2 * lv.size,))
    _lib.check(lib.shg_line_bisector(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), fit.data_ptr(), int(half_width), int(shift),
                                     _host_ptr(lv) if lv.size else None, int(lv.size), int(bool(flip_x)), out.data_ptr(),
                                     out.stride(0), out.stride(1), n_cols, int(k_offset), _stream()), 'shg_line_bisector')
    return out


def line_bisector_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, half_width=None, display_range=None):
    """shg_line_bisector_finish: the 2K raw planes float32 [2K, ih, N] of line_bisector through doppler_finish's geometry, all in one
    launch -> (maps float32 [2K, out_h, nw], png uint16 [2K, out_h, nw] or None).  With half_width H and display_range R also the
    display planes: 0 for NaN; the bisectors as the Dopplergram's shift, the chords clip(rint(1 + v * 65534 / (2H + 1)), 1, 65535)."""
    planes = raw.shape[0] if isinstance(raw, torch.Tensor) and raw.dim() == 3 and raw.shape[0] % 2 == 0 else -1
    return _planes_finish('shg_line_bisector_finish', planes, '2K', raw, h00, h01, h02, out_h, out_w, circle, crop, half_width,
                          display_range, planes // 2)


# ---- the emission-line maps ---------------------------------------------------------------------------
LINE_EMISSION_PLANES = ('shift', 'peak', 'width', 'cog', 'flux')


def line_emission(stack, fit, half_width, shift=0, min_excess=0.0, flip_x=False, n_cols=None, k_offset=0, out=None):
    """shg_line_emission: the five planes (LINE_EMISSION_PLANES, float32) of a line seen in emission, for every slit row and frame,
    measured around the line shifted by `shift` pixels -> planes [5, ih, n_cols] as line_profile's.  Every plane is NaN unless the
    window's first maximum is bracketed and rises min_excess (sample units, finite and >= 0) above the mean of the window's end
    samples.  fit float64 [ih, 4] (host array or GPU tensor)."""
    n, h, w, bpp, fit, n_cols, out = _line_map_setup(stack, fit, n_cols, k_offset, out, (len(LINE_EMISSION_PLANES),))
    _lib.check(lib.shg_line_emission(stack.data_ptr(), n, h, w, bpp, frame_stride(stack), fit.data_ptr(), int(half_width), int(shift),
                                     float(min_excess), int(bool(flip_x)), out.data_ptr(), out.stride(0), out.stride(1), n_cols,
                                     int(k_offset), _stream()), 'shg_line_emission')
    return out


def line_emission_finish(raw, h00, h01, h02, out_h, out_w, ring=None, crop=None, half_width=None, display_range=None):
    """shg_line_emission_finish: the five raw planes float32 [5, ih, N] of line_emission through doppler_finish's geometry, NaN on
    and inside the circle of radius r_in and outside the one of radius r_out of `ring` (cx, cy, r_in, r_out; None: no mask; r_in < 0:
    no inner mask; r_out may be inf) -> (maps float32 [5, out_h, nw], png uint16 [5, out_h, nw] or None).  Display planes with
    half_width H and display_range R: 0 for NaN; shift and cog as the Dopplergram's, peak clip(rint(v), 1, 65535), width
    clip(rint(1 + v * 65534 / (2H + 1)), 1, 65535), flux clip(rint(v / (2H + 1)), 1, 65535)."""
    if ring is not None and len(ring) != 4:
        raise ValueError('ring is (cx, cy, r_in, r_out)')
    return _planes_finish('shg_line_emission_finish', len(LINE_EMISSION_PLANES), '5', raw, h00, h01, h02, out_h, out_w, ring, crop,
                          half_width, display_range)


# ---- removing a fitted plane from a finished map -----------------------------------------------------
def map_plane_moments(m, circle=None, prev=None, out=None):
    """shg_map_plane_moments: the ten integer moments {N, sum c, sum r, sum c^2, sum c r, sum r^2, sum q, sum q c, sum q r, sum q^2}
    (q = rint(4096 v)) of the used pixels of the map float32 [h, w] -> int64 [10] on the map's device (`out`: the caller's,
    overwritten).  Used: finite, |v| < 64, inside `circle` (cx, cy, r; None or (-1, -1, -1): no mask) and, with prev = (a, b, g,
    limit), within limit of that plane."""
    ptr, h, w, pitch = _img(m, 'map', torch.float32)
    c3 = _circle3_or_none(circle)
    p4 = None if prev is None else np.ascontiguousarray([float(v) for v in prev], dtype=np.float64)
    if p4 is not None and p4.size != 4:
        raise ValueError('circle is (cx, cy, r) and prev is (a, b, g, limit)')
    out = _int64_out(out, (10,), m.device)
    _lib.check(lib.shg_map_plane_moments(ptr, h, w, pitch, _host_ptr(c3), _host_ptr(p4), out.data_ptr(), _stream()),
               'shg_map_plane_moments')
    return out


def map_detrend(m, plane, display_range=None, out=None):
    """shg_map_detrend: the map float32 [h, w] minus the plane (a, b, g): a + b * column + g * row -> (out float32 [h, w], png uint16
    [h, w] or None).  out: the caller's view (the map itself: in place), else a new one.  display_range R: also the 16-bit display
    plane of the output, as doppler_finish's."""
    ptr, h, w, pitch = _img(m, 'map', torch.float32)
    p3 = np.ascontiguousarray([float(v) for v in plane], dtype=np.float64)
    if p3.size != 3:
        raise ValueError('plane is (a, b, g)')
    out, optr, opitch = _out_like(out, h, w, torch.float32, m.device)
    png = None if display_range is None else torch.empty((h, w), dtype=torch.uint16, device=m.device)
    _lib.check(lib.shg_map_detrend(ptr, h, w, pitch, _host_ptr(p3), optr, opitch, None if png is None else png.data_ptr(), w,
                                   0.0 if display_range is None else float(display_range), _stream()), 'shg_map_detrend')
    return out, png


# ---- flattening the disk: ring medians and the division by the radial profile -------------------------
def _circle3(circle):
    """(circle as a host float64 [3] array, K = floor(rad) + 1 rings)."""
    c3 = np.ascontiguousarray([float(v) for v in circle], dtype=np.float64)
    if c3.size != 3:
        raise ValueError('circle is (cx, cy, r)')
    if not (np.isfinite(c3).all() and 0.0 <= c3[2] < 16384.0):
        raise ValueError('circle (%r, %r, %r) must be finite with a radius in [0, 16384)' % tuple(c3))
    return c3, int(np.floor(c3[2])) + 1


def _circle3_or_none(circle):
    """The optional disk of a pixel set as a host float64 [3] array, or None."""
    c3 = None if circle is None else np.ascontiguousarray([float(v) for v in circle], dtype=np.float64)
    if c3 is not None and c3.size != 3:
        raise ValueError('circle is (cx, cy, r)')
    return c3


def ring_medians_u16(img, circle, out=None):
    """shg_ring_medians_u16: for each of the K = floor(r) + 1 one-pixel rings around the centre of `circle` (cx, cy, r), over the
    pixels of the uint16 image that lie on the disk -> (count uint32 [K], lo uint16 [K], hi uint16 [K]) on the image's device: the
    ring's pixels, its (n - 1) / 2-th and its n / 2-th smallest value (the median is (lo + hi) / 2; both 0 for an empty ring).
    out: the caller's three tensors, overwritten."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    c3, k = _circle3(circle)
    if out is None:
        out = (torch.empty(k, dtype=torch.uint32, device=img.device), torch.empty(k, dtype=torch.uint16, device=img.device),
               torch.empty(k, dtype=torch.uint16, device=img.device))
    count, lo, hi = out
    for t, dt in ((count, torch.uint32), (lo, torch.uint16), (hi, torch.uint16)):
        if _dev(t, 'out').dtype != dt or tuple(t.shape) != (k,) or not t.is_contiguous():
            raise ValueError('out is (count uint32 [%d], lo uint16 [%d], hi uint16 [%d]), contiguous' % (k, k, k))
    ws, ws_bytes = _workspace(None, lib.shg_ring_medians_u16_workspace_bytes(k), img.device)
    _lib.check(lib.shg_ring_medians_u16(ptr, h, w, pitch, _host_ptr(c3), k, count.data_ptr(), lo.data_ptr(), hi.data_ptr(), ws.data_ptr(),
                                        ws_bytes, _stream()), 'shg_ring_medians_u16')
    return count, lo, hi


def ring_flatten_u16(img, circle, gain, out=None):
    """shg_ring_flatten_u16: every on-disk pixel of the uint16 image times the gain of its radius (gain float64 [K] on the host,
    gain[k] at radius k + 1/2, linear in between, constant beyond either end), rounded to nearest even and saturated; pixels off
    the disk as they are -> uint16 [h, w].  out: the caller's view (the image itself: in place), else a new one."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    c3, k = _circle3(circle)
    g = np.ascontiguousarray(gain, dtype=np.float64).reshape(-1)
    if g.size != k:
        raise ValueError('gain must hold %d values (floor(r) + 1), got %d' % (k, g.size))
    out, optr, opitch = _out_like(out, h, w, torch.uint16, img.device)
    _lib.check(lib.shg_ring_flatten_u16(ptr, h, w, pitch, _host_ptr(c3), _host_ptr(g), k, optr, opitch, _stream()),
               'shg_ring_flatten_u16')
    return out


# ---- stacking a series of scans: resample-and-combine, and the SSD over a window of integer offsets ----
STACK_MODES = {'mean': 0, 'median': 1, 'sigma': 2}


def lattice_shape(shape, step):
    """(gh, gw) of the lattice of `step` pixels that covers a grid of `shape`: nodes at every multiple of `step`, the last at or past the last pixel."""
    oh, ow, step = int(shape[0]), int(shape[1]), int(step)
    return (oh - 1 + step - 1) // step + 1, (ow - 1 + step - 1) // step + 1


def _lattices(tensors, who, what, shape):
    """The node pointers of one optional lattice a source (None: a null pointer), each a contiguous float64 tensor of `shape`."""
    for t in tensors:
        if t is not None and (_dev(t, who).dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError('a %s is None or a contiguous float64 [%s] tensor' % (what, ', '.join('%d' % v for v in shape)))
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _stack_combine(fn, images, transforms, fields, weights, step, shape, mode, kappa, iterations, out, count, want_count):
    """What the three combines share: the checks, the marshalling and the call of the entry point `fn`.  step None: the plain
    combine, without a lattice; weights None: without weight lattices (with them, fields None is no field for any image)."""
    if mode not in STACK_MODES:
        raise ValueError('mode is one of %s, got %r' % (', '.join(STACK_MODES), mode))
    if weights is not None and mode == 'median':
        raise ValueError('there is no weighted median: mode is mean or sigma')
    images = list(images)
    n = len(images)
    xf = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(-1, 4))
    given = ['%d images' % n, '%d transforms (s, tx, ty, gain)' % xf.shape[0]]
    lengths = [n, xf.shape[0]]
    if step is not None:
        fields = [None] * n if fields is None and weights is not None else list(fields)
        given.append('%d fields' % len(fields)), lengths.append(len(fields))
    if weights is not None:
        weights = list(weights)
        given.append('%d weight lattices' % len(weights)), lengths.append(len(weights))
    if n < 1 or lengths != [n] * len(lengths):
        raise ValueError(', '.join(given[:-1]) + ' and ' + given[-1])
    if step is not None and not 8 <= int(step) <= 128:
        raise ValueError('step must be 8 to 128, got %r' % (step,))
    geo = [_img(t, 'image', torch.uint16) for t in images]
    dev = images[0].device
    oh, ow = int(shape[0]), int(shape[1])
    lattice = ()
    if step is not None:
        gh, gw = lattice_shape((oh, ow), step)
        fptrs = _lattices(fields, 'field', 'field', (gh, gw, 2))
        if weights is None:
            lattice = (fptrs, gh, gw, int(step))
        else:
            wptrs = _lattices(weights, 'weights', 'weight lattice', (gh, gw))
            lattice = (None if all(f is None for f in fields) else fptrs, wptrs, gh, gw, int(step))
    out, optr, opitch = _out_like(out, oh, ow, torch.uint16, dev)
    cptr, cpitch = None, 0
    if count is not None or want_count:
        count, cptr, cpitch = _out_like(count, oh, ow, torch.uint8, dev, 'count')
    ptrs = (ctypes.c_void_p * n)(*[g[0] for g in geo])
    dims = np.ascontiguousarray([[g[1], g[2], g[3]] for g in geo], dtype=np.int64)
    _lib.check(getattr(lib, fn)(ptrs, _host_ptr(dims), _host_ptr(xf), *lattice, n, STACK_MODES[mode], float(kappa), int(iterations), optr,
                                oh, ow, opitch, cptr, cpitch, _stream()), fn)
    return out, count


def stack_combine_u16(images, transforms, shape, mode='sigma', kappa=2.5, iterations=2, out=None, count=None, want_count=True):
    """shg_stack_combine_u16: the N uint16 images (2-D views, any sizes) resampled into one grid of `shape` = (oh, ow) by their
    transforms -- N rows (s, tx, ty, gain): the output pixel (r, c) reads source j at (tx + s c, ty + s r), bilinear, times gain --
    and combined pixel by pixel in one launch; mode 'mean', 'median' or 'sigma' (the kappa-sigma clipped mean, `iterations` passes)
    -> (out uint16 [oh, ow], count uint8 [oh, ow] or None): the samples that went into each pixel.  out, count: the caller's
    views."""
    return _stack_combine('shg_stack_combine_u16', images, transforms, None, None, None, shape, mode, kappa, iterations, out, count,
                          want_count)


def shift_ssd_u16(ref, img, search, circle=None, out=None):
    """shg_shift_ssd_u16: the sums of squared differences between two uint16 images of one shape, for every integer offset (u, v)
    with |u|, |v| <= search (0 to 8): out[(v + S) (2 S + 1) + (u + S)] = sum (ref[r, c] - img[r + v, c + u])^2 over the pixels at
    least S from every edge and, with `circle` (cx, cy, r; None or (-1, -1, -1): none), on that disk; out[(2 S + 1)^2] = how many
    -> int64 [(2 S + 1)^2 + 1] on the images' device (the sums stay below 2^60).  out: the caller's, overwritten."""
    rptr, h, w, rpitch = _img(ref, 'ref', torch.uint16)
    iptr, ih, iw, ipitch = _img(img, 'img', torch.uint16)
    if (ih, iw) != (h, w):
        raise ValueError('ref [%d, %d] and img [%d, %d] must have one shape' % (h, w, ih, iw))
    s = int(search)
    if not 0 <= s <= 8:
        raise ValueError('search must be 0 to 8, got %r' % (search,))
    c3 = _circle3_or_none(circle)
    out = _int64_out(out, ((2 * s + 1) ** 2 + 1,), ref.device)
    _lib.check(lib.shg_shift_ssd_u16(rptr, rpitch, iptr, ipitch, h, w, s, _host_ptr(c3), out.data_ptr(), _stream()), 'shg_shift_ssd_u16')
    return out


# ---- local alignment points: one SSD table a patch, and the combine with a displacement field a source ----
def patch_ssd_u16(ref, img, points, half, search, circle=None, out=None):
    """shg_patch_ssd_u16: for each of the n points (row, col) -- an int32 [n, 2] tensor on the images' device, or a host array that
    is uploaded -- the sums of squared differences between the (2 half + 1)^2 patch of `ref` around it and `img`, for every integer
    offset (u, v) with |u|, |v| <= search (0 to 8), over the patch's pixels at least `search` from every edge and, with `circle`, on
    that disk -> int64 [n, (2 S + 1)^2 + 3] on the images' device: the sums, then the pixels of the set, the sum of ref and the sum
    of ref^2 over it (a row of zeros for an empty set).  half is 1 to 32.  out: the caller's, overwritten."""
    rptr, h, w, rpitch = _img(ref, 'ref', torch.uint16)
    iptr, ih, iw, ipitch = _img(img, 'img', torch.uint16)
    if (ih, iw) != (h, w):
        raise ValueError('ref [%d, %d] and img [%d, %d] must have one shape' % (h, w, ih, iw))
    b, s = int(half), int(search)
    if not 1 <= b <= 32:
        raise ValueError('half must be 1 to 32, got %r' % (half,))
    if not 0 <= s <= 8:
        raise ValueError('search must be 0 to 8, got %r' % (search,))
    points, n = _points(points, ref.device)
    c3 = _circle3_or_none(circle)
    out = _int64_out(out, (n, (2 * s + 1) ** 2 + 3), ref.device)
    _lib.check(lib.shg_patch_ssd_u16(rptr, rpitch, iptr, ipitch, h, w, points.data_ptr(), n, b, s, _host_ptr(c3), out.data_ptr(), _stream()),
               'shg_patch_ssd_u16')
    return out


def stack_combine_field_u16(images, transforms, fields, step, shape, mode='sigma', kappa=2.5, iterations=2, out=None, count=None,
                            want_count=True):
    """shg_stack_combine_field_u16: stack_combine_u16 with a displacement field a source.  fields: one entry an image, None (no
    field) or a contiguous float64 [gh, gw, 2] tensor on the images' device, (dx, dy) at the nodes (j step, i step) of the lattice
    lattice_shape(shape, step); step is 8 to 128.  The output pixel (r, c) reads source j at (tx + s (c + dx), ty + s (r + dy)) with
    (dx, dy) bilinear between the four nodes around it; a displacement that is not finite makes the sample absent; None and a field
    of zeros give stack_combine_u16's result bit for bit -> (out uint16 [oh, ow], count uint8 [oh, ow] or None)."""
    return _stack_combine('shg_stack_combine_field_u16', images, transforms, fields, None, step, shape, mode, kappa, iterations, out,
                          count, want_count)


# ---- ranking scans by sharpness: the sums of a quality figure a patch, and the combine with a weight lattice a source ----
def patch_sharpness_u16(img, points, half, arm, circle=None, out=None):
    """shg_patch_sharpness_u16: for each of the n points (row, col) -- an int32 [n, 2] tensor on the image's device, or a host array
    that is uploaded -- over the pixels of the (2 half + 1)^2 patch of the uint16 image around it that lie at least `arm` from every
    edge and, with `circle`, on that disk -> int64 [n, 4] on the image's device: the pixels of the set, the sum of I, the sum of I^2
    and the sum of L^2 with L = 4 I[r, c] - I[r - arm, c] - I[r + arm, c] - I[r, c - arm] - I[r, c + arm] (a row of zeros for an empty
    set).  half is 1 to 32, arm 1 to 8.  out: the caller's, overwritten."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    b, d = int(half), int(arm)
    if not 1 <= b <= 32:
        raise ValueError('half must be 1 to 32, got %r' % (half,))
    if not 1 <= d <= 8:
        raise ValueError('arm must be 1 to 8, got %r' % (arm,))
    points, n = _points(points, img.device)
    c3 = _circle3_or_none(circle)
    out = _int64_out(out, (n, 4), img.device)
    _lib.check(lib.shg_patch_sharpness_u16(ptr, pitch, h, w, points.data_ptr(), n, b, d, _host_ptr(c3), out.data_ptr(), _stream()),
               'shg_patch_sharpness_u16')
    return out


def stack_combine_weighted_u16(images, transforms, fields, weights, step, shape, mode='sigma', kappa=2.5, iterations=2, out=None, count=None,
                               want_count=True):
    """shg_stack_combine_weighted_u16: stack_combine_field_u16 with a weight lattice a source.  fields: None (no image has one) or one
    entry an image as there; weights: one entry an image, None (weight 1 everywhere) or a contiguous float64 [gh, gw] tensor on the
    images' device, one weight a node of lattice_shape(shape, step), the caller's to keep finite, >= 0 and <= 2^20.  A source's
    weight at a pixel is bilinear between the four nodes around it; a source is present where stack_combine_field_u16 has it and
    its weight is > 0; mode 'mean' or 'sigma' (the clipping does not see the weights; 'median' is a ValueError); the result is
    sum (w v) / sum w over the kept samples in source order and count the kept samples.  Weights of None or 1 give
    stack_combine_field_u16's result bit for bit -> (out uint16 [oh, ow], count uint8 [oh, ow] or None)."""
    return _stack_combine('shg_stack_combine_weighted_u16', images, transforms, fields, weights, step, shape, mode, kappa, iterations,
                          out, count, want_count)


# ---- sharpening a disk: the a-trous wavelet layers with gains and gates, and the noise they are gated by ----
def wavelet_sharpen_u16(img, gain_q8, threshold_q6=None, out=None, want_planes=False, workspace=None):
    """shg_wavelet_sharpen_u16: the uint16 image split into L = len(gain_q8) B3-spline a-trous layers (1 to 6) and put together again,
    layer j times gain_q8[j] / 256 (integers in [0, 4096]) after a soft threshold of threshold_q6[j] (integers in [0, 2^22], 64 a
    count; None: zeros) -> (out uint16 [h, w], planes int32 [L + 1, h, w] or None: w_1 .. w_L, then c_L).  out: the caller's view,
    which must not overlap the image.  workspace: the caller's uint8 tensor of at least wavelet_workspace_bytes(h, w, L)."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    g = np.ascontiguousarray(gain_q8, dtype=np.int64).reshape(-1)
    levels = int(g.size)
    t = np.zeros(levels, np.int64) if threshold_q6 is None else np.ascontiguousarray(threshold_q6, dtype=np.int64).reshape(-1)
    if not 1 <= levels <= 6 or t.size != levels:
        raise ValueError('1 to 6 gains and as many thresholds, got %d and %d' % (levels, t.size))
    if g.min() < 0 or g.max() > 4096 or t.min() < 0 or t.max() > 1 << 22:
        raise ValueError('gain_q8 lies in [0, 4096] and threshold_q6 in [0, 2^22]')
    g, t = g.astype(np.int32), t.astype(np.int32)
    out, optr, opitch = _out_like(out, h, w, torch.uint16, img.device)
    planes = torch.empty((levels + 1, h, w), dtype=torch.int32, device=img.device) if want_planes else None
    ws, ws_bytes = _workspace(workspace, lib.shg_wavelet_workspace_bytes(h, w, levels), img.device)
    _lib.check(lib.shg_wavelet_sharpen_u16(ptr, h, w, pitch, levels, _host_ptr(g), _host_ptr(t), optr, opitch,
                                           None if planes is None else planes.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
               'shg_wavelet_sharpen_u16')
    return out, planes


def wavelet_noise_u16(img, circle=None, out=None, workspace=None):
    """shg_wavelet_noise_u16: over the pixels of the uint16 image on the disk `circle` (cx, cy, r; None or (-1, -1, -1): every
    pixel) -> int64 [2] on the image's device: the lower median of |w_1|, the finest wavelet layer, in Q6 (64 a count), and the
    number of pixels (0 and 0 for an empty set).  out: the caller's, overwritten."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    c3 = _circle3_or_none(circle)
    out = _int64_out(out, (2,), img.device)
    ws, ws_bytes = _workspace(workspace, lib.shg_wavelet_workspace_bytes(h, w, 1), img.device)
    _lib.check(lib.shg_wavelet_noise_u16(ptr, h, w, pitch, _host_ptr(c3), out.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
               'shg_wavelet_noise_u16')
    return out


# ---- deconvolving a disk: Richardson-Lucy with a separable point-spread function ----
def rl_deconvolve_u16(img, taps, iterations, out=None, want_estimate=False, workspace=None):
    """shg_rl_deconvolve_u16: `iterations` (1 to 200) Richardson-Lucy iterations of the uint16 image with the separable blur of the
    2 R + 1 float32 `taps` (R = 0 to 16; each 0 or in [2^-30, 1]; their sum within 2^-10 of 1) -> (out uint16 [h, w], the estimate
    float32 [h, w] before its rounding, or None).  out: the caller's view, which must not overlap the image.  workspace: the caller's
    uint8 tensor of at least shg_rl_workspace_bytes(h, w)."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    k = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if k.size % 2 != 1 or k.size > 33:
        raise ValueError('2 R + 1 taps with R from 0 to 16, got %d' % k.size)
    if not (np.isfinite(k).all() and ((k == 0) | ((k >= np.float32(2.0 ** -30)) & (k <= 1))).all()):
        raise ValueError('a tap is 0 or lies in [2^-30, 1]')
    if abs(float(k.astype(np.float64).sum()) - 1.0) > 2.0 ** -10:
        raise ValueError('the taps sum to %r, more than 2^-10 off 1' % float(k.astype(np.float64).sum()))
    if not (isinstance(iterations, (int, np.integer)) and 1 <= iterations <= 200):
        raise ValueError('iterations is an integer from 1 to 200, got %r' % (iterations,))
    out, optr, opitch = _out_like(out, h, w, torch.uint16, img.device)
    estimate = torch.empty((h, w), dtype=torch.float32, device=img.device) if want_estimate else None
    ws, ws_bytes = _workspace(workspace, lib.shg_rl_workspace_bytes(h, w), img.device)
    _lib.check(lib.shg_rl_deconvolve_u16(ptr, h, w, pitch, _host_ptr(k), k.size // 2, int(iterations), optr, opitch,
                                         None if estimate is None else estimate.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
               'shg_rl_deconvolve_u16')
    return out, estimate


def _rl_taps(taps, axis):
    k = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    if k.size % 2 != 1 or k.size > 33:
        raise ValueError('2 R + 1 taps along %s with R from 0 to 16, got %d' % (axis, k.size))
    if not (np.isfinite(k).all() and ((k == 0) | ((k >= np.float32(2.0 ** -30)) & (k <= 1))).all()):
        raise ValueError('a tap along %s is 0 or lies in [2^-30, 1]' % axis)
    if abs(float(k.astype(np.float64).sum()) - 1.0) > 2.0 ** -10:
        raise ValueError('the taps along %s sum to %r, more than 2^-10 off 1' % (axis, float(k.astype(np.float64).sum())))
    return k


def rl_deconvolve_xy_u16(img, taps_x, taps_y, iterations, out=None, want_estimate=False, workspace=None):
    """shg_rl_deconvolve_xy_u16: rl_deconvolve_u16 with a tap set an axis -- `taps_x` (2 Rx + 1 float32 values) blurs along the columns
    of a row, `taps_y` (2 Ry + 1) down the rows of a column; each set under rl_deconvolve_u16's limits -> (out uint16 [h, w], the
    estimate float32 [h, w] or None).  Equal sets give rl_deconvolve_u16's bits."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    kx, ky = _rl_taps(taps_x, 'x'), _rl_taps(taps_y, 'y')
    if not (isinstance(iterations, (int, np.integer)) and 1 <= iterations <= 200):
        raise ValueError('iterations is an integer from 1 to 200, got %r' % (iterations,))
    out, optr, opitch = _out_like(out, h, w, torch.uint16, img.device)
    estimate = torch.empty((h, w), dtype=torch.float32, device=img.device) if want_estimate else None
    ws, ws_bytes = _workspace(workspace, lib.shg_rl_workspace_bytes(h, w), img.device)
    _lib.check(lib.shg_rl_deconvolve_xy_u16(ptr, h, w, pitch, _host_ptr(kx), kx.size // 2, _host_ptr(ky), ky.size // 2, int(iterations),
                                            optr, opitch, None if estimate is None else estimate.data_ptr(), ws.data_ptr(), ws_bytes,
                                            _stream()), 'shg_rl_deconvolve_xy_u16')
    return out, estimate


# ---- measuring the blur from the limb: the edge-spread tables of the annulus around the circle ----
def sector_thresholds(sectors):
    """The S / 8 - 1 thresholds of shg_limb_profile_u16 for `sectors` = S sectors of equal angle: tan((k + 1) pi / (4 S / 8)) as host
    float64 -- computed once here, so that the library and a restatement are handed the same doubles."""
    if not (isinstance(sectors, (int, np.integer)) and 8 <= sectors <= 64 and sectors % 8 == 0):
        raise ValueError('sectors is a multiple of 8 from 8 to 64, got %r' % (sectors,))
    n = int(sectors) // 8
    return np.tan(np.arange(1, n, dtype=np.float64) * (np.pi / (4.0 * n)))


def limb_profile_u16(img, circle, reach, sub, sectors, thresholds=None):
    """shg_limb_profile_u16: the pixels of the uint16 image within `reach` (1 to 64, at most r - 1) pixels of the limb of `circle`
    (cx, cy, r), binned by sector (`sectors`: a multiple of 8 from 8 to 64, counted from the +column axis towards the +row axis) and by
    distance from the centre in bins of 1 / `sub` (1 to 8) pixel -> (count uint32, sum uint64, sumsq uint64), each
    [sectors, 2 reach sub] on the image's device.  thresholds: sector_thresholds(sectors) unless given."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    c3, _ = _circle3(circle)
    for name, v, lo, hi in (('reach', reach, 1, 64), ('sub', sub, 1, 8)):
        if not (isinstance(v, (int, np.integer)) and lo <= v <= hi):
            raise ValueError('%s is an integer from %d to %d, got %r' % (name, lo, hi, v))
    if not reach <= c3[2] - 1.0:
        raise ValueError('reach is at most rad - 1 = %r, got %r' % (float(c3[2] - 1.0), reach))
    t = sector_thresholds(sectors) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if t.size != sectors // 8 - 1:
        raise ValueError('%d sectors take %d thresholds, got %d' % (sectors, sectors // 8 - 1, t.size))
    shape = (int(sectors), 2 * int(reach) * int(sub))
    count = torch.empty(shape, dtype=torch.uint32, device=img.device)
    total = torch.empty(shape, dtype=torch.uint64, device=img.device)
    sumsq = torch.empty(shape, dtype=torch.uint64, device=img.device)
    _lib.check(lib.shg_limb_profile_u16(ptr, h, w, pitch, _host_ptr(c3), int(reach), int(sub), int(sectors), _host_ptr(t) if t.size else None,
                                        count.data_ptr(), total.data_ptr(), sumsq.data_ptr(), _stream()), 'shg_limb_profile_u16')
    return count, total, sumsq


# ---- limb protection: the image as a disk plane and a sky plane without the limb's step, and the filtered planes put back ----
def _limb_ring(circle, margin):
    """(circle as a host float64 [3] array, margin as a float); ValueError unless rad > 0, margin >= 0 and rad - margin >= 1."""
    c3, _ = _circle3(circle)
    if not (isinstance(margin, (int, float, np.integer, np.floating)) and np.isfinite(margin) and margin >= 0.0):
        raise ValueError('margin is finite and >= 0, got %r' % (margin,))
    if not (c3[2] > 0.0 and c3[2] - float(margin) >= 1.0):
        raise ValueError('rad - margin is at least 1, got a radius of %r and a margin of %r' % (float(c3[2]), margin))
    return c3, float(margin)


def limb_split_u16(img, circle, margin, reach, inner=None, outer=None, want_inner=True, want_outer=True):
    """shg_limb_split_u16: the uint16 image as two planes without the step at the limb of `circle` (cx, cy, r) -> (inner, outer)
    uint16 [h, w]: inner is the image out to r - margin and its point reflection about that edge beyond it, outer the image from
    r + margin outwards and its point reflection inwards; both hold a plateau beyond `reach` (1 to r - margin) pixels from their
    edge.  want_inner / want_outer False: None in that place (not both).  inner, outer: the caller's views, which must overlap
    neither the image nor each other."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    c3, margin = _limb_ring(circle, margin)
    if not (isinstance(reach, (int, float, np.integer, np.floating)) and np.isfinite(reach) and 1.0 <= reach <= c3[2] - margin):
        raise ValueError('reach lies in [1, rad - margin = %r], got %r' % (float(c3[2] - margin), reach))
    if not (want_inner or want_outer):
        raise ValueError('at least one of the two planes')
    iptr = optr = None
    ipitch = opitch = 0
    if want_inner:
        inner, iptr, ipitch = _out_like(inner, h, w, torch.uint16, img.device, 'inner')
    if want_outer:
        outer, optr, opitch = _out_like(outer, h, w, torch.uint16, img.device, 'outer')
    _lib.check(lib.shg_limb_split_u16(ptr, h, w, pitch, _host_ptr(c3), margin, float(reach), iptr, ipitch, optr, opitch, _stream()),
               'shg_limb_split_u16')
    return (inner if want_inner else None), (outer if want_outer else None)


def limb_merge_u16(img, disk, sky, circle, margin, blend, out=None):
    """shg_limb_merge_u16: the filtered planes put back -> uint16 [h, w]: `disk` inside r - margin and `sky` (None: the image)
    beyond r + margin, each blended into the image over `blend` pixels from that edge, and the image itself in between.  out: the
    caller's view, which must overlap none of the three."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    dptr, dh, dw, dpitch = _img(disk, 'disk', torch.uint16)
    sptr, spitch = None, 0
    if sky is not None:
        sptr, sh, sw, spitch = _img(sky, 'sky', torch.uint16)
        if (sh, sw) != (h, w):
            raise ValueError('sky must be a uint16 [%d, %d] view' % (h, w))
    if (dh, dw) != (h, w):
        raise ValueError('disk must be a uint16 [%d, %d] view' % (h, w))
    c3, margin = _limb_ring(circle, margin)
    if not (isinstance(blend, (int, float, np.integer, np.floating)) and np.isfinite(blend) and blend > 0.0):
        raise ValueError('blend is finite and > 0, got %r' % (blend,))
    out, optr, opitch = _out_like(out, h, w, torch.uint16, img.device)
    _lib.check(lib.shg_limb_merge_u16(ptr, pitch, dptr, dpitch, sptr, spitch, h, w, _host_ptr(c3), margin, float(blend), optr, opitch,
                                      _stream()), 'shg_limb_merge_u16')
    return out


# ---- scan jitter along the slit: the limb crossings of every column, and every column resampled along itself ----
COLUMN_LIMB_SEGMENTS = 128        # the row segments a workgroup of shg_column_limb_u16 splits its columns into (csrc/dejitter.hip)
COLUMN_LIMB_COLUMNS = 64          # the columns a workgroup owns
COLUMN_SHIFT_COLUMNS = 256        # the columns a launch of shg_column_shift_u16 carries in its arguments
COLUMN_SHIFT_ROWS = 128           # the rows a workgroup of it handles


def column_limb_segment(h, window):
    """The rows a segment of shg_column_limb_u16 owns for an image of h rows: segment g owns the window sums s[g L .. (g + 1) L - 1],
    L = ceil((h - window + 1) / COLUMN_LIMB_SEGMENTS) -> L (0 when h < window)."""
    ni = int(h) - int(window) + 1
    return max(0, (ni + COLUMN_LIMB_SEGMENTS - 1) // COLUMN_LIMB_SEGMENTS)


def column_limb_u16(img, window, threshold, out=None):
    """shg_column_limb_u16: the two limb crossings of every column of the uint16 image, with s[i] the sum of the `window` (odd, 1 to
    15) rows from i on and A[i] = s[i] >= window * threshold (0 to 65535) -> int32 [w, 6] on the image's device: (i_top, s[i_top - 1],
    s[i_top], i_bot, s[i_bot], s[i_bot + 1]), -1 in all six for a column without a measurement.  out: the caller's, overwritten."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    if not (isinstance(window, (int, np.integer)) and 1 <= window <= 15 and window % 2 == 1):
        raise ValueError('window is an odd integer from 1 to 15, got %r' % (window,))
    if not (isinstance(threshold, (int, np.integer)) and 0 <= threshold <= 65535):
        raise ValueError('threshold is an integer from 0 to 65535, got %r' % (threshold,))
    if out is None:
        out = torch.empty((w, 6), dtype=torch.int32, device=img.device)
    if _dev(out, 'out').dtype != torch.int32 or tuple(out.shape) != (w, 6) or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 [%d, 6] tensor' % w)
    _lib.check(lib.shg_column_limb_u16(ptr, h, w, pitch, int(window), int(threshold), out.data_ptr(), _stream()), 'shg_column_limb_u16')
    return out


def column_shift_u16(planes, offset, weight, out=None):
    """shg_column_shift_u16: every column of the uint16 planes -- [h, w], or [n, h, w] with n from 1 to 64, unit column stride --
    resampled along itself: out[p, r, c] = clip((sum_k weight[c, k] * planes[p, clamp(r + offset[c] + k - 1, 0, h - 1), c] + 8192) >> 14,
    0, 65535).  offset: int32 [w], |offset| <= 16384; weight: int32 [w, 4] in Q14, each in [-4096, 20480], a column's summing to 16384
    (host arrays: they travel in the launches' arguments) -> uint16 of the planes' shape.  out: the caller's view, which must not
    overlap the planes."""
    _dev(planes, 'planes')
    if planes.dtype != torch.uint16:
        raise TypeError('planes must be torch.uint16, got %s' % planes.dtype)
    single = planes.dim() == 2
    stack = planes[None] if single else planes
    if stack.dim() != 3 or (stack.shape[2] > 1 and stack.stride(2) != 1):
        raise ValueError('planes must be an [h, w] or [n, h, w] view with contiguous rows')
    n, h, w = (int(v) for v in stack.shape)
    if not 1 <= n <= 64:
        raise ValueError('1 to 64 planes, got %d' % n)
    o = np.ascontiguousarray(offset, dtype=np.int64).reshape(-1)
    q = np.ascontiguousarray(weight, dtype=np.int64)
    if o.shape != (w,) or q.shape != (w, 4):
        raise ValueError('offset [%d] and weight [%d, 4], got %s and %s' % (w, w, o.shape, q.shape))
    if w and (np.abs(o).max() > 16384 or q.min() < -4096 or q.max() > 20480 or (q.sum(axis=1) != 16384).any()):
        raise ValueError('|offset| <= 16384, every weight in [-4096, 20480] and a column\'s weights summing to 16384')
    o, q = o.astype(np.int32), np.ascontiguousarray(q.astype(np.int32))
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.uint16, device=planes.device)
    dst = out[None] if out.dim() == 2 else out
    if _dev(out, 'out').dtype != torch.uint16 or tuple(dst.shape) != (n, h, w) or (w > 1 and dst.stride(2) != 1):
        raise ValueError('out must be a uint16 view of the planes\' shape with contiguous rows')
    _lib.check(lib.shg_column_shift_u16(stack.data_ptr(), n, h, w, stack.stride(1), stack.stride(0), _host_ptr(o), _host_ptr(q), dst.data_ptr(),
                                        dst.stride(1), dst.stride(0), _stream()), 'shg_column_shift_u16')
    return out[0] if single and out.dim() == 3 else out


# ---- differential rotation: a finished disk carried to another time ------------------------------------
DEROTATE_MAX_RATE = 0.5           # |k0| + |k1| + |k2| in radians: the range of shg_derotate_u16's sine and cosine polynomials


def derotate_u16(img, circle, matrix, rate3, clv=None, out=None):
    """shg_derotate_u16: every on-disk pixel of the uint16 image taken from where it was the time difference ago -- carried to the
    sphere by circle (cx, cy, r) and the orthonormal matrix [3, 3] (image right / up / observer -> west / pole / central meridian),
    turned back about the pole by a = (k2 s2 + k1) s2 + k0 with s2 = sin^2(latitude) and rate3 = (k0, k1, k2) in radians, sampled
    with a Keys cubic in Q14 both ways -- and, with clv (a float64 [K] device tensor of positive, finite values, K = floor(r) + 1,
    clv[k] at radius k + 1/2 as ring_flatten_u16's gain), times clv(new radius) / clv(old radius).  Pixels off the disk, with a = 0
    or with a source behind the limb stay as they are -> uint16 [h, w].  out: the caller's view, which must not overlap the image."""
    ptr, h, w, pitch = _img(img, 'img', torch.uint16)
    c3, k = _circle3(circle)
    m9 = np.ascontiguousarray(matrix, dtype=np.float64).reshape(-1)
    k3 = np.ascontiguousarray([float(v) for v in rate3], dtype=np.float64)
    if m9.size != 9 or k3.size != 3:
        raise ValueError('matrix is [3, 3] and rate3 is (k0, k1, k2)')
    if not (np.isfinite(k3).all() and np.abs(k3).sum() <= DEROTATE_MAX_RATE):
        raise ValueError('rate3 %r must be finite with |k0| + |k1| + |k2| <= %g radians' % (tuple(k3), DEROTATE_MAX_RATE))
    if clv is not None and (_dev(clv, 'clv').dtype != torch.float64 or tuple(clv.shape) != (k,) or not clv.is_contiguous()):
        raise ValueError('clv must be a contiguous float64 [%d] device tensor (floor(r) + 1 rings)' % k)
    out, optr, opitch = _out_like(out, h, w, torch.uint16, img.device)
    _lib.check(lib.shg_derotate_u16(ptr, h, w, pitch, _host_ptr(c3), _host_ptr(m9), _host_ptr(k3), None if clv is None else clv.data_ptr(), k,
                                    optr, opitch, _stream()), 'shg_derotate_u16')
    return out
