"""Pitched uint16 device images for the kernel tests: the layout production hands every per-disk kernel (ops.pitched_u16, the
disk and frame arenas: row pitch a multiple of 64 pixels, rows 16-byte aligned), with a known value in every element that is
not the image's -- so that a kernel that reads its padding shows it in its result and one that writes it is caught afterwards.
A dense tensor (pitch = width) sends every width that is not a multiple of 8 to the one-pixel-a-lane kernels."""
import numpy as np

POISON = 23131           # source padding: inside the value range of the test images (a leaked sample survives every clip)
DST_POISON = 43981       # destination stores before the kernel writes them


def pitch_for(w, col0=0, align=64):
    return (col0 + w + align - 1) // align * align


def pitched(np_img, pitch=None, poison=POISON, col0=0):
    """-> (store, view): store is a uint16 device tensor [h, pitch] (pitch: the next multiple of 64 at or above col0 + w unless
    given), view = store[:, col0:col0 + w] holds np_img and every other element holds `poison`.  col0 = 0: rows 16-byte aligned
    (torch's allocations are); col0 = 1: rows 2 bytes off, whatever the pitch."""
    import torch
    np_img = np.asarray(np_img)
    assert np_img.dtype == np.uint16 and np_img.ndim == 2
    h, w = np_img.shape
    pitch = pitch_for(w, col0) if pitch is None else int(pitch)
    assert pitch >= col0 + w
    full = np.full((h, pitch), poison, np.uint16)
    full[:, col0:col0 + w] = np_img
    store = torch.from_numpy(full).cuda()
    assert store.data_ptr() % 16 == 0
    return store, store[:, col0:col0 + w]


def pitched_blank(h, w, pitch=None, poison=DST_POISON, col0=0):
    """A destination: every element of the store, the view's included, holds `poison`."""
    return pitched(np.full((h, w), poison, np.uint16), pitch, poison, col0)


def view_to_host(view):
    return np.ascontiguousarray(view.cpu().numpy())


def padding_untouched(store, view, poison):
    """Whether every element of `store` outside `view` still holds `poison`."""
    full = store.cpu().numpy().copy()
    col0 = view.storage_offset() - store.storage_offset()
    assert 0 <= col0 and col0 + view.shape[1] <= store.shape[1] and view.shape[0] == store.shape[0] and view.stride(0) == store.stride(0)
    full[:, col0:col0 + view.shape[1]] = poison
    return bool((full == poison).all())
