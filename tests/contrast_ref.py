"""The contrast stage of one disk (shg_stage_process_frames: row factors, crop / pad, CLAHE, the three order statistics, the three
rescales, the disc) composed from the oracle's own functions.  NumPy only; nothing comes from the package under test."""
import numpy as np

from oracle import shg_oracle as orc

PRODUCTS = ('final', 'cl1', 'hc', 'protus', 'cc')


def detrans_of(frame, factors):
    """The last lines of orc.correct_transversalium2 for given row factors c (float64 [h])."""
    ret = (frame.T * np.asarray(factors, dtype=np.float64)).T
    ret[ret > 65535] = 65535
    return np.array(ret, dtype='uint16')


def crop_pad(img, crop):
    """orc.crop_center's block in the (crop_w, sx0, dx0, ncopy) form process_frames takes: dst[:, dx0:dx0 + ncopy] =
    src[:, sx0:sx0 + ncopy], img[0, 0] elsewhere."""
    crop_w, sx0, dx0, ncopy = crop
    out = np.full((img.shape[0], crop_w), img[0, 0], dtype=img.dtype)
    out[:, dx0:dx0 + ncopy] = img[:, sx0:sx0 + ncopy]
    return out


def crop_plan(w, cx, fixed_width):
    """(crop_w, sx0, dx0, ncopy) of orc.crop_center(img [h][w], (cx, ., .), fixed_width, False), line by line."""
    nw2 = fixed_width // 2
    tx = nw2 - int(cx)
    lo, hi = max(0, int(cx) - nw2), min(int(cx) + nw2, w)
    if tx > 0:
        return fixed_width, lo, tx, min(hi - lo, fixed_width - tx)       # rolled right by tx: what passes the right edge is overwritten
    return fixed_width, lo, 0, hi - lo


def stage_reference(frame_u16, factors=None, crop=None, disc=None, clip_limit=0.8, tiles=2):
    """-> dict(detrans, final, cl1, hc, protus, cc), or raises AssertionError where rescale_brightness does."""
    frame = np.asarray(frame_u16)
    assert frame.dtype == np.uint16 and frame.ndim == 2
    detrans = detrans_of(frame, factors) if factors is not None else frame.copy()
    final = crop_pad(detrans, crop) if crop is not None and crop[0] > 0 else detrans
    cl1 = orc.clahe(final, clip_limit, tiles)
    bright = np.percentile(final, 99.9999)
    dark_clahe = np.percentile(cl1, 10)
    bright_clahe = np.max(cl1)
    hc = orc.rescale_brightness(final, bright * 0.25, bright)
    protus = orc.rescale_brightness(final, 0, bright * 0.18)
    cc = orc.rescale_brightness(cl1, dark_clahe, bright_clahe)
    if disc is not None and disc[2] > 0:
        protus = orc.filled_circle(protus, int(disc[0]), int(disc[1]), int(disc[2]), 80)
    return dict(detrans=detrans, final=final, cl1=cl1, hc=hc, protus=protus, cc=cc)


def raises(frame_u16, **kw):
    try:
        stage_reference(frame_u16, **kw)
    except AssertionError:
        return True
    return False
