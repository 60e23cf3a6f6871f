"""Helpers shared by the line maps' tests (the Dopplergram, the line-profile and the line-bisector maps, and their overlay on the
products): bit-for-bit comparison, hand-built and synthetic scans and fits, the kernels' layout cases, stack upload, the finish
geometries, the single-JSON-line CLI runner and the marked scan."""
import json

import numpy as np

from tests import linemaps_ref as ref

IH, N, IW = 400, 300, 48                    # the synthetic disk scans: slit rows, frames, spectral samples


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN positions differ (%d vs %d)' % (np.isnan(got).sum(), np.isnan(want).sum())
    g, w = got.view(np.uint32).copy(), want.view(np.uint32).copy()
    g[np.isnan(got)] = w[np.isnan(want)] = 0          # (NaN payloads are not part of the contract)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, '%d values differ, first at %s: %r vs %r' % (bad.size, np.unravel_index(bad[0], got.shape),
                                                                      got.flat[bad[0]], want.flat[bad[0]])


# ---- hand-built scans (CPU) ----
def one_row_scan(profiles_yk, rotate=True):
    """frames [n, H, W] (file layout) whose slit row y of frame k is profiles_yk[y, k] (uint16 [rows, n, iw]).  The slit axis is the
    longer one (a1 rotates when W > H): rows beyond those given repeat the last one, up to iw + 1."""
    rows, n, iw = profiles_yk.shape
    ih = max(rows, iw + 1)
    prof = np.concatenate([profiles_yk, np.repeat(profiles_yk[-1:], ih - rows, axis=0)])
    img = np.transpose(prof, (1, 0, 2))                         # [n, ih, iw]
    if rotate:
        return np.ascontiguousarray(np.rot90(img, -1, axes=(1, 2)))   # img[y, x] = raw[x, W - 1 - y]
    return np.ascontiguousarray(img)


def fit_at(centre, ih=None):
    """fit [ih, 4] of a line at centre[y] (the last value repeated up to ih rows)."""
    centre = np.asarray(centre, dtype=np.float64)
    if ih is not None and ih > centre.shape[0]:
        centre = np.concatenate([centre, np.repeat(centre[-1:], ih - centre.shape[0])])
    return np.stack([np.floor(centre), centre - np.floor(centre), np.arange(centre.shape[0], dtype=np.float64), centre], axis=1)


def parabola(iw, quad, lin, const):
    j = np.arange(iw, dtype=np.int64)
    return (quad * j * j + lin * j + const).astype(np.uint16)


def fit_for(synth, ih, iw, seed, jitter=3.0, edges=True, nans=True):
    """A fit [ih, 4] around synth's line: per-row jitter (minima land on window edges too), rows whose line is within H of both
    frame edges, and non-finite rows."""
    rng = np.random.default_rng(seed)
    centre = synth.curve_of_row(np.arange(ih, dtype=np.float64), ih, iw) + rng.uniform(-jitter, jitter, ih)
    if edges:
        centre[0:ih:11] = rng.uniform(-1.5, 4.0, centre[0:ih:11].shape)
        centre[5:ih:13] = rng.uniform(iw - 5.0, iw + 1.5, centre[5:ih:13].shape)
    fit = np.stack([np.floor(centre), centre - np.floor(centre), np.arange(ih, dtype=np.float64), centre], axis=1)
    if nans:
        fit[3, 0], fit[7, 0], fit[9, 3] = np.nan, np.inf, np.nan
    return fit


# ---- the kernels' layouts (GPU) ----
CASES = [  # (name, n, width, height, bits, half_width, flip_x, sharded, pitched)
    ('rot_u16', 37, 300, 40, 16, 5, False, False, False),
    ('rot_u8', 37, 304, 40, 8, 5, False, False, False),
    ('plain_u16', 37, 40, 300, 16, 5, False, False, False),
    ('plain_u8', 37, 40, 300, 8, 5, False, False, False),
    ('flip', 37, 304, 40, 16, 5, True, False, False),
    ('sharded', 37, 304, 40, 16, 5, False, True, False),
    ('sharded_flip', 37, 304, 40, 8, 5, True, True, False),
    ('h1', 20, 304, 40, 16, 1, False, False, False),
    ('h32', 20, 600, 80, 16, 32, False, False, False),
    ('h32_plain', 20, 80, 600, 16, 32, True, False, False),
    ('n1', 1, 304, 40, 16, 5, False, False, False),
    ('odd_ih', 37, 301, 40, 16, 5, False, False, False),
    ('odd_ih_u8', 37, 517, 40, 8, 7, True, False, False),
    ('pitched', 37, 304, 40, 16, 5, False, False, True),
    ('pitched_u8_odd', 37, 301, 41, 8, 5, False, False, True),
]
# CASES at S = 0, plus shifts whose windows clip at either edge of the frame
SHIFT_CASES = [c + (0,) for c in CASES] + [
    ('s_minus', 37, 304, 40, 16, 5, False, False, False, -14),
    ('s_plus', 37, 304, 40, 16, 5, True, False, False, 15),
    ('s_plus_u8_plain', 37, 40, 300, 8, 7, False, False, False, 13),
    ('s_minus_h32', 20, 600, 80, 16, 32, False, True, True, -30),
]


def upload(ops, frames, bits, pitched=False):
    """frames (uint8 / uint16, file layout) on the GPU as a plain or a pitched stack."""
    import torch
    dtype = torch.uint8 if bits == 8 else torch.uint16
    host = torch.from_numpy(frames.view(np.int16) if bits == 16 else frames)
    if pitched:
        stack = ops.padded_stack(*frames.shape, dtype, 'cuda')
        stack.copy_(host.view(dtype).cuda())
        assert stack.stride(0) > frames.shape[1] * frames.shape[2]
        return stack
    return host.cuda().view(dtype)


def scan_reader(frames):
    from solex_ser_recon_en_amd.video_reader import array_reader
    return array_reader(upload(None, frames, 8 if frames.dtype == np.uint8 else 16))


def finish_cases():
    from solex_ser_recon_en_amd import SHG_MAIN
    base = SHG_MAIN.default_options()
    return [('none', None, dict(base)), ('square', None, dict(base, crop_width_square=True)),
            ('wide', None, dict(base, fixed_width=700)), ('narrow', None, dict(base, fixed_width=120)),
            ('circle', (250.3, 199.6, 150.2), dict(base)), ('circle_square', (250.3, 199.6, 150.2), dict(base, crop_width_square=True)),
            ('circle_wide', (250.3, 199.6, 150.2), dict(base, fixed_width=701)), ('circle_narrow', (250.3, 199.6, 150.2), dict(base, fixed_width=121)),
            ('no_circle', (-1, -1, -1), dict(base, fixed_width=300))]


# ---- the command lines ----
def write_scan(tmp_path_factory, name, frames):
    """frames written as <tmp>/<name>/scan.ser: its path."""
    from solex_ser_recon_en_amd import synth
    path = tmp_path_factory.mktemp(name) / 'scan.ser'
    synth.write_ser(str(path), frames)
    return str(path)


def run_json(main, capsys, argv):
    """main(argv) succeeds and prints one line of JSON: that, parsed."""
    capsys.readouterr()
    assert main(argv) == 0
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1, out
    return json.loads(out[0])


# ---- the marked scan: the maps overlay the products ----
K0, K1, Y0, Y1 = 70, 100, 120, 200          # the marker: frames [K0, K1) x slit rows [Y0, Y1), off-centre both ways
SHIFT, GAIN = 2.0, 1.25


def marked_scan():
    """doppler_scan's scene without noise, the marker's continuum GAIN times brighter and its line SHIFT px to the red."""
    mark = (np.arange(IH) >= Y0)[:, None] & (np.arange(IH) < Y1)[:, None] & (np.arange(N) >= K0) & (np.arange(N) < K1)
    return ref.disk_scan(ref.gaussian(np.where(mark, SHIFT, 0.0)), IH, N, IW, noise=0.0, gain=np.where(mark, GAIN, 1.0))[0]


def grow(m):
    """m dilated by one pixel (3 x 3)."""
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def same_region(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.sum() > 200 and b.sum() > 200, (what, int(a.sum()), int(b.sum()))
    assert not (a & ~grow(b)).any() and not (b & ~grow(a)).any(), '%s: the marker lies on other pixels (%d vs %d px, %d apart)' % (
        what, int(a.sum()), int(b.sum()), int((a & ~grow(b)).sum() + (b & ~grow(a)).sum()))
