"""shg_line_core_shift and shg_line_profile on seeded adversarial profiles (tests/profile_adversarial.py) in every layout the
kernels branch on: bit for bit against the NumPy restatement (tests/linemaps_ref.py), within the derived bound of the exact
reference (tests/linemaps_exact.py), and line_profile's shift plane equal to line_core_shift's at S = 0.  The finish kernels' display
rounding on exact ties and clips, and the library route (dopplergram(), line_profile_maps()) on 8-bit and un-rotated scans."""
import numpy as np
import pytest

from tests import linemaps_exact as ex
from tests import linemaps_ref as ref
from tests import profile_adversarial as adv
from tests.linemaps_util import IH, IW, N, same_bits, scan_reader, upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import ops
    return ops


LAYOUTS = [  # (name, n, ih, iw, bits, half_width, shift, rotated file, pitched, flip_x, sharded)
    ('rot_u16_vec', 12, 304, 48, 16, 7, 0, True, False, False, False),        # ih % 8 == 0: 16-byte loads
    ('rot_u16_odd', 12, 301, 48, 16, 7, 0, True, False, False, False),        # scalar loads
    ('rot_u8_vec', 12, 304, 48, 8, 7, 0, True, False, False, False),
    ('rot_u8_odd', 12, 301, 48, 8, 7, 0, True, False, False, False),
    ('rot_tail', 17, 513, 40, 16, 5, 0, True, False, False, False),           # last tile one row, last phase one frame
    ('plain_u16', 131, 45, 40, 16, 7, 0, False, False, False, False),          # three blockIdx.x blocks, the last partial
    ('plain_u8', 131, 45, 40, 8, 7, 0, False, False, False, False),
    ('padded_rot', 12, 304, 48, 16, 7, 0, True, True, False, False),
    ('padded_plain', 70, 45, 40, 8, 7, 0, False, True, False, False),
    ('flip_sharded_rot', 12, 304, 48, 8, 7, 0, True, False, True, True),
    ('flip_sharded_plain', 70, 45, 40, 16, 7, 0, False, False, True, True),
    ('h1', 12, 200, 40, 16, 1, 0, True, False, False, False),
    ('h32_rot', 12, 320, 72, 16, 32, 0, True, False, False, False),
    ('h32_plain_u8', 20, 80, 72, 8, 32, 0, False, False, False, False),
    ('s_max', 12, 304, 48, 16, 7, 48 - 4 + 7, True, False, False, False),     # the accepted extremes of S: +-(iw - 4 + H)
    ('s_min', 12, 304, 48, 8, 7, -(48 - 4 + 7), True, False, False, False),
    ('s_max_plain', 70, 45, 40, 16, 5, 40 - 4 + 5, False, False, True, False),
    ('s_min_plain', 70, 45, 40, 8, 5, -(40 - 4 + 5), False, False, False, False),
]


@pytest.mark.parametrize('layout', LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_adversarial_profiles(ops, layout):
    name, n, ih, iw, bits, hw, shift, rot, pitched, flip, sharded = layout
    P, fit, cls = adv.profiles(n, ih, iw, bits, hw, shift, seed=9)
    raw = adv.to_file(P, bits, rot)
    assert raw.shape[1:] == ((iw, ih) if rot else (ih, iw)) and (raw.shape[2] > raw.shape[1]) == rot     # the kernel it picks
    stack = upload(ops, raw, bits, pitched)
    n_cols, k_offset = (n + 9, 4) if sharded else (n, 0)
    cols = k_offset + np.arange(n)
    held = n_cols - 1 - cols if flip else cols                     # frame k's column
    kw = dict(flip_x=flip, n_cols=n_cols, k_offset=k_offset)
    records = {s: ex.records(P, fit, hw, s) for s in sorted({0, shift})}
    counts = adv.occurrences(records[shift], cls, fit, bits, shift)
    print('%s: %s' % (name, ', '.join('%s %d' % kv for kv in sorted(counts.items()))))
    if hw >= 5 and shift == 0:
        missing = [c for c in adv.REQUIRED if not counts.get(c)]
        assert not missing, 'classes never reached: %s' % missing
    if hw == 32:
        assert counts.get('maxsum')

    core = ops.line_core_shift(stack, fit, hw, **kw).cpu().numpy()
    same_bits(core, ref.line_core_shift(raw, fit, hw, **kw))
    worst = {'line_core_shift': ex.within(core[:, held], records[0], *ex.plane('shift'))}
    for s, rec in records.items():
        got = ops.line_profile(stack, fit, hw, s, **kw).cpu().numpy()
        want = ref.line_profile(raw, fit, hw, s, **kw)
        for q, plane in enumerate(ref.PLANES):
            same_bits(got[q], want[q])
            assert np.isfinite(got[q][:, held]).any(), plane
            worst['%s S=%d' % (plane, s)] = ex.within(got[q][:, held], rec, *ex.plane(plane, s))
        if s == 0:
            same_bits(got[0], core)
    print('%s: largest error / bound %s' % (name, ', '.join('%s %.3f' % kv for kv in worst.items())))


# ---- the display planes on exact ties and clips: identity geometry (t = 0), so every map is its raw input ----
F32_MAX = float(np.finfo(np.float32).max)
# (v, display value) for shift and cog at R = 32767 (scale exactly 1.0): e = 32768 + v, rint half to even, clip to [1, 65535]
SHIFT_TIES = [(-32767.5, 1), (-32766.5, 2), (-32765.5, 2), (-32764.5, 4), (0.5, 32768), (1.5, 32770), (-0.5, 32768),
              (32765.5, 65534), (32766.5, 65534), (32767.5, 65535), (-0.0, 32768), (0.0, 32768), (-F32_MAX, 1), (F32_MAX, 65535),
              (-32768.0, 1), (np.nan, 0), (np.inf, 0), (-np.inf, 0)]
# (v, display value) for core: e = v
CORE_TIES = [(0.5, 1), (1.5, 2), (2.5, 2), (3.5, 4), (4.5, 4), (65534.5, 65534), (65535.5, 65535), (65533.5, 65534), (-0.0, 1),
             (-0.5, 1), (-3.0, 1), (1e9, 65535), (np.nan, 0), (np.inf, 0), (-np.inf, 0), (65535.0, 65535), (0.0, 1)]
# (v, display value) for width and ew at H = 3 (scale 65534 / 7 = 9362 exactly): e = 1 + 9362 v
WIDTH_CLIPS = [(0.0, 1), (-0.0, 1), (-1.0, 1), (1.0, 9363), (7.0, 65535), (8.0, 65535), (-F32_MAX, 1), (np.nan, 0), (np.inf, 0)]


def tie_planes():
    m = max(len(SHIFT_TIES), len(CORE_TIES), len(WIDTH_CLIPS))

    def col(pairs):
        return np.array([p[0] for p in pairs] + [0.0] * (m - len(pairs)), dtype=np.float32)

    sv, cv, wv = col(SHIFT_TIES), col(CORE_TIES), col(WIDTH_CLIPS)
    return np.stack([sv, cv, wv, sv[::-1].copy(), wv])[:, None, :].repeat(3, axis=1)      # [5, 3, m]: cog takes shift's reversed


def test_finish_display_ties(ops):
    raw = tie_planes()
    m = raw.shape[2]
    rt = torch.from_numpy(raw).cuda()
    maps, png = ops.line_profile_finish(rt, 1.0, 0.0, 0.0, 3, m, None, None, 3, 32767.0)
    maps, png = maps.cpu().numpy(), png.cpu().numpy()
    want, want_png = ref.line_profile_finish(raw, 1.0, 0.0, 0.0, 3, m, None, None, 3, 32767.0)
    same_bits(maps, want)
    assert np.array_equal(png, want_png)
    # the map is the raw input (inf becomes NaN: t R = 0 x inf), and the hand-written display values
    with np.errstate(invalid='ignore'):
        same_bits(maps, np.where(np.isinf(raw), np.float32(np.nan), raw))
    assert np.array_equal(np.signbit(maps[raw == 0]), np.signbit(raw[raw == 0]))       # -0.0 stays -0.0
    for q, pairs in ((0, SHIFT_TIES), (1, CORE_TIES), (2, WIDTH_CLIPS), (4, WIDTH_CLIPS)):
        expect = np.array([p[1] for p in pairs], dtype=np.uint16)
        for r in range(3):
            assert np.array_equal(png[q, r, :len(pairs)], expect), (ref.PLANES[q], png[q, r, :len(pairs)], expect)
    rev = np.array([p[1] for p in SHIFT_TIES], dtype=np.uint16)[::-1]
    assert np.array_equal(png[3, 0, m - len(SHIFT_TIES):], rev)
    # the Dopplergram's finish on the shift plane: the same display values
    one, dpng = ops.doppler_finish(rt[0], 1.0, 0.0, 0.0, 3, m, None, None, 32767.0)
    same_bits(one.cpu().numpy(), maps[0])
    dwant, dwant_png = ref.doppler_finish(raw[0], 1.0, 0.0, 0.0, 3, m, None, None, 32767.0)
    assert np.array_equal(dpng.cpu().numpy(), dwant_png) and np.array_equal(dwant_png, png[0])
    assert np.array_equal(dpng.cpu().numpy()[:, :len(SHIFT_TIES)], np.tile(np.array([p[1] for p in SHIFT_TIES], dtype=np.uint16), (3, 1)))


# ---- the library route on the file kinds the 16-bit rotated tests do not cover ----
@pytest.mark.parametrize('kind', ['u8_rotated', 'u16_plain'])
def test_library_route_other_file_kinds(ops, kind):
    from solex_ser_recon_en_amd import doppler, lineprofile
    from solex_ser_recon_en_amd.ellipse_to_circle import _warp_geometry
    shift, sigma, depth = ref.injected_fields(IH, N)
    frames, _, _, _ = ref.profile_scan(shift, sigma, depth, IW, noise=0.004, seed=3, rotate=kind == 'u8_rotated')
    if kind == 'u8_rotated':
        frames = (frames >> 8).astype(np.uint8)
    assert (frames.shape[2] > frames.shape[1]) == (kind == 'u8_rotated')
    res = doppler.dopplergram(scan_reader(frames))
    same_bits(res['raw'], ref.line_core_shift(frames, res['fit'], 5))
    assert np.isfinite(res['raw']).mean() > 0.3
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(res['phi'], res['ratio'], IH, N)
    want, want_png = ref.doppler_finish(res['raw'], mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, res['circle'],
                                        res['crop'], 2.0)
    same_bits(res['map'], want)
    assert np.array_equal(res['png'], want_png)
    lp = lineprofile.line_profile_maps(scan_reader(frames))
    raw = np.stack([lp['raw'][p] for p in ref.PLANES])
    for q, plane in enumerate(ref.PLANES):
        same_bits(raw[q], ref.line_profile(frames, lp['fit'], 10)[q])
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(lp['phi'], lp['ratio'], IH, N)
    maps, png = ref.line_profile_finish(raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, lp['circle'], lp['crop'],
                                        10, 2.0)
    for q, plane in enumerate(ref.PLANES):
        same_bits(lp['maps'][plane], maps[q])
        assert np.array_equal(lp['png'][plane], png[q]), plane
