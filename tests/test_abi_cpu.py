"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports exactly
the symbols include/shg_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, 'include', 'shg_hip.h')


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', text)))


def test_library_loads_and_exports_every_declared_symbol():
    from solex_ser_recon_en_amd import _lib
    names = declared_symbols()
    assert len(names) >= 30
    for name in names:
        assert hasattr(_lib.lib, name), 'libshg_hip.so does not export %s' % name
        assert name in _lib.SIGNATURES, 'no ctypes signature for %s' % name
    assert sorted(_lib.SIGNATURES) == names
    assert _lib.lib.shg_abi_version() == _lib.ABI_VERSION == 16
    assert isinstance(_lib.last_error(), str)


def test_workspace_queries_need_no_gpu():
    from solex_ser_recon_en_amd._lib import lib
    assert lib.shg_accumulate_workspace_bytes(2000, 200, 2000, 2) >= 400000 * 6
    assert lib.shg_accumulate_workspace_bytes(0, 200, 2000, 2) == 0
    assert lib.shg_accumulate_workspace_bytes(10, 200, 2000, 3) == 0
    assert lib.shg_clahe_workspace_bytes(2, 2) == 4 * 65536 * 6
    assert lib.shg_clahe_workspace_bytes(3, 1) == 9 * 256 * 6
    assert lib.shg_clahe_workspace_bytes(0, 2) == 0
    # the roomier 16-bit layout: [hist | lut], then one 128 KiB slice histogram per run of whole tile rows holding at most 32768
    # pixels (1000 x 1048 tiles: 31 rows a slice, 33 slices), chunk sums, clipped totals (128 words a tile: one per 512 bins for the
    # saturated slices, 32 x 2 for the u16 ones)
    assert lib.shg_clahe_workspace_bytes_for(2000, 2096, 2, 2) == 4 * 65536 * 6 + 4 * 33 * 131072 + 4 * 1024 * 4 + 4 * 128 * 4
    assert lib.shg_clahe_workspace_bytes_for(77, 50, 4, 1) == lib.shg_clahe_workspace_bytes(4, 1)
    assert lib.shg_contrast_stats_workspace_bytes_for(2000, 2096, 2) == lib.shg_contrast_stats_workspace_bytes(2) + 4 * 33 * 131072 + 4 * 1024 * 4 + 4 * 128 * 4


def _up256(n):
    return (n + 255) // 256 * 256


def _clahe_bytes(tiles, bpp):
    """[hist | lut]: a u32 histogram and a u16 LUT of hist_size entries per tile."""
    if not 1 <= tiles <= 16 or bpp not in (1, 2):
        return 0
    return tiles * tiles * (256 if bpp == 1 else 65536) * (4 + 2)


def _clahe_bytes_for(h, w, tiles, bpp):
    """16-bit: behind [hist | lut] (rounded up to 256 bytes) one 128 KiB slice histogram per run of whole tile rows holding at most
    32768 pixels, 1024 words of chunk sums a tile, 128 words of clipped totals a tile.  The tiles are OpenCV's: a grid that does
    not divide the image extends BOTH axes to the next multiple (a dividing axis by a whole tile count)."""
    base = _clahe_bytes(tiles, bpp)
    if base == 0 or h <= 0 or w <= 0:
        return 0
    if bpp == 1:
        return base
    if h % tiles or w % tiles:
        h, w = h + tiles - h % tiles, w + tiles - w % tiles
    th, tw = h // tiles, w // tiles
    rows = 1 if tw >= 32768 else 32768 // tw
    slices = -(-th // rows)
    return _up256(base) + tiles * tiles * (slices * 131072 + 1024 * 4 + 128 * 4)


def _select_bytes(n_ranks):
    """Eight copies of (1 + n_ranks) 256-bin histograms, then the ranks."""
    return 8 * (1 + n_ranks) * 256 * 4 + n_ranks * 8 if 1 <= n_ranks <= 8 else 0


def _contrast_stats_bytes(clahe_bytes):
    """[clahe | 2-rank select | 3-rank select + window (8 copies of 8 x 256 counts) + its 16-byte state | chunk sums], each
    rounded up to 256 bytes."""
    if clahe_bytes == 0:
        return 0
    select3 = _select_bytes(3) + 8 * 8 * 256 * 4 + 16
    return _up256(clahe_bytes) + _up256(_select_bytes(2)) + _up256(select3) + _up256(1024 * 4)


def test_workspace_queries_follow_the_documented_layout():
    from solex_ser_recon_en_amd._lib import lib
    shapes = [(2000, 2096), (2000, 2097), (201, 304), (64, 2096), (77, 50), (2560, 2675), (17, 17)]
    for tiles in (0, 1, 2, 3, 4, 8, 16, 17):
        for bpp in (1, 2, 3):
            assert lib.shg_clahe_workspace_bytes(tiles, bpp) == _clahe_bytes(tiles, bpp), (tiles, bpp)
            for h, w in shapes + [(0, 17), (17, 0), (-1, 17), (17, -1)]:
                assert lib.shg_clahe_workspace_bytes_for(h, w, tiles, bpp) == _clahe_bytes_for(h, w, tiles, bpp), (h, w, tiles, bpp)
        assert lib.shg_contrast_stats_workspace_bytes(tiles) == _contrast_stats_bytes(_clahe_bytes(tiles, 2)), tiles
        for h, w in shapes + [(0, 17), (17, 0), (-1, 17), (17, -1)]:
            assert lib.shg_contrast_stats_workspace_bytes_for(h, w, tiles) == _contrast_stats_bytes(_clahe_bytes_for(h, w, tiles, 2)), (h, w, tiles)
    for n_ranks in range(0, 10):
        assert lib.shg_select_u16_workspace_bytes(n_ranks) == _select_bytes(n_ranks), n_ranks
    assert lib.shg_select_u16_workspace_bytes(0) == 0 and lib.shg_select_u16_workspace_bytes(9) == 0
    assert lib.shg_clahe_workspace_bytes(0, 2) == 0 and lib.shg_clahe_workspace_bytes(17, 2) == 0 and lib.shg_clahe_workspace_bytes(2, 3) == 0


def test_argument_errors_are_reported_not_thrown():
    """Bad arguments are rejected before any HIP call, so this runs without a GPU."""
    from solex_ser_recon_en_amd import _lib
    lib = _lib.lib
    assert lib.shg_accumulate_sum_max(None, 1, 1, 1, 2, 0, None, None, None, 0, None) == -1
    assert 'null pointer' in _lib.last_error()
    one = ctypes.c_void_p(16)
    assert lib.shg_extract_columns(one, 0, 4, 4, 2, 0, one, one, one, 1, one, 4, 16, 4, 0, 0, None) == -1
    assert lib.shg_frame_pitch_bytes(800000) == 802816 and lib.shg_frame_pitch_bytes(1310720) == 1310720
    assert lib.shg_box_blur_u16(one, 10, 10, 25, 0, one, one, None) == -1      # cv2.blur rejects a zero kernel too
    assert 'must be positive' in _lib.last_error()
    assert lib.shg_rescale_u16(one, 4, 4, 4, 5.0, 5.0, 1.0, one, 4, None) == -1   # assert(sat >= hi > lo)
    with pytest.raises(RuntimeError):
        _lib.check(-1, 'unit test')


def test_warp_route_predicate_truth_table():
    """shg_warp_rows_wide_fits is the launcher's own gate for k_warp_rows8 (csrc/warp.hip): from a layout that fits, each row
    flips one condition."""
    from solex_ser_recon_en_amd._lib import lib
    A = 1 << 20                                                  # any 16-byte aligned address: the pointers are only looked at
    good = dict(src=A, h=60, w=84, src_pitch=128, h00=1.0, h01=0.01, h02=-3.5, dst=A + 4096, out_h=60, out_w=96, dst_pitch=128)

    def fits(**change):
        a = dict(good, **change)
        return lib.shg_warp_rows_wide_fits(a['src'], a['h'], a['w'], a['src_pitch'], a['h00'], a['h01'], a['h02'], a['dst'], a['out_h'],
                                           a['out_w'], a['dst_pitch'])
    assert fits() == 1
    table = [
        (dict(src_pitch=84), 0), (dict(src_pitch=132), 0), (dict(src_pitch=136), 1),                  # pitch % 8
        (dict(dst_pitch=100), 0), (dict(dst_pitch=96), 1),
        (dict(src=A + 2), 0), (dict(src=A + 8), 0), (dict(src=A + 16), 1),                            # pointer & 15
        (dict(dst=A + 4096 + 2), 0), (dict(dst=A + 4096 + 8), 0),
        (dict(w=8, src_pitch=8), 1), (dict(w=7, src_pitch=8), 0), (dict(w=7), 0), (dict(w=8), 1),     # w < 8
        (dict(out_w=9), 1), (dict(out_w=8), 0), (dict(out_w=1), 0), (dict(out_w=16), 1),              # nv < 2
        (dict(h00=-0.1), 0), (dict(h00=0.0), 1), (dict(h00=1.75), 1), (dict(h00=1.76), 0),            # the window's column step
        (dict(h00=float('nan')), 0), (dict(h01=1e300), 0), (dict(h02=-1e300), 0), (dict(h01=float('inf')), 0), (dict(h02=float('nan')), 0),
        (dict(h01=9.9e299), 1),
        (dict(src_pitch=1 << 24, h=64), 0), (dict(src_pitch=(1 << 24) - 8, h=64), 1),                 # pitches in 24 bits
        (dict(src_pitch=1 << 16, w=1 << 16, h=1 << 15), 0), (dict(src_pitch=1 << 16, w=1 << 16, h=(1 << 15) - 1), 1),    # 32-bit offsets
        (dict(dst_pitch=1 << 16, out_h=1 << 15), 0), (dict(dst_pitch=1 << 16, out_h=(1 << 15) - 1), 1),
        (dict(out_h=65536), 0), (dict(h=0), 0), (dict(out_w=0), 0), (dict(src_pitch=80), 0), (dict(dst_pitch=88), 0),   # nothing the launcher takes
    ]
    for change, want in table:
        assert fits(**change) == want, change


def test_scale_rows_route_predicate_truth_table():
    """shg_scale_rows_vec_fits: the launcher's gate for k_scale_rows8 (csrc/transversalium.hip)."""
    from solex_ser_recon_en_amd._lib import lib
    A = 1 << 20
    good = dict(img=A, h=5, w=17, pitch=64, dst=A + 4096, dst_pitch=64)

    def fits(**change):
        a = dict(good, **change)
        return lib.shg_scale_rows_vec_fits(a['img'], a['h'], a['w'], a['pitch'], a['dst'], a['dst_pitch'])
    assert fits() == 1
    table = [
        (dict(pitch=17), 0), (dict(pitch=20), 0), (dict(pitch=24), 1), (dict(dst_pitch=17), 0), (dict(dst_pitch=28), 0), (dict(dst_pitch=24), 1),
        (dict(img=A + 2), 0), (dict(img=A + 8), 0), (dict(img=A + 16), 1), (dict(dst=A + 4098), 0), (dict(dst=A + 4104), 0),
        (dict(w=1, pitch=8, dst_pitch=8), 1), (dict(w=8, pitch=8, dst_pitch=8), 1), (dict(h=1), 1),    # any width, any height: the tail goes pixel by pixel
        (dict(h=0), 0), (dict(w=0), 0), (dict(pitch=16), 0), (dict(h=65536), 0),                      # nothing the launcher takes
    ]
    for change, want in table:
        assert fits(**change) == want, change


def test_products_route_predicate_truth_table():
    """shg_contrast_products_vec_fits: the launcher's gate for k_products8 (csrc/post.hip)."""
    from solex_ser_recon_en_amd._lib import lib
    A = 1 << 20
    good = dict(frame=A, frame_pitch=64, cl1=A + 4096, cl1_pitch=128, h=7, w=17, hc=A + 8192, protus=A + 12288, cc=A + 16384, dst_pitch=192)

    def fits(**change):
        a = dict(good, **change)
        return lib.shg_contrast_products_vec_fits(a['frame'], a['frame_pitch'], a['cl1'], a['cl1_pitch'], a['h'], a['w'], a['hc'], a['protus'],
                                                  a['cc'], a['dst_pitch'])
    assert fits() == 1
    table = [
        (dict(frame_pitch=17), 0), (dict(frame_pitch=60), 0), (dict(cl1_pitch=17), 0), (dict(cl1_pitch=100), 0), (dict(dst_pitch=17), 0),
        (dict(dst_pitch=196), 0), (dict(frame_pitch=24, cl1_pitch=24, dst_pitch=24), 1),                             # pitch % 8
        (dict(frame=A + 2), 0), (dict(cl1=A + 4096 + 8), 0), (dict(hc=A + 8192 + 4), 0), (dict(protus=A + 12288 + 8), 0), (dict(cc=A + 16384 + 2), 0),
        (dict(frame=A + 16), 1),                                                                                     # pointer & 15
        (dict(w=9), 1), (dict(w=8), 0), (dict(w=1), 0), (dict(w=16), 1),                                             # w < 9: two vectors a row
        (dict(dst_pitch=1 << 24), 0), (dict(dst_pitch=(1 << 24) - 8), 1),                                            # pitches in 24 bits
        (dict(frame_pitch=1 << 16, h=1 << 15), 0), (dict(frame_pitch=1 << 16, h=(1 << 15) - 1), 1),                  # 32-bit offsets
        (dict(h=0), 0), (dict(w=0), 0), (dict(frame_pitch=16), 0), (dict(h=65536), 0),                               # nothing the launcher takes
    ]
    for change, want in table:
        assert fits(**change) == want, change


def test_contrast_plan_query_truth_table(monkeypatch):
    """shg_contrast_plan_query is plan_clahe asked as the contrast stage asks it (csrc/clahe.hip): from two aligned 2000 x 2096 disks
    at the default clip limit (12 pixels a bin, the 5th and 6th largest: nibble counters, ranks from the top), each row flips one
    input.  Fields: batched, disks, route (2 u16 / 3 bytes / 4 nibbles / 1 atomics), bits, clip, ..., from_top [10], blend pixels [11],
    LUT for all tiles [13], window [14], fused [15]."""
    from solex_ser_recon_en_amd import _lib
    for name in ('SHG_CLAHE_SAT', 'SHG_CLAHE_SAT_PX', 'SHG_SELECT_WINDOW', 'SHG_CONTRAST_BATCH', 'SHG_INTERP_SHAPE', 'SHG_FUSE_SCALE'):
        monkeypatch.delenv(name, raising=False)
    good = dict(k=2, h=2000, w=2096, pitch=2112, dst_pitch=2112, bits=0, clip_limit=0.8, tiles=2, fused=1, ranks=1, window=-1)

    def plan(**change):
        a = dict(good, **change)
        out = (ctypes.c_int64 * 16)()
        err = _lib.lib.shg_contrast_plan_query(a['k'], a['h'], a['w'], a['pitch'], a['dst_pitch'], a['bits'], a['clip_limit'], a['tiles'], a['fused'],
                                               a['ranks'], a['window'], out)
        return err, list(out)
    err, p = plan()
    assert err == 0 and p[:5] == [1, 2, 4, 4, 12] and p[8:11] == [6, 5, 1] and p[11:] == [4, 1, 0, 0, 1]
    assert p[6] == -(-1000 // p[5]) and p[7] == 65280 // 1048
    table = [
        (dict(k=1), {0: 1, 1: 1, 15: 1}), (dict(k=1, fused=0), {0: 0, 1: 1, 2: 2, 3: 16, 10: 0, 15: 0}),       # one disk: batched only to be made on the way
        (dict(k=4), {1: 4, 11: 8, 14: 1}), (dict(k=8), {13: 1}), (dict(k=40), {1: 32}),
        (dict(clip_limit=0.0), {0: 0, 2: 1, 3: 0, 4: 0}), (dict(clip_limit=1.01), {2: 3, 3: 8, 4: 16}), (dict(clip_limit=15.98), {2: 3, 4: 255}),
        (dict(clip_limit=16.02), {2: 2, 3: 16, 4: 256, 10: 0}), (dict(clip_limit=0.3), {2: 2, 4: 4, 10: 0}),     # the 6th largest is out of reach of clip 4
        (dict(ranks=0), {2: 2, 3: 16, 8: 0, 9: 0, 10: 0}), (dict(window=1), {14: 1}), (dict(k=4, window=0), {14: 0}),
        (dict(fused=0), {0: 1, 15: 0}), (dict(bits=8, k=4), {11: 4}), (dict(bits=2), {11: 1, 14: 0}), (dict(pitch=2100, dst_pitch=2100, k=4), {11: 4}),
        (dict(tiles=4, k=8), {13: 1}), (dict(tiles=5, k=8), {13: 0}),
    ]
    for change, want in table:
        err, p = plan(**change)
        assert err == 0 and {i: p[i] for i in want} == want, (change, p)
    monkeypatch.setenv('SHG_CLAHE_SAT', '8')
    assert plan()[1][2:4] == [3, 8]
    monkeypatch.setenv('SHG_CLAHE_SAT', '0')
    assert plan()[1][2:4] == [2, 16]
    monkeypatch.setenv('SHG_CONTRAST_BATCH', '0')
    assert plan()[1][:2] == [0, 1]
    assert plan(tiles=17)[0] != 0 and 'tiles' in _lib.last_error()
    assert plan(h=0)[0] == -1 and _lib.lib.shg_contrast_plan_query(2, 10, 10, 16, 16, 0, 0.8, 2, 1, 1, -1, None) == -1


def test_ops_refuse_cpu_tensors():
    import torch
    from solex_ser_recon_en_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.accumulate_sum_max(torch.zeros((2, 4, 4), dtype=torch.uint8))


def test_header_compiles_as_plain_c(tmp_path):
    """include/shg_hip.h is the drop-in boundary: it must be valid C99 (no C++, no torch types)."""
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    src = os.path.join(os.path.dirname(__file__), 'c_abi', 'header_is_c.c')
    inc = os.path.join(os.path.dirname(os.path.dirname(__file__)), 'include')
    r = subprocess.run([gcc, '-std=c99', '-Wall', '-Werror', '-pedantic', '-I', inc, '-c', src, '-o', str(tmp_path / 'h.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_c_caller_builds_against_the_library(tmp_path):
    """tests/c_abi/abi_smoke.cpp (a torch-free, Python-free caller) compiles and links against libshg_hip.so here;
    it RUNS in the gpu test of the same name."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    root = os.path.dirname(os.path.dirname(__file__))
    lib_dir = os.path.join(root, 'solex_ser_recon_en_amd', 'csrc')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-I', os.path.join(root, 'include'),
                        os.path.join(root, 'tests', 'c_abi', 'abi_smoke.cpp'), '-L', lib_dir, '-lshg_hip',
                        '-Wl,-rpath,' + lib_dir, '-o', str(tmp_path / 'abi_smoke')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
