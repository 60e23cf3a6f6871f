"""Exact restatement of the limb stage's statistics -- get_flood_image's front half, ellipse_to_circle.py:159-169, 241, 299-301 --
written from include/shg_hip.h's description of shg_limb_prepare and from the reference's NumPy calls, not from the kernels, and
the seeded adversarial inputs that hold both chains of the stage (csrc/limb_fused.hip, csrc/limb.hip) to it.

Why it is exact.  The 4x4 block mean of uint16 / 65536 is B * 2^-20 with B the block's integer sum (zero-padded blocks
included), so every k x k window sum of cv2.blur (BORDER_REFLECT_101, anchor k // 2) is an integer W below 2^53 and the blurred
value is (W * 2^-20) * (1 / (k * k)) with one rounding.  Order statistics are a sort, the histogram is np.histogram itself.
Nothing here has a tolerance.

prepare(img_u16, k) returns the numbers and a Counter of the decision classes the input reached; cases(seed) the inputs;
REQUIRED the classes the whole set must reach (tests/test_limb_stats_cpu.py checks that on the CPU, so that the GPU test cannot
pass on easy inputs)."""
from collections import Counter

import numpy as np

from solex_ser_recon_en_amd import hostmath, order_stats

UNIT = 2.0 ** -20
BLOCK_MAX = 16 * 65535                # the largest block sum
HIST_BINS = 20
TILE = 16                             # the blur kernel's output tile, FLOOD_SLOTS slots shared by its workgroups
FLOOD_SLOTS = 9
SELECT_CHUNK = 2048                   # elements per workgroup of the selects, 256 workgroups at most
SELECT_MAX_GROUPS = 256


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------
def block_sums(img_u16):
    """int64 [ceil(h/4), ceil(w/4)]: the 4x4 block sums, blocks beyond the image padded with zeros (block_reduce, cval 0)."""
    img = np.asarray(img_u16)
    assert img.dtype == np.uint16 and img.ndim == 2
    h, w = img.shape
    padded = np.zeros((-(-h // 4) * 4, -(-w // 4) * 4), np.int64)
    padded[:h, :w] = img
    return padded.reshape(padded.shape[0] // 4, 4, padded.shape[1] // 4, 4).sum(axis=(1, 3))


def reflect101(i, n):
    """BORDER_REFLECT_101 (d c b | a b c d | c b a), folded as often as needed."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def window_sums(B, k):
    """int64 [sh, sw]: the k x k window sums of B, anchor k // 2 (cv2.blur's default), BORDER_REFLECT_101."""
    sh, sw = B.shape
    taps = np.arange(k) - k // 2
    rx = reflect101(np.arange(sw)[:, None] + taps[None, :], sw)           # [sw, k]
    ry = reflect101(np.arange(sh)[:, None] + taps[None, :], sh)           # [sh, k]
    rows = np.zeros((sh, sw), np.int64)
    for j in range(k):
        rows += B[:, rx[:, j]]
    out = np.zeros((sh, sw), np.int64)
    for j in range(k):
        out += rows[ry[:, j], :]
    return out


def blurred_plane(W, k):
    return (W.astype(np.float64) * UNIT) * (1.0 / (float(k) * float(k)))


def stage_ranks(n):
    """([lo, hi of np.median, lo, hi of np.percentile(., 99)], gamma of the percentile)."""
    m_lo, m_hi, _ = order_stats.median_order_stats(n)
    p_lo, p_hi, _ = order_stats.lerp_order_stats(n, 99)
    return [m_lo, m_hi, p_lo, p_hi], order_stats.lerp_gamma(n, 99)


def radix_digits(k):
    """(high, low) digit widths of the fused path's two-pass select: a window sum of blur max(k, 5) is below 2^(high + low)."""
    kk = max(int(k), 5)
    total = int(kk * kk * BLOCK_MAX).bit_length()
    return total - total // 2, total // 2


def prepare(img_u16, k):
    """The stage's statistics for the disk img_u16 and the blur window k.  -> dict:
    B, Wk, W5 int64 [sh, sw]; blur_k, blur_5 float64; ranks [4], order_stats float64 [4] = [median pair of blur 5, 99th-percentile
    pair of blur k]; gamma, very_bright, median5; total = np.sum(block mean); data, mn, mx (None when data is empty), counts int64
    [20]; threshold (hostmath.flood_threshold, None when data is empty: the reference raises there); classes (Counter)."""
    k = int(k)
    assert k >= 1
    img = np.asarray(img_u16)
    h, w = img.shape
    B = block_sums(img)
    sh, sw = B.shape
    n = sh * sw
    Wk = window_sums(B, k)
    W5 = Wk if k == 5 else window_sums(B, 5)
    blur_k, blur_5 = blurred_plane(Wk, k), blurred_plane(W5, 5)
    ranks, gamma = stage_ranks(n)
    s5, sk = np.sort(blur_5, axis=None), np.sort(blur_k, axis=None)
    stats = np.array([s5[ranks[0]], s5[ranks[1]], sk[ranks[2]], sk[ranks[3]]])
    very_bright = order_stats.lerp_order_stats(n, 99)[2](stats[2], stats[3])
    median5 = order_stats.median_order_stats(n)[2](stats[0], stats[1])
    total = float(B.sum()) * UNIT                                 # every partial sum of np.sum is a whole number of 2^-20: exact
    flat = blur_k.ravel()
    data = flat[flat < very_bright]
    cls = Counter()
    if data.size:
        mn, mx = float(data.min()), float(data.max())
        counts, edges = np.histogram(data, HIST_BINS)
        counts = counts.astype(np.int64)
        threshold = hostmath.flood_threshold(total, (sh, sw), mn, mx, counts)
        distinct = np.unique(data)
        cls['data_one_value' if distinct.size == 1 else 'data_many'] += 1
        hit = [j for j in range(1, HIST_BINS) if np.any(distinct == edges[j])]
        if distinct.size > 1:
            cls['on_interior_edge'] += int(sum(np.count_nonzero(data == edges[j]) for j in hit))
            cls['on_interior_edge_distinct'] = len(hit)
            cls['on_last_edge'] += int(np.count_nonzero(data == edges[HIST_BINS]))
    else:
        mn = mx = threshold = None
        counts = np.zeros(HIST_BINS, np.int64)
        cls['data_empty'] += 1
    # ---- what the input reached
    a, b = stats[2], stats[3]
    if a == b:
        cls['p99_pair_tied'] += 1
        if data.size:
            cls['p99_tied_with_values_below'] += 1                # the fused path scans the image for the flood's max
    else:
        cls['p99_pair_apart_gamma_zero' if gamma == 0.0 else 'p99_pair_apart_gamma_pos'] += 1
    if n % 2:
        cls['median_n_odd'] += 1
    else:
        cls['median_n_even_tied' if stats[0] == stats[1] else 'median_n_even_apart'] += 1
    if h % 4:
        cls['padded_blocks_rows'] += 1
    if w % 4:
        cls['padded_blocks_cols'] += 1
    before, after = k // 2, k - 1 - k // 2
    if max(before, after) > min(sh, sw) - 1:
        cls['reflect_more_than_once'] += 1
    elif before > 0 or after > 0:
        cls['reflect_once'] += 1
    high, low = radix_digits(k)
    for W, kw, lo_hi in ((W5, 5, ranks[0:2]), (Wk, k, ranks[2:4])):
        srt = np.sort(W, axis=None)
        present = np.unique(srt)
        for r in lo_hi:
            s = int(srt[r])
            for unit, name in ((1 << low, 'pair_straddles_high_digit'), (1 << (low + high - 8), 'pair_straddles_high_chunk'),
                               (1 << (low - 8), 'pair_straddles_low_chunk')):
                above = s % unit == 0 and s > 0 and (s - 1) in present
                below = (s + 1) % unit == 0 and (s + 1) in present
                if above or below:
                    cls[name] += 1
    distinct_k = np.unique(Wk)
    if distinct_k.size > 1:
        if np.unique(distinct_k >> low).size == 1:
            cls['sums_share_high_digit'] += 1
        if np.unique(distinct_k & ((1 << low) - 1)).size == 1:
            cls['sums_share_low_digit'] += 1
    if int(Wk.max()) == k * k * BLOCK_MAX:
        cls['largest_window_sum'] += 1
    if k == 5:
        cls['k5_one_array'] += 1
    tiles = -(-sh // TILE) * -(-sw // TILE)
    if tiles > 1:
        cls['several_tiles'] += 1
    if tiles > FLOOD_SLOTS:
        cls['flood_slots_wrap'] += 1
    if n == SELECT_CHUNK:
        cls['select_one_full_group'] += 1
    if n > SELECT_CHUNK:
        cls['select_several_groups'] += 1
    if n > SELECT_CHUNK * SELECT_MAX_GROUPS:
        cls['select_grid_capped'] += 1
    return dict(B=B, Wk=Wk, W5=W5, blur_k=blur_k, blur_5=blur_5, ranks=ranks, order_stats=stats, gamma=gamma, very_bright=very_bright,
                median5=median5, total=total, data=data, mn=mn, mx=mx, counts=counts, threshold=threshold, classes=cls)


# ---- the layouts: how the disk lies in its store (tests/pitched_util.pitched's pitch and col0) ---------------------------------------
def layout_args(layout, w):
    """-> (pitch or None, col0) for pitched_util.pitched.  'vec': rows a multiple of 64 pixels apart on a 16-byte aligned base: the
    8-byte loads of k_limb_blur and k_downscale_mean; 'odd': an odd pitch; 'off1': the view one column into its store."""
    if layout == 'vec':
        return None, 0
    if layout == 'odd':
        return (w + 7) | 1, 0
    assert layout == 'off1'
    return None, 1


def layout_classes(case):
    h, w = case['disk'].shape
    cls = Counter()
    if case['layout'] == 'vec':
        cls['vec_route'] += 1
        if h % 4 and w % 4:
            cls['vec_route_partial_blocks'] += 1
    else:
        cls['scalar_route'] += 1
        cls['scalar_route_' + case['layout']] += 1
    return cls


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def disk_from_block_sums(B, rng=None):
    """A uint16 disk [4 sh, 4 sw] whose 4x4 block sums are B (0 ... 16 * 65535): s // 16 everywhere, s % 16 pixels one more (at
    seeded places with rng, the first ones without)."""
    B = np.asarray(B, np.int64)
    assert B.min() >= 0 and B.max() <= BLOCK_MAX
    sh, sw = B.shape
    q, r = B // 16, B % 16
    order = np.arange(16)[None, None, :].repeat(sh, 0).repeat(sw, 1)
    if rng is not None:
        order = rng.permuted(order, axis=2)
    px = q[:, :, None] + (order < r[:, :, None])
    return px.reshape(sh, sw, 4, 4).transpose(0, 2, 1, 3).reshape(sh * 4, sw * 4).astype(np.uint16)


def _placed(rng, sh, sw, sorted_values):
    """Block sums [sh, sw] holding `sorted_values` (one per block) at seeded places."""
    v = np.asarray(sorted_values, np.int64)
    assert v.size == sh * sw
    return rng.permutation(v).reshape(sh, sw)


def cases(seed=0):
    """The adversarial cases: dicts of name, disk (uint16 [h, w]), k, layout ('vec' / 'odd' / 'off1'), fence (whether the GPU test
    also runs the case under SHG_LIMB_FENCE=1) and big (the one large case)."""
    rng = np.random.default_rng([seed, 159])
    out = []

    def add(name, disk, k, layout, fence=False, big=False):
        out.append(dict(name=name, disk=np.ascontiguousarray(disk, dtype=np.uint16), k=k, layout=layout, fence=fence, big=big))

    def noise(h, w):
        return rng.integers(0, 65536, (h, w)).astype(np.uint16)

    # ---- shapes and windows, random full-range values.  Quarter size in the name; h % 4 and w % 4 cover 1, 2, 3
    add('3x3_k16', noise(9, 10), 16, 'vec', fence=True)                      # every halo folds more than once
    add('3x3_k1', noise(12, 9), 1, 'odd')
    add('3x3_k15', noise(11, 11), 15, 'off1')                               # (k = 16 on 3 x 3 covers four whole periods: every window alike)
    add('3x4_k6', noise(11, 13), 6, 'off1')
    add('15x17_k2', noise(57, 67), 2, 'vec')
    add('16x16_k3', noise(62, 64), 3, 'odd')
    add('17x15_k4', noise(68, 58), 4, 'off1')
    add('32x33_k6', noise(127, 129), 6, 'vec', fence=True)
    add('33x32_k15', noise(129, 128), 15, 'odd')
    add('17x33_k16', noise(66, 131), 16, 'vec')
    add('64x64_k5', noise(253, 255), 5, 'vec', fence=True)                    # 16 tiles on 9 slots, two workgroups in the select
    add('32x64_k1', noise(128, 256), 1, 'off1')                             # n = 2048
    add('3x683_k16', noise(10, 2731), 16, 'odd')                            # n = 2049, rows fold more than once
    add('13x77_k2', noise(50, 305), 2, 'vec')                               # (n - 1) % 100 == 0: gamma == 0, very_bright = the lower statistic
    add('7x43_k5', noise(28, 171), 5, 'off1')                               # the same with one array
    # ---- constants: data is empty
    add('zeros_k1', np.zeros((80, 84), np.uint16), 1, 'vec')
    add('max_k16', np.full((80, 72), 65535, np.uint16), 16, 'odd', fence=True)      # the largest window sums there are
    add('const_k3', np.full((76, 84), 12345, np.uint16), 3, 'off1')
    # ---- few grey levels in bands, the lowest wide enough to hold the median of blur 5: both pairs of order statistics tie
    two = np.where(np.arange(20)[None, :] < 13, 700 * 16, 52000 * 16) + np.zeros((20, 1), np.int64)
    add('two_levels_k1', disk_from_block_sums(two), 1, 'vec')
    four = np.repeat([300, 9000, 9001, 60000], [15, 3, 3, 3])[None, :] * 16 + np.zeros((18, 1), np.int64)
    add('four_levels_k2', disk_from_block_sums(four), 2, 'odd', fence=True)
    # ---- a flat top: the 99th-percentile pair ties with values below it (the fused path looks the image over)
    flat = np.minimum(rng.integers(0, BLOCK_MAX + 1, (21, 23)), int(0.93 * BLOCK_MAX))
    add('flat_top_k1', disk_from_block_sums(flat, rng), 1, 'off1', fence=True)
    plateau = rng.integers(0, 40000 * 16, (30, 34))
    plateau[4:20, 5:25] = 61000 * 16
    add('flat_top_k3', disk_from_block_sums(plateau, rng)[:118, :135], 3, 'vec')
    # ---- one bright pixel on black; all equal but one block (n <= 100: the 99th-percentile pair is the last two)
    one = np.zeros((80, 80), np.uint16)
    one[37, 42] = 65535
    add('one_pixel_k2', one, 2, 'vec')
    but_one = np.full((9, 11), 16 * 1000, np.int64)
    but_one[4, 7] = 16 * 1000 + 5
    add('all_but_one_k1', disk_from_block_sums(but_one), 1, 'odd')
    lower = np.full((20, 20), 16 * 1000, np.int64)
    lower[11, 3] = 16 * 1000 - 7
    add('one_lower_k1', disk_from_block_sums(lower), 1, 'off1')
    # ---- k = 1, 22 levels in arithmetic progression, the top one on more than 1 % of the blocks: very_bright is the top level, data
    # the 21 below, and np.linspace(min, max, 21) runs through every one of them
    levels = 1000 + 4096 * np.arange(22)
    ap = levels[rng.integers(0, 22, (24, 25))]
    ap.ravel()[rng.choice(ap.size, 40, replace=False)] = levels[21]
    ap.ravel()[:22] = levels
    add('edges_k1', disk_from_block_sums(ap, rng), 1, 'vec', fence=True)
    # ---- radix digits (k <= 5: 13 + 12 bits)
    add('low_digit_k1', disk_from_block_sums(5 * 4096 + rng.integers(0, 4096, (19, 21)), rng), 1, 'odd')
    add('high_digit_k1', disk_from_block_sums(4096 * rng.integers(0, 256, (19, 21)) + 77, rng), 1, 'vec')
    # the 99th-percentile pair (ranks 395, 396 of 400) on the two sides of a digit boundary that is a coarse-chunk boundary of both passes
    edge = 4096 * 192
    srt = np.concatenate([np.full(150, 4096 * 3 - 1), np.full(150, 4096 * 3), np.sort(rng.integers(4096 * 3 + 1, edge - 1, 95)),
                          [edge - 1, edge], np.sort(rng.integers(edge + 1, BLOCK_MAX, 3))])
    add('straddle_p99_k1', disk_from_block_sums(_placed(rng, 20, 20, srt), rng), 1, 'off1', fence=True)
    # ... and inside a high digit, on a chunk boundary of the low digit alone (16 fine bins a chunk)
    edge = 4096 * 7 + 16 * 9
    srt = np.concatenate([np.sort(rng.integers(0, edge - 1, 395)), [edge - 1, edge], np.sort(rng.integers(edge + 1, edge + 900, 3))])
    add('straddle_low_chunk_k1', disk_from_block_sums(_placed(rng, 20, 20, srt), rng), 1, 'vec')
    # k = 5, one array for both: 983 a block gives 25 * 983 = 6 * 4096 - 1; eight blocks one more, five apart, put 200 of the 400 windows
    # on 6 * 4096: the median pair is (24575, 24576), the 99th-percentile pair ties, data holds one value
    base = np.full((20, 20), 983, np.int64)
    for y, x in [(3, 3), (3, 9), (3, 15), (9, 3), (9, 9), (9, 15), (15, 3), (15, 9)]:
        base[y, x] += 1
    add('straddle_median_k5', disk_from_block_sums(base), 5, 'odd', fence=True)
    # ---- the one large case: n > 256 * 2048, the select's grid is capped and every thread takes more than one trip
    yy, xx = np.mgrid[0:2900, 0:2898]
    r2 = ((xx - 1500.0) / 1200.0) ** 2 + ((yy - 1400.0) / 1250.0) ** 2
    big = np.where(r2 < 1, 9000 + 30000 * np.sqrt(np.clip(1 - r2, 0, 1)), 900.0) + rng.normal(0, 250, r2.shape)
    add('725x725_k5', np.clip(big, 0, 65535), 5, 'vec', big=True)
    return out


# every class the set must reach; REQUIRED_MIN: classes that must be reached with at least this count in one case
REQUIRED = ('p99_pair_tied', 'p99_pair_apart_gamma_pos', 'p99_pair_apart_gamma_zero', 'p99_tied_with_values_below',
            'median_n_odd', 'median_n_even_tied', 'median_n_even_apart',
            'data_empty', 'data_one_value', 'data_many', 'on_interior_edge', 'on_last_edge',
            'padded_blocks_rows', 'padded_blocks_cols', 'reflect_once', 'reflect_more_than_once',
            'pair_straddles_high_digit', 'pair_straddles_high_chunk', 'pair_straddles_low_chunk',
            'sums_share_high_digit', 'sums_share_low_digit', 'largest_window_sum', 'k5_one_array',
            'several_tiles', 'flood_slots_wrap', 'select_one_full_group', 'select_several_groups', 'select_grid_capped',
            'vec_route', 'vec_route_partial_blocks', 'scalar_route', 'scalar_route_odd', 'scalar_route_off1')
REQUIRED_MIN = {'on_interior_edge_distinct': 3}
WINDOWS = (1, 2, 3, 4, 5, 6, 15, 16)           # every one of them occurs in the set
