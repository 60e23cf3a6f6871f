"""The warp cases of tests/test_pitched_rows_gpu.py and what each of them is there for, stated as facts about the sampling positions
x = h00 c + h01 r + h02 the reference (oracle.shg_oracle.warp_rows, scikit-image's _warp_fast) computes -- checked on the CPU
(tests/test_pitched_cases_cpu.py) and again before a case runs on the GPU, so that an edit of a number cannot quietly turn "runs
off the right edge" into one more interior case."""
import math

import numpy as np

# (id, h, w, out_h, out_w, h00, h01, h02, the facts the case must have)
WARP_CASES = [
    ('narrow9', 33, 9, 33, 40, 1.0, 0.5, -3.0, ('narrower_than_two_pieces', 'mostly_outside', 'beyond_left', 'beyond_right', 'source_tail')),
    ('nv2', 12, 8, 12, 9, 0.5, 0.0, -0.5, ('two_vectors_a_row', 'first_pixel_at_minus_half', 'left_fraction', 'shared_samples')),
    ('w15', 20, 15, 23, 17, 0.93, 0.11, -0.5, ('source_tail', 'rows_beyond_source', 'left_fraction', 'right_fraction')),
    ('w17', 20, 17, 20, 33, 0.55, -0.2, 2.25, ('source_tail', 'left_fraction', 'right_fraction', 'beyond_right')),
    ('w63', 40, 63, 40, 70, 1.0, 0.0, -2.4, ('source_tail', 'beyond_left', 'left_fraction', 'right_fraction', 'beyond_right')),
    ('w64', 40, 64, 44, 64, 1.0, 0.0, 0.5, ('no_padding', 'rows_beyond_source', 'right_fraction')),
    ('w65', 40, 65, 40, 65, 1.0, 0.01, -0.75, ('source_tail', 'left_fraction')),
    ('typical', 300, 517, 310, 540, 0.957, 0.013, -9.4, ('source_tail', 'beyond_left', 'left_fraction', 'rows_beyond_source')),
    ('whole', 257, 1003, 257, 1003, 1.0, 0.0, 5.0, ('whole_positions', 'beyond_right', 'source_tail')),
    ('widest', 64, 203, 64, 131, 1.75, 0.1, -20.25, ('widest_step', 'source_tail', 'beyond_left', 'beyond_right')),
    ('shared', 64, 203, 64, 300, 0.31, 0.0, 190.0, ('shared_samples', 'mostly_outside', 'beyond_right', 'right_fraction')),
    ('hair', 50, 301, 50, 300, 1.0, 0.0, -1e-13, ('weights_a_hair_from_one', 'left_fraction', 'source_tail')),
    ('h00_zero', 48, 77, 48, 90, 0.0, 0.9, 3.5, ('one_position_a_row', 'shared_samples', 'source_tail')),
    ('creep', 48, 77, 48, 90, 1e-3, 0.0, 75.95, ('creeps_across_last_column', 'right_fraction', 'shared_samples')),
    ('shear', 300, 131, 300, 200, 0.8, 0.9, -150.0, ('row_across', 'beyond_left', 'beyond_right', 'mostly_outside', 'source_tail')),
    ('steep_shear', 300, 131, 300, 200, 0.8, 2.0, -400.0, ('row_wholly_left', 'row_wholly_right', 'row_across', 'source_tail')),
    ('inside', 70, 4197, 70, 4200, 0.98, 0.004, 17.3, ('inside_waves', 'source_tail')),
    ('four_a_thread', 2100, 8197, 2100, 8192, 0.999, 1e-4, 2.0, ('four_vectors_a_thread', 'inside_waves', 'source_tail')),
]
WARP_IDS = [c[0] for c in WARP_CASES]


def warp_facts(h, w, oh, ow, h00, h01, h02, only=None):
    """What the positions of an (h, w) -> (oh, ow) warp look like (only the rows the source has count); `only`: the facts wanted."""
    rows = min(h, oh)
    r = np.arange(rows, dtype=np.float64)
    nv = -(-ow // 8)
    memo = {}

    def pos(cols):                                                    # warp_rows' own expression, row by row
        return h00 * np.asarray(cols, dtype=np.float64)[None, :] + h01 * r[:, None] + h02

    def x():
        if 'x' not in memo:
            memo['x'] = pos(np.arange(ow))
        return memo['x']

    def fl():
        if 'fl' not in memo:
            memo['fl'] = np.floor(x())
        return memo['fl']

    def ends():                                                       # first and last position of every 8-column vector (h00 >= 0: they bound the rest)
        if 'ends' not in memo:
            memo['ends'] = pos(np.arange(nv) * 8), pos(np.minimum(np.arange(nv) * 8 + 7, ow - 1))
        return memo['ends']
    facts = {
        'left_fraction': lambda: ((x() > -1) & (x() < 0)).any(),           # left neighbour outside, right one inside
        'right_fraction': lambda: ((x() > w - 1) & (x() < w)).any(),       # right neighbour outside, left one inside
        'beyond_left': lambda: (x() <= -1).any(),
        'beyond_right': lambda: (x() >= w).any(),
        'mostly_outside': lambda: ((x() < 0) | (x() > w - 1)).mean() > 0.5,
        'whole_positions': lambda: (x() == fl()).all(),
        'rows_beyond_source': lambda: oh > h,
        'row_wholly_left': lambda: (x() <= -1).all(axis=1).any(),
        'row_wholly_right': lambda: (x() >= w).all(axis=1).any(),
        'row_across': lambda: ((x() < 0).any(axis=1) & (x() > w - 1).any(axis=1)).any(),
        'one_position_a_row': lambda: h00 == 0.0,
        'creeps_across_last_column': lambda: ((ends()[0] < w - 1) & (ends()[1] > w - 1) & (ends()[1] - ends()[0] < 1)).any(),
        'weights_a_hair_from_one': lambda: ((x() - fl() > 1 - 1e-12) & (x() - fl() < 1)).any(),
        'shared_samples': lambda: ow > 1 and (fl()[:, 1:] == fl()[:, :-1]).any(),
        'widest_step': lambda: h00 == 1.75,
        'two_vectors_a_row': lambda: nv == 2,
        'first_pixel_at_minus_half': lambda: pos([0])[0, 0] == -0.5,
        'narrower_than_two_pieces': lambda: w < 16,
        'source_tail': lambda: w % 8 != 0,                                 # the window's pieces reach into the padding columns
        'no_padding': lambda: w % 64 == 0,                                 # the next row follows directly
        'inside_waves': lambda: ((ends()[0] >= 0) & (ends()[1] < w - 1)).mean() > 0.9,
        'four_vectors_a_thread': lambda: oh * nv >= 4 * 256 * 2048,
    }
    return {k: bool(f()) for k, f in facts.items() if only is None or k in only}


def assert_warp_case(case):
    name, h, w, oh, ow, h00, h01, h02, claims = case
    facts = warp_facts(h, w, oh, ow, h00, h01, h02, only=claims)
    missing = [k for k in claims if not facts[k]]
    assert not missing, 'warp case %s no longer has: %s' % (name, ', '.join(missing))
    assert 0.0 <= h00 <= 1.75 and w >= 8 and ow >= 9, 'warp case %s is not one for the eight-pixel kernel' % name


def warp_image(h, w, poison):
    """Noise in [2000, 60000] that never takes the padding's value; img[0, 0] (the warp's cval) = 31337."""
    rng = np.random.default_rng(h * 65537 + w)
    img = rng.integers(2000, 60001, (h, w)).astype(np.uint16)
    img[img == poison] += 1
    img[0, 0] = 31337
    assert 2000 < poison < 60000 and poison != 31337
    return img


def warp_reference(orc, img, oh, ow, h00, h01, h02, minmax=None):
    """(2**16 * warp(img / 65536)).astype(uint16), ellipse_to_circle.py:112-118; minmax: clip to this pair, not the image's own."""
    mat3 = np.array([[h00, h01, h02], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    warped = orc.warp_rows(img / 65536, mat3, (oh, ow), img[0, 0] / 65536)
    if minmax is not None:
        warped = np.clip(warped, minmax[0] / 65536, minmax[1] / 65536)
    return (2 ** 16 * warped).astype(np.uint16)


# ---- the row kernels (scale rows, contrast products) ------------------------------------------------------------------------------
ROW_WIDTHS = [8, 9, 15, 17, 1023, 2049, 2097, 4100]
ROW_HEIGHTS = [1, 2, 3, 5, 7, 130]                 # fewer rows than the four a lane takes, and counts that are no multiple of four


def product_discs(h, w):
    """(x0, y0, r) or None.  A row's span is [x0 - half, x0 + half], half = isqrt(r^2 - dy^2)."""
    y0 = h // 2
    t0 = (w // 8) * 8                                        # first column of the partial last vector (w % 8 != 0 for every width here)
    end = min(t0 + 1, w - 1)
    on_vectors = (12, y0, 4) if w >= 17 else (4, y0, 4)      # centre row [x0 - 4, x0 + 4] starts on a vector's first column, the rows one and
    #                                                          two off it ([x0 - 3, x0 + 3]) end on a vector's last (a span's length is odd:
    #                                                          no single row does both)
    return [None,
            (end - 3, y0, 3),                                # the centre row's span ends inside the partial last vector
            (w - 2, y0, 6),                                  # reaches past w
            (-50, y0, 20),                                   # wholly left of the image
            on_vectors,
            (w, y0, 1)]                                      # [w - 1, w + 1] on the centre row: a single pixel, in the last column


def disc_mask(h, w, disc):
    yy, xx = np.mgrid[0:h, 0:w]
    ady = np.abs(yy - disc[1])
    half = np.vectorize(lambda d: math.isqrt(max(disc[2] ** 2 - int(d) ** 2, 0)))(ady[:, 0])[:, None]
    return (ady <= disc[2]) & (np.abs(xx - disc[0]) <= half)     # cv2.circle(frame_protus, centre, r, 80, -1)
