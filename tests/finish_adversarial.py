"""Seeded adversarial inputs for shg_doppler_finish / shg_line_profile_finish: small geometries that each aim at a few of the
finish's decisions (the taps, the rows, the mask, the crop, the layout and the values), and the list of decision classes
(finish_exact.finish's Counter keys) that the whole set must reach.

A case is a dict: raw float32 [P, h, w]; geometry (h00, h01, h02, out_h, out_w); circle; crop (crop_plan's (nw, lo, dx0, n) or
None); display_range and half_width (the display planes); layout (extra elements of every pitch and plane stride, and the offset
of the raw view inside a larger tensor: what the GPU test allocates)."""
import math

import numpy as np

H, W = 9, 37                         # the raw map of most cases: 9 slit rows, 37 frames
# display values: with R = 32767 / 256 the shift / cog scale is exactly 256, with H = 3 (2H + 1 = 7 divides 65534) the width / ew
# scale is exactly 9362, so these land exactly on .5 ties (up and down), below 1 and above 65535 in every plane
TIE_RANGE = 32767.0 / 256.0
SPECIALS = np.array([1 / 512, 3 / 512, 0.25, 0.75, 2.5, 3.5, -200.0, 200.0, 70000.0, 0.3, -0.0, 0.0, 1e-40, -1e-42, np.inf, -np.inf,
                     np.nan, 7.0, -7.0], dtype=np.float32)


def values(rng, P, h, w, specials=True):
    """raw float32 [P, h, w]: N(0, 1.5), about 6 % NaN, and (specials) the SPECIALS along each plane's rows."""
    raw = rng.normal(0.0, 1.5, (P, h, w)).astype(np.float32)
    raw[rng.random((P, h, w)) < 0.06] = np.nan
    if specials:
        flat = raw.reshape(P, -1)
        for q in range(P):
            at = rng.choice(flat.shape[1], min(2 * len(SPECIALS), flat.shape[1]), replace=False)
            flat[q, at] = np.resize(SPECIALS, at.size)
    return raw


def _whole_right_nan(raw):
    """Columns 4, 11, 20 of every row: finite with a NaN right-hand neighbour; column 27: NaN itself, column 30: +inf."""
    for j in (4, 11, 20):
        raw[:, :, j] = 1.25 + j
        raw[:, :, j + 1] = np.nan
    raw[:, :, 27] = np.nan
    raw[:, :, 30] = np.inf
    return raw


LAYOUTS = ({}, {'raw_pitch': 3, 'map_pitch': 5, 'png_pitch': 7, 'raw_plane': 13, 'map_plane': 11, 'png_plane': 3, 'view': (1, 2)},
           {'raw_pitch': 1, 'map_pitch': 1, 'png_pitch': 2, 'raw_plane': 1, 'map_plane': 1, 'png_plane': 1, 'view': (2, 5)})


def cases(P, seed=0):
    """The adversarial cases for P planes (1: the Dopplergram's finish, 5: the line-profile finish)."""
    rng = np.random.default_rng([seed, P])
    out = []

    def add(name, raw, geometry, circle=None, crop=None, display_range=1.7, half_width=3):
        out.append(dict(name=name, raw=raw, geometry=tuple(geometry), circle=circle, crop=crop, display_range=display_range,
                        half_width=half_width if P > 1 else None, layout=LAYOUTS[len(out) % len(LAYOUTS)]))

    # ---- taps
    add('whole', _whole_right_nan(values(rng, P, H, W)), (1.0, 0.0, 0.0, H, W + 2), display_range=TIE_RANGE)
    add('whole_h1', values(rng, P, H, W), (1.0, 0.0, 0.0, H, W), display_range=TIE_RANGE, half_width=1)
    add('whole_h32', values(rng, P, H, W), (1.0, 0.0, 0.0, H, W), display_range=0.05, half_width=32)
    add('whole_shifted', _whole_right_nan(values(rng, P, H, W)), (1.0, 0.0, -3.0, H, W + 1))
    add('half', values(rng, P, H, W), (1.0, 0.0, -0.5, H, W + 2), display_range=TIE_RANGE)
    add('neg_zero', values(rng, P, 3, W), (-1.0, -1.0, -0.0, 3, 3))
    add('h00_zero', values(rng, P, H, W), (0.0, 0.5, 3.25, H, 20))
    add('warp_like', values(rng, P, H, W), (1.0734, 0.1213, -2.7, H, W + 4))
    add('warp_like_neg', values(rng, P, H, W), (0.913, -0.3137, 5.2, H, W + 6))
    add('steep', values(rng, P, H, W), (1.75, 0.0625, -0.375, H, 24))
    add('column_ramp', values(rng, P, H, W), (1.0, 1.0, -4.0, H, W))        # whole positions moving right a row at a time
    for name, g in (('far_pos', (1.0, 0.0, 1e20)), ('far_neg', (1.0, 0.0, -1e20)), ('far_2_63', (0.0, 0.0, 2.0 ** 63)),
                    ('huge', (1.0, 0.0, 1e300)), ('huge_neg', (1.0, 0.0, -1e300)), ('huge_step', (1e308, 0.0, 0.0)),
                    ('h02_inf', (1.0, 0.0, np.inf)), ('h02_-inf', (1.0, 0.0, -np.inf)), ('h02_nan', (1.0, 0.0, np.nan))):
        add(name, values(rng, P, 2, W, specials=False), g + (2, 5))
    # ---- rows
    add('rows_beyond', values(rng, P, H, W), (1.0, 0.25, 0.5, H + 4, W))
    add('one_row', values(rng, P, H, W), (1.0, 0.0, 0.0, 1, W))
    # ---- the mask (integer centres: the Pythagorean pixels lie on the circle exactly in float64)
    mh, mw = 24, 41
    ident = (1.0, 0.0, 0.0, mh, mw)
    add('circle_on', values(rng, P, mh, mw), ident, circle=(20.0, 12.0, 5.0))
    add('circle_in', values(rng, P, mh, mw), ident, circle=(20.0, 12.0, math.nextafter(10.0, 11.0)))
    add('circle_out', values(rng, P, mh, mw), ident, circle=(20.0, 12.0, math.nextafter(13.0, 0.0)))
    for d2 in (41, 50, 65, 85, 130, 145):            # rad = fl(sqrt(d2)): fl(rad^2) may be d2 though rad^2 is not
        add('circle_sqrt%d' % d2, values(rng, P, mh, mw), ident, circle=(20.0, 12.0, math.sqrt(d2)))
    add('circle_frac', values(rng, P, mh, mw), (1.0734, 0.1213, -1.2, mh, mw), circle=(19.7, 11.3, 9.55))
    add('circle_none', values(rng, P, mh, mw), ident, circle=None)
    add('circle_minus1', values(rng, P, mh, mw), ident, circle=(-1.0, -1.0, -1.0))
    # ---- the crop: (nw, lo, dx0, n)
    cw = 300
    for name, crop in (('crop_lo', (40, 5, 0, 35)), ('crop_pad_both', (50, 0, 7, 30)), ('crop_pad_right', (60, 250, 0, 50)),
                       ('crop_n0', (20, 3, 4, 0)), ('crop_nw1', (1, 10, 0, 1)), ('crop_wider', (320, 0, 10, 300)),
                       ('crop_255', (255, 20, 0, 255)), ('crop_256', (256, 0, 0, 256)), ('crop_257', (257, 5, 3, 254)),
                       ('crop_circle', (101, 130, 4, 97))):
        circle = (180.4, 1.5, 40.25) if name == 'crop_circle' else None
        add(name, values(rng, P, 2, cw), (1.0, 0.0, 0.0, 2, cw), circle=circle, crop=crop)
    return out


# every class the set must reach, on the exact reference and on the kernel
REQUIRED = ('x_whole', 'x_fraction', 'x_neg_zero', 'x_in_minus1_0', 'x_w_minus_1', 'x_in_last', 'whole_tap_nan', 'whole_tap_inf',
            'whole_right_neighbour_nan', 'x_far', 'x_nan', 'x_inf', 'h00_zero', 'tap_outside', 'row_beyond_h', 'crop_pad',
            'mask_on', 'mask_off', 'mask_none', 'mask_on_circle_f64', 'mask_just_in', 'mask_just_out', 'masked',
            'v_nan', 'v_inf', 'v_pos_zero', 'v_neg_zero', 'v_denormal', 'v_finite',
            'shift_tie_up', 'shift_tie_down', 'shift_below_1', 'shift_above_65535')
REQUIRED_PROFILE = tuple('%s_%s' % (p, k) for p in ('core', 'width', 'cog', 'ew')
                         for k in ('tie_up', 'tie_down', 'below_1', 'above_65535'))
# case-level classes: the geometry and the crop, by the case's own numbers
CASE_CLASSES = {
    'out_h_1': lambda c: c['geometry'][3] == 1,
    'out_h_gt_h': lambda c: c['geometry'][3] > c['raw'].shape[1],
    'crop_lo_gt_0': lambda c: c['crop'] is not None and c['crop'][1] > 0,
    'crop_pad_left': lambda c: c['crop'] is not None and c['crop'][2] > 0,
    'crop_pad_right': lambda c: c['crop'] is not None and c['crop'][2] + c['crop'][3] < c['crop'][0],
    'crop_n0': lambda c: c['crop'] is not None and c['crop'][3] == 0,
    'crop_nw1': lambda c: c['crop'] is not None and c['crop'][0] == 1,
    'crop_nw_gt_out_w': lambda c: c['crop'] is not None and c['crop'][0] > c['geometry'][4],
    'nw_255': lambda c: c['crop'] is not None and c['crop'][0] == 255,
    'nw_256': lambda c: c['crop'] is not None and c['crop'][0] == 256,
    'nw_257': lambda c: c['crop'] is not None and c['crop'][0] == 257,
    'half_width_1': lambda c: c['half_width'] == 1,
    'half_width_32': lambda c: c['half_width'] == 32,
    'pitched': lambda c: c['layout'].get('raw_pitch', 0) % 4 != 0 and c['layout'].get('map_pitch', 0) % 4 != 0,
    'view': lambda c: 'view' in c['layout'],
}


def case_classes(all_cases, P):
    """How many cases reach each case-level class (the half-width ones only where there are display planes of width)."""
    names = [k for k in CASE_CLASSES if P > 1 or not k.startswith('half_width')]
    return {k: sum(bool(CASE_CLASSES[k](c)) for c in all_cases) for k in names}
