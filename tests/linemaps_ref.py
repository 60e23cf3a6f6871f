"""NumPy restatement of the line maps' six kernels (include/shg_hip.h: shg_line_core_shift, shg_line_profile, shg_line_bisector
and their finishes), written from the arithmetic the header states, not from the kernels: the GPU must match these bit for bit.
Laid out as the header states the calls: the window, the vertex, the sums, one crossing walk at a float64 level, the column
placement and one finish.  Also the synthetic disk scans with known fields, and the accuracy the restatement reaches on them."""
import numpy as np

C_KM_S = 299792.458
PLANES = ('shift', 'core', 'width', 'cog', 'ew')


def profiles(frames, y):
    """p(j) of slit row y in every frame: int64 [n, iw].  a1's rotation (out[i, j] = raw[j, W - 1 - i] when W > H), 8-bit x 256."""
    frames = np.asarray(frames)
    _, h, w = frames.shape
    p = frames[:, :, w - 1 - y] if w > h else frames[:, y, :]
    p = p.astype(np.int64)
    return p * 256 if frames.dtype == np.uint8 else p


def window(f0, shift, half_width, iw):
    """(lo, hi) of a slit row, or None: c = int(fit[y, 0] + S) (truncated, as a5's astype(int)), lo = max(c - H, 1),
    hi = min(c + H, iw - 2), none when fit[y, 0] is not finite or hi - lo < 2.  The Dopplergram's window is S = 0."""
    if not np.isfinite(f0):
        return None
    c = int(np.clip(np.float64(f0) + np.float64(shift), -2.0 ** 30, 2.0 ** 30))
    lo, hi = max(c - half_width, 1), min(c + half_width, iw - 2)
    return None if hi - lo < 2 else (lo, hi)


def vertex(seg, lo, ref):
    """The frames k whose first minimum j* over the window seg = p[:, lo:hi + 1] lies inside it, and their j* - lo, a, b, e, den,
    shift (float32) and core_d."""
    jrel = np.argmin(seg, axis=1)                        # first occurrence
    k = np.flatnonzero((jrel > 0) & (jrel < seg.shape[1] - 1))
    rk = jrel[k]
    a, b, e = seg[k, rk - 1], seg[k, rk], seg[k, rk + 1]
    den = a + e - 2 * b
    delta = (a - e).astype(np.float64) / (2 * den).astype(np.float64)
    shift = (((lo + rk).astype(np.float64) + delta) - ref).astype(np.float32)
    core_d = b.astype(np.float64) - ((a - e) * (a - e)).astype(np.float64) / (8.0 * den.astype(np.float64))
    return dict(k=k, rk=rk, a=a, b=b, e=e, den=den, shift=shift, core_d=core_d)


def sums(seg, lo, ref):
    """C2, S0, S1 (int64) and cog, ew (float32, NaN when S0 <= 0 / C2 == 0) of every frame over the window seg."""
    m = seg.shape[1]
    jj = np.arange(lo, lo + m, dtype=np.int64)
    c2 = seg[:, 0] + seg[:, -1]
    s0 = m * c2 - 2 * seg.sum(axis=1)
    s1 = c2 * jj.sum() - 2 * (seg * jj).sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        cog = (s1.astype(np.float64) / s0.astype(np.float64) - ref).astype(np.float32)
        ew = (s0.astype(np.float64) / c2.astype(np.float64)).astype(np.float32)
    return c2, s0, s1, np.where(s0 > 0, cog, np.float32(np.nan)), np.where(c2 != 0, ew, np.float32(np.nan))


def crossings(sk, rk, b, level, lo):
    """(has, xl, xr) of the window rows sk [k, m] with their minimum at rk, at the float64 level [k]: has = p(j*) < level and both
    jl (the largest j in [lo, j*) with p >= level) and jr (the smallest j in (j*, hi] with p >= level) exist."""
    m = sk.shape[1]
    ge = sk >= level[:, None]
    idx = np.arange(m)[None, :]
    jl = np.where(ge & (idx < rk[:, None]), idx, -1).max(axis=1)
    jr = np.where(ge & (idx > rk[:, None]), idx, m).min(axis=1)
    has = (b.astype(np.float64) < level) & (jl >= 0) & (jr < m)
    rows = np.arange(sk.shape[0])
    jl, jr = np.clip(jl, 0, m - 2), np.clip(jr, 1, m - 1)
    pl, pl1, pr, pr1 = sk[rows, jl], sk[rows, jl + 1], sk[rows, jr], sk[rows, jr - 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        xl = (lo + jl).astype(np.float64) + (pl.astype(np.float64) - level) / (pl - pl1).astype(np.float64)
        xr = (lo + jr).astype(np.float64) - (pr.astype(np.float64) - level) / (pr - pr1).astype(np.float64)
    return has, xl, xr


def level_of(f, core_d, c2):
    """level = ((1.0 - f) * core_d) + (f * (0.5 * (double)C2)), one IEEE operation a step."""
    f = np.float64(f)
    return ((np.float64(1.0) - f) * core_d) + (f * (np.float64(0.5) * np.asarray(c2, dtype=np.float64)))


def _map(frames, fit, half_width, shift, n_planes, measure, flip_x, n_cols, k_offset):
    """planes float32 [n_planes, ih, n_cols]: measure(p, lo, hi, ref) -> [n_planes, n] of every slit row with a window, placed in
    the columns k_offset .. k_offset + n - 1 (reversed with flip_x); the other columns NaN."""
    frames = np.asarray(frames)
    fit = np.asarray(fit, dtype=np.float64)
    n, h, w = frames.shape
    ih, iw = (w, h) if w > h else (h, w)
    n_cols = n if n_cols is None else int(n_cols)
    out = np.full((n_planes, ih, n_cols), np.nan, dtype=np.float32)
    cols = k_offset + np.arange(n)
    cols = n_cols - 1 - cols if flip_x else cols
    for y in range(ih):
        win = window(fit[y, 0], shift, half_width, iw)
        if win is not None:
            out[:, y, cols] = measure(profiles(frames, y), *win, fit[y, 3] + np.float64(shift))
    return out


def _planes(p, lo, hi, ref, levels=None):
    """The five PLANES of the profiles p [n, iw] over [lo, hi] or, given levels, the K bisectors then the K chords."""
    seg = p[:, lo:hi + 1]
    out = np.full((len(PLANES) if levels is None else 2 * len(levels), p.shape[0]), np.nan, dtype=np.float32)
    c2, _, _, cog, ew = sums(seg, lo, ref)
    v = vertex(seg, lo, ref)
    k, c2k, sk = v['k'], c2[v['k']], seg[v['k']]
    if levels is None:
        out[3], out[4] = cog, ew
        out[0, k], out[1, k] = v['shift'], v['core_d'].astype(np.float32)
        half = 0.5 * (0.5 * c2k.astype(np.float64) + v['core_d'])          # the header's half, as it writes it
        has, xl, xr = crossings(sk, v['rk'], v['b'], half, lo)
        out[2, k] = np.where(has, (xr - xl).astype(np.float32), np.float32(np.nan))
        return out
    for i, f in enumerate(levels):
        has, xl, xr = crossings(sk, v['rk'], v['b'], level_of(f, v['core_d'], c2k), lo)
        with np.errstate(invalid='ignore', divide='ignore'):
            out[i, k] = np.where(has, ((0.5 * (xl + xr)) - ref).astype(np.float32), np.float32(np.nan))
            out[len(levels) + i, k] = np.where(has, (xr - xl).astype(np.float32), np.float32(np.nan))
    return out


def line_core_shift(frames, fit, half_width, flip_x=False, n_cols=None, k_offset=0):
    """map float32 [ih, n_cols]: the shift plane of line_profile at S = 0."""
    return _map(frames, fit, half_width, 0, 1, lambda p, lo, hi, ref: _planes(p, lo, hi, ref)[:1], flip_x, n_cols, k_offset)[0]


def line_profile(frames, fit, half_width, shift=0, flip_x=False, n_cols=None, k_offset=0):
    """planes float32 [5, ih, n_cols] (PLANES order) of frames [n, H, W] (file layout)."""
    return _map(frames, fit, half_width, shift, len(PLANES), _planes, flip_x, n_cols, k_offset)


def line_bisector(frames, fit, half_width, levels, shift=0, flip_x=False, n_cols=None, k_offset=0):
    """planes float32 [2K, ih, n_cols] (bisectors, then chords) of frames [n, H, W] (file layout)."""
    levels = [float(f) for f in levels]
    return _map(frames, fit, half_width, shift, 2 * len(levels), lambda p, lo, hi, ref: _planes(p, lo, hi, ref, levels),
                flip_x, n_cols, k_offset)


def _warp(raw, h00, h01, h02, out_h, out_w, circle, crop):
    """One raw plane float32 [h, w] in the products' geometry: x = (h00 c + h01 r) + h02, taps floor / ceil of row r (NaN outside
    [0, w) and for r >= h), (1 - t) L + t R in float64 then float32, NaN outside the circle, crop_plan's (nw, lo, dx0, n)."""
    raw = np.asarray(raw, dtype=np.float32)
    h, w = raw.shape
    r = np.arange(out_h, dtype=np.float64)[:, None]
    c = np.arange(out_w, dtype=np.float64)[None, :]
    x = (h00 * c + h01 * r) + h02
    x0, x1 = np.floor(x), np.ceil(x)
    t = x - x0
    rows = np.broadcast_to(np.arange(out_h)[:, None], x.shape)
    src = np.full((max(out_h, h), w), np.nan, dtype=np.float64)
    src[:h] = raw

    def tap(xi):
        inside = (xi >= 0) & (xi < w)
        idx = np.where(inside, xi, 0).astype(np.int64)
        return np.where(inside, src[rows, idx], np.nan)

    with np.errstate(invalid='ignore'):
        v = ((1.0 - t) * tap(x0) + t * tap(x1)).astype(np.float32)
    if circle is not None and tuple(circle) != (-1, -1, -1):
        cx, cy, rad = (float(q) for q in circle)
        dx, dy = c - cx, r - cy
        v[dx * dx + dy * dy > rad * rad] = np.nan
    if crop is not None:
        nw, lo, dx0, n = (int(q) for q in crop)
        out = np.full((out_h, nw), np.nan, dtype=np.float32)
        out[:, dx0:dx0 + n] = v[:, lo:lo + n]
        v = out
    return v


def display(v, kind, half_width, display_range):
    """uint16 display plane of one finished plane: 0 for NaN, else clip(rint(e), 1, 65535), e as the header states: the velocity
    scale for shift, cog and the bisectors, v for core, the window scale for width, ew and the chords."""
    v64 = np.asarray(v, dtype=np.float32).astype(np.float64)
    if kind in ('shift', 'cog', 'bisector'):
        e = 32768.0 + v64 * (32767.0 / float(display_range))
    elif kind == 'core':
        e = v64
    else:
        e = 1.0 + v64 * (65534.0 / float(2 * half_width + 1))
    with np.errstate(invalid='ignore'):
        q = np.clip(np.rint(e), 1, 65535)
    return np.where(np.isnan(v), 0, q).astype(np.uint16)


def finish(raw, kinds, h00, h01, h02, out_h, out_w, circle=None, crop=None, half_width=None, display_range=None):
    """(maps float32 [P, out_h, nw], png uint16 [P, out_h, nw] or None): every plane of raw [P, h, w] warped alike, plane q's
    display as display(kinds[q])."""
    maps = np.stack([_warp(r, h00, h01, h02, out_h, out_w, circle, crop) for r in raw])
    if display_range is None:
        return maps, None
    return maps, np.stack([display(m, kind, half_width, display_range) for m, kind in zip(maps, kinds)])


def doppler_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, display_range=None):
    """(map float32 [out_h, nw], png uint16 or None) of the raw map float32 [h, w]."""
    maps, png = finish(np.asarray(raw)[None], ('shift',), h00, h01, h02, out_h, out_w, circle, crop, None, display_range)
    return maps[0], None if png is None else png[0]


def line_profile_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, half_width=None, display_range=None):
    return finish(raw, PLANES, h00, h01, h02, out_h, out_w, circle, crop, half_width, display_range)


def line_bisector_finish(raw, h00, h01, h02, out_h, out_w, circle=None, crop=None, half_width=None, display_range=None):
    kk = raw.shape[0] // 2
    return finish(raw, ('bisector',) * kk + ('chord',) * kk, h00, h01, h02, out_h, out_w, circle, crop, half_width, display_range)


# ---- synthetic disk scans with known fields ----
def disk_scan(line, ih, n, iw, noise=0.004, seed=0, rotate=True, gain=None):
    """synth's scene (a limb-darkened disk crossing the slit) with the relative line profile line(x [1, iw], centre
    [ih], frame k) -> [ih, iw] and the continuum of frame k times gain[:, k] -> (frames uint16 in file layout, true line centre
    [ih], disk mask [ih, n], continuum [ih, n] on the relative scale)."""
    from solex_ser_recon_en_amd import synth
    sp = synth.scene_params(n, ih, iw)
    y = np.arange(ih, dtype=np.float64)
    x = np.arange(iw, dtype=np.float64)[None, :]
    centre = synth.curve_of_row(y, ih, iw)
    lit = ((y > sp['y_lo']) & (y < sp['y_hi'])).astype(np.float64)
    frames = np.empty((n, iw, ih) if rotate else (n, ih, iw), dtype=np.uint16)
    on = np.zeros((ih, n), dtype=bool)
    cont = np.zeros((ih, n))
    for k in range(n):
        r2 = ((k - sp['cx']) / sp['ax']) ** 2 + ((y - sp['cy']) / sp['ay']) ** 2
        on[:, k] = (r2 < 0.9) & (lit > 0)
        bright = np.where(r2 < 1.0, 0.35 + 0.65 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0)), sp['sky']) * lit
        if gain is not None:
            bright = bright * gain[:, k]
        cont[:, k] = sp['gain'] * bright
        img = cont[:, k:k + 1] * line(x, centre, k) + noise * np.random.default_rng([seed, k]).standard_normal((ih, iw))
        img = np.clip(np.rint(img * 65535.0), 0, 65535).astype(np.uint16)
        frames[k] = np.rot90(img, -1) if rotate else img
    return frames, centre, on, cont


def gaussian(shift, sigma=3.0, depth=0.8):
    """The Gaussian line (synth's width and depth by default) of frame k, row y displaced by shift[y, k] px, of width sigma and
    depth depth (scalars or [ih, n])."""
    def col(v, k):
        return v[:, k:k + 1] if np.ndim(v) else v
    return lambda x, c, k: 1.0 - col(depth, k) * np.exp(-0.5 * ((x - (c + shift[:, k])[:, None]) / col(sigma, k)) ** 2)


def injected_field(ih, n, gradient=1.5, blob=1.0):
    """A linear +-gradient px ramp across the frames plus a +-blob px Gaussian (positive) at a quarter of the disk."""
    y = np.arange(ih, dtype=np.float64)[:, None]
    k = np.arange(n, dtype=np.float64)[None, :]
    ramp = gradient * (2.0 * k / max(n - 1, 1) - 1.0)
    g = blob * np.exp(-0.5 * (((y - 0.35 * ih) / (0.08 * ih)) ** 2 + ((k - 0.6 * n) / (0.08 * n)) ** 2))
    return ramp + g


def injected_fields(ih, n, sigma=3.0, depth=0.8):
    """(shift, sigma, depth) [ih, n]: injected_field's shift; sigma and depth varied by +-20 % / -25 % in two Gaussian patches
    (a 'filament' that broadens the line and a 'plage' that fills it in) and a linear ramp of sigma across the slit."""
    y = np.arange(ih, dtype=np.float64)[:, None]
    k = np.arange(n, dtype=np.float64)[None, :]
    shift = injected_field(ih, n)
    fil = np.exp(-0.5 * (((y - 0.6 * ih) / (0.06 * ih)) ** 2 + ((k - 0.4 * n) / (0.12 * n)) ** 2))
    plage = np.exp(-0.5 * (((y - 0.45 * ih) / (0.1 * ih)) ** 2 + ((k - 0.55 * n) / (0.1 * n)) ** 2))
    s = sigma * (1.0 + 0.2 * fil + 0.1 * (2.0 * y / max(ih - 1, 1) - 1.0)) + 0.0 * k
    d = depth * (1.0 - 0.25 * plage) + 0.0 * y
    return shift, s, d


def doppler_scan(field, iw, noise=0.004, seed=0, rotate=True):
    """synth's curved Gaussian line displaced by field[y, k] px -> (frames, true line centre [ih] before the displacement, on)."""
    return disk_scan(gaussian(field), *field.shape, iw, noise, seed, rotate)[:3]


def profile_scan(shift, sigma, depth, iw, noise=0.004, seed=0, rotate=True):
    """The Gaussian line of the fields (shift, sigma, depth) -> (frames, centre, on, the noise-free core intensity [ih, n] on the
    sample scale)."""
    frames, centre, on, cont = disk_scan(gaussian(shift, sigma, depth), *shift.shape, iw, noise, seed, rotate)
    return frames, centre, on, cont * (1.0 - depth) * 65535.0


def profile_errors(planes, fit, shift, sigma, depth, centre, core, on):
    """(RMS, max) on the disk of: cog's line position against the injected one (px), width against 2 sqrt(2 ln 2) sigma (px), and
    core against the noise-free core intensity (relative)."""
    pos = planes[3].astype(np.float64) + fit[:, 3:4]
    fwhm = 2.0 * np.sqrt(2.0 * np.log(2.0)) * sigma
    out = {}
    with np.errstate(invalid='ignore', divide='ignore'):
        core_err = planes[1] / core - 1.0
    for name, err in (('cog', pos - (centre[:, None] + shift)), ('width', planes[2] - fwhm), ('core', core_err)):
        e = err[on]
        out[name] = (float(np.sqrt(np.mean(e * e))), float(np.abs(e).max()), int(np.isnan(e).sum()))
    return out


# the asymmetric line: a narrow deep component and a broad shallow one, each displaced by its own field
NARROW = (0.6, 1.6)          # (depth, sigma px)
BROAD = (0.25, 4.5)


def asym_fields(ih, n):
    """(s1, s2) [ih, n]: the narrow component's shift (injected_field) and the broad one's (0.5 s1 + 1.2 px, a red wing)."""
    s1 = injected_field(ih, n)
    return s1, 0.5 * s1 + 1.2


def asym_line(x, c1, c2):
    """The asymmetric line's relative profile at x (broadcast) with the components centred on c1 and c2."""
    return (1.0 - NARROW[0] * np.exp(-0.5 * ((x - c1) / NARROW[1]) ** 2)
            - BROAD[0] * np.exp(-0.5 * ((x - c2) / BROAD[1]) ** 2))


def asym_truth(fit, half_width, levels, centre, s1, s2, iters=60):
    """Reference bisectors [K, ih, n] of the asymmetric scan, in pixels from fit[y, 3], found on the analytic profile with the
    kernel's definitions: the window [lo, hi] of fit[y, 0]; continuum = the mean of the profile at lo and hi; core = the profile's
    minimum in the window (golden-section search); level = (1 - f) core + f continuum; the crossings the roots of profile = level
    between lo and the minimum and between the minimum and hi (bisection), NaN where a side does not reach the level."""
    ih, n = s1.shape
    iw_big = 1 << 20
    out = np.full((len(levels), ih, n), np.nan)
    for y in range(ih):
        win = window(fit[y, 0], 0, half_width, iw_big)
        if win is None:
            continue
        lo, hi = float(win[0]), float(win[1])
        c1, c2 = centre[y] + s1[y], centre[y] + s2[y]

        def prof(x):
            return asym_line(x, c1, c2)

        a, b = np.full(n, lo), np.full(n, hi)
        g = (np.sqrt(5.0) - 1.0) / 2.0
        for _ in range(iters):
            x1, x2 = b - g * (b - a), a + g * (b - a)
            left = prof(x1) < prof(x2)
            b = np.where(left, x2, b)
            a = np.where(left, a, x1)
        xm = 0.5 * (a + b)
        core, cont = prof(xm), 0.5 * (prof(np.full(n, lo)) + prof(np.full(n, hi)))
        for i, f in enumerate(levels):
            level = (1.0 - f) * core + f * cont
            roots = []
            for u, v in ((np.full(n, lo), xm), (xm, np.full(n, hi))):
                ok = (prof(u) - level) * (prof(v) - level) <= 0
                uu, vv = u.copy(), v.copy()
                for _ in range(iters):
                    mid = 0.5 * (uu + vv)
                    same = (prof(mid) - level) * (prof(uu) - level) > 0
                    uu = np.where(same, mid, uu)
                    vv = np.where(same, vv, mid)
                roots.append(np.where(ok, 0.5 * (uu + vv), np.nan))
            out[i, y] = 0.5 * (roots[0] + roots[1]) - fit[y, 3]
    return out


def sym_truth(fit, centre, shift, k):
    """The symmetric scan's true bisector of every level [K, ih, n]: the line's centre, from fit[y, 3]."""
    return np.broadcast_to((centre[:, None] + shift) - fit[:, 3:4], (k,) + shift.shape)


def bisector_errors(bis, truth, on):
    """{level index: (RMS, max |error| px, NaN count)} of bisector planes [K, ih, n] against the truth [K, ih, n] on the disk."""
    out = {}
    for i in range(bis.shape[0]):
        e = bis[i].astype(np.float64)[on] - truth[i][on]
        out[i] = (float(np.sqrt(np.nanmean(e * e))), float(np.nanmax(np.abs(e))), int(np.isnan(e).sum()))
    return out


def bisector_scan(kind, ih, n, iw, noise, seed=3):
    """(frames, centre, on, truth(fit, half_width, levels) -> [K, ih, n]) of the symmetric scan (profile_scan's: every bisector of
    a symmetric line is its centre) or the asymmetric one."""
    if kind == 'symmetric':
        shift, sigma, depth = injected_fields(ih, n)
        frames, centre, on, _ = profile_scan(shift, sigma, depth, iw, noise, seed)
        return frames, centre, on, lambda fit, hw, levels: sym_truth(fit, centre, shift, len(levels))
    s1, s2 = asym_fields(ih, n)
    frames, centre, on, _ = disk_scan(lambda x, c, k: asym_line(x, (c + s1[:, k])[:, None], (c + s2[:, k])[:, None]), ih, n, iw,
                                      noise, seed)
    return frames, centre, on, lambda fit, hw, levels: asym_truth(fit, hw, levels, centre, s1, s2)


# What the restatement achieves, measured, not assumed (the CPU tests re-measure them); the values are the measurements rounded up
# in their last digit.
#  doppler: on doppler_scan(injected_field(400, 300), 48, noise, seed=3) with the exact line centre as the fit, (RMS, max) of
#    |shift - injected| on the disk in px: 0.0038 / 0.0056 without noise, 0.072 / 0.434 at synth's 0.004.
#  profile: on profile_scan(*injected_fields(400, 300), 48, noise, seed=3) at H = 10 with the fitted line placed off the true centre
#    by each of FIT_OFFSETS px (a scan's own fit lies within a pixel of it; the window moves with int(fit[y, 0]), and a window
#    off-centre on the line biases cog and width): the worst (RMS, max) of profile_errors() on the disk.  Without noise cog
#    0.0899 / 0.317 px, width 0.0677 / 0.193 px, core 0.0014 / 0.0046; at 0.004 cog 0.101 / 0.503, width 0.0991 / 0.501, core
#    0.0286 / 0.165.
#  bisector: at H = 10 on the levels LEVELS, on bisector_scan(kind, 400, 300, 48) (seed 3) with the fit off by each of FIT_OFFSETS:
#    the worst (RMS, max) bisector error in px on the disk over the levels and offsets.  Without noise: symmetric 0.0116 / 0.0265
#    (the worst at f = 0.8, where the linear interpolation between samples is coarsest against the Gaussian's curvature),
#    asymmetric 0.0228 / 0.0466; at 0.004: symmetric 0.0416 / 0.1999, asymmetric 0.0711 / 0.511 (f = 0.8, near the continuum,
#    where the profile is flattest and the noise moves the crossings most).  No NaN on the disk in either.
LEVELS = (0.2, 0.4, 0.5, 0.6, 0.8)
FIT_OFFSETS = (-1.0, -0.5, 0.0, 0.5, 1.0)
TOLERANCE = {
    'doppler': {0.0: (0.004, 0.006), 0.004: (0.075, 0.46)},
    'profile': {0.0: {'cog': (0.09, 0.32), 'width': (0.068, 0.2), 'core': (0.0014, 0.0047)},
                0.004: {'cog': (0.101, 0.51), 'width': (0.1, 0.51), 'core': (0.029, 0.166)}},
    'bisector': {0.0: {'symmetric': (0.012, 0.027), 'asymmetric': (0.023, 0.047)},
                 0.004: {'symmetric': (0.042, 0.201), 'asymmetric': (0.072, 0.52)}}}
