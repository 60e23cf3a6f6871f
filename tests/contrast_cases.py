"""The images and the case table of tests/test_contrast_oracle_gpu.py (NumPy only, deterministic).  Every builder carries the
property it is there for as a checkable fact; tests/test_contrast_cases_cpu.py checks those facts from the image and the reference
alone, and asks the library's own plan (shg_contrast_plan_query) whether each case lands on the route its id names."""
import numpy as np

HIST = 65536
PCT = 99.9999


# ---- the geometry and the numbers the oracle's CLAHE works with ------------------------------------------------------------
def grid(h, w, tiles):
    """-> (he, we, th, tw): the padded size (cv2's copyMakeBorder: both axes to the next multiple when either does not divide) and a tile's."""
    if h % tiles or w % tiles:
        he, we = h + tiles - h % tiles, w + tiles - w % tiles
    else:
        he, we = h, w
    return he, we, he // tiles, we // tiles


def clip_of(clip_limit, area):
    return max(int(clip_limit * area / HIST), 1) if clip_limit > 0 else 0


def clip_limit_for(clip, area):
    """A clip limit that gives exactly `clip` pixels a bin on tiles of `area` pixels."""
    limit = (clip + 0.5) * HIST / area
    assert clip_of(limit, area) == clip
    return limit


def k_tops(n):
    """np.percentile(x, 99.9999) of n values reads the (n - lo)-th and (n - hi)-th LARGEST: -> (n - lo, n - hi)."""
    lo = int(np.floor((n - 1) * (PCT / 100)))
    return n - lo, n - min(lo + 1, n - 1)


def padded(img, tiles):
    h, w = img.shape
    he, we, _, _ = grid(h, w, tiles)
    return img if (he, we) == (h, w) else np.pad(img, ((0, he - h), (0, we - w)), mode='reflect')


def tile_hists(img, tiles):
    """[tiles * tiles][65536]: what each tile of the padded image counts."""
    src = padded(img, tiles)
    th, tw = src.shape[0] // tiles, src.shape[1] // tiles
    return np.stack([np.bincount(src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=HIST)
                     for ty in range(tiles) for tx in range(tiles)])


def clip_facts(hist, clip):
    """CLAHE_CalcLut_Body's redistribution numbers of one tile histogram."""
    clipped = int(np.maximum(hist - clip, 0).sum())
    batch = clipped // HIST
    residual = clipped - batch * HIST
    return dict(clipped=clipped, batch=batch, residual=residual, step=max(HIST // residual, 1) if residual else None)


# ---- the solar family of tests/test_kernels_gpu.py (flat sky, optional flat top) -------------------------------------------
def solar(h, w, seed, flat_top=False, sky=0.01, gain=1.0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.hypot(yy - h / 2, xx - w / 2) / (0.42 * min(h, w))
    disc = np.where(r < 1, 0.35 + 0.55 * np.sqrt(np.clip(1 - r * r, 0, 1)), sky)
    img = np.clip((disc + 0.01 * rng.standard_normal((h, w))) * 65535, 0, 65535).astype(np.uint16)
    img[r >= 1] = int(sky * 65535)
    if flat_top:
        img[img > 55000] = 65535
    if gain != 1.0:
        img = np.clip(img.astype(np.float64) * gain, 0, 65535).astype(np.uint16)
    img[0, 0] = 777 + seed % 100                         # the padding value of a crop is img[0, 0]: unlike its neighbours
    return img


# ---- planted tile histograms -------------------------------------------------------------------------------------------------
class Infeasible(Exception):
    pass


TARGETS = (1, 2, 21845, 21846, 32768, 32769, 65535, 65536, 65537)
LAYOUTS = ('band', 'rows', 'mirror')


def heavy_value(tile, seed):
    return 20000 + 1000 * tile + 37 * (seed % 20)


def planted(h, w, tiles, clip, target, layout, seed=0):
    """Every tile of the padded image counts ONE value (heavy_value) exactly target + clip times and every other value at most clip
    times: the clipped excess of every tile is `target`.  layout: 'band' -- the heavy pixels are the tile's first in row order (one
    slice holds them all); 'rows' -- dealt one to a row, row after row (a slice holds few, the tile all); 'mirror' -- first the
    pixels the reflected border counts a second time (last row / column but one of a size the grid does not divide)."""
    he, we, th, tw = grid(h, w, tiles)
    goal = target + clip
    if goal > th * tw:
        raise Infeasible('a %d x %d tile cannot hold %d + %d pixels' % (th, tw, target, clip))
    idx = np.arange(h * w).reshape(h, w)
    pidx = idx if (he, we) == (h, w) else np.pad(idx, ((0, he - h), (0, we - w)), mode='reflect')
    rng = np.random.default_rng(1000 * seed + target % 997)
    out = np.zeros(h * w, dtype=np.uint16)
    for t in range(tiles * tiles):
        ty, tx = divmod(t, tiles)
        ids, wt = np.unique(pidx[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw], return_counts=True)   # the tile's own pixels, how often it counts each
        nrows, ncols = ids[-1] // w - ids[0] // w + 1, ids[-1] % w - ids[0] % w + 1
        assert ids.size == nrows * ncols
        j = np.arange(ids.size)
        if layout == 'band':
            order = j
        elif layout == 'rows':
            yy = j % nrows
            order = yy * ncols + (j // nrows + yy) % ncols
        elif layout == 'mirror':
            order = np.argsort(-wt, kind='stable')
        else:
            raise ValueError(layout)
        cw = np.cumsum(wt[order])
        n_full = int(np.searchsorted(cw, goal, side='right'))
        take = list(order[:n_full])
        rem, j = goal - (int(cw[n_full - 1]) if n_full else 0), n_full
        while rem > 0:
            if wt[order[j]] <= rem:
                take.append(order[j])
                rem -= int(wt[order[j]])
            j += 1
        heavy = np.zeros(ids.size, dtype=bool)
        heavy[take] = True
        v = heavy_value(t, seed)
        out[ids[heavy]] = v
        multi, single = ~heavy & (wt > 1), ~heavy & (wt == 1)
        if multi.any() and int(wt[multi].max()) > clip:
            raise Infeasible('a pixel counted %d times cannot stay at %d a bin' % (int(wt[multi].max()), clip))
        n_multi, n_single = int(multi.sum()), int(single.sum())
        n_values = -(-n_single // clip)
        if n_multi + n_values > HIST - 1:
            raise Infeasible('%d other pixels at %d a bin need more than 65535 values' % (n_single + n_multi, clip))
        pool = rng.permutation(HIST)
        pool = pool[pool != v]
        out[ids[multi]] = pool[:n_multi]
        out[ids[single]] = rng.permutation(np.repeat(pool[n_multi:n_multi + n_values], clip)[:n_single])
    return out.reshape(h, w)


def heavy_per_slice(img, tiles, slice_rows, seed=0):
    """The largest number of heavy pixels any slice (slice_rows rows of a tile of the padded image) counts."""
    src = padded(img, tiles)
    th, tw = src.shape[0] // tiles, src.shape[1] // tiles
    worst = 0
    for t in range(tiles * tiles):
        ty, tx = divmod(t, tiles)
        rows = (src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] == heavy_value(t, seed)).sum(axis=1)
        worst = max(worst, max(int(rows[y:y + slice_rows].sum()) for y in range(0, th, slice_rows)))
    return worst


# ---- the top of the histogram --------------------------------------------------------------------------------------------------
TOP = 65000


def top_image(h, w, seed, count, place='scatter', second=None):
    """The solar image kept below 60000, then exactly `count` pixels of TOP: scattered, as a run in the last row but one
    ('mirror_row': the row a border below mirrors), or in the last column but one ('mirror_col').  second = (value, count): that many
    scattered pixels of a second value below TOP."""
    img = np.minimum(solar(h, w, seed), 60000).astype(np.uint16)
    rng = np.random.default_rng(7000 + seed)
    free = rng.permutation(h * w)
    if place == 'scatter':
        pos = free[:count]
    elif place == 'mirror_row':
        assert count <= w - w // 3 - 2
        pos = (h - 2) * w + w // 3 + np.arange(count)
    elif place == 'mirror_col':
        assert count <= h - h // 3 - 2
        pos = (h // 3 + np.arange(count)) * w + (w - 2)
    else:
        raise ValueError(place)
    img.flat[pos] = TOP
    if second:
        rest = free[~np.isin(free, pos)]
        img.flat[rest[:second[1]]] = second[0]
    return img


def kth_largest(img, k):
    return int(np.partition(img.ravel(), img.size - k)[img.size - k])


def served_from_top(img, tiles, clip, k):
    """The k-th largest pixel as it can be told from tile histograms CLAMPED to `clip` (csrc/clahe.hip, hist_rank_top_job), or None
    where it cannot and the stage has to select over the image.  On a grid that divides the image: always, for k <= clip.  With a
    reflected border the clamped counts hold border pixels too; they are taken out again, the walk from the top settles on the first
    64-bin run, then bin, whose running count reaches k, and the answer stands only if the clamped count above that bin, border
    included, is below clip (then nothing up there was clamped)."""
    assert 1 <= k <= clip
    with_b = np.minimum(tile_hists(img, tiles), clip).sum(axis=0)[::-1]                  # from the top bin down
    border_b = (np.bincount(padded(img, tiles).ravel(), minlength=HIST) - np.bincount(img.ravel(), minlength=HIST))[::-1]
    local_b = with_b - border_b
    with_c, local_c = with_b.reshape(1024, 64).sum(axis=1), local_b.reshape(1024, 64).sum(axis=1)
    incl = np.cumsum(local_c)
    hit = np.flatnonzero((incl - local_c < k) & (k <= incl))
    if hit.size == 0:
        return None
    c = int(hit[0])
    above, above_with = int(incl[c] - local_c[c]), int(np.cumsum(with_c)[c] - with_c[c])
    lb, wb = local_b[c * 64:(c + 1) * 64], with_b[c * 64:(c + 1) * 64]
    inc2 = np.cumsum(lb)
    mine = np.flatnonzero((above + inc2 - lb < k) & (k <= above + inc2))
    if mine.size == 0:
        return None
    lane = int(mine[0])
    if border_b.any() and not above_with + int(np.cumsum(wb)[lane] - wb[lane]) < clip:
        return None
    return HIST - 1 - (c * 64 + lane)


def falls_back(img, tiles, clip):
    """Whether the stage must select over this image: one of np.percentile(img, 99.9999)'s two order statistics cannot be served."""
    return any(served_from_top(img, tiles, clip, k) is None for k in k_tops(img.size))


# ---- value extremes ------------------------------------------------------------------------------------------------------------
def full_noise(h, w, seed):
    """Uniform noise in which every one of the 65536 values occurs."""
    assert h * w >= HIST
    rng = np.random.default_rng(seed)
    v = np.concatenate([np.arange(HIST), rng.integers(0, HIST, h * w - HIST)])
    return rng.permutation(v).astype(np.uint16).reshape(h, w)


def binary(h, w, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 65535).astype(np.uint16)


def staircase(h, w, tiles, seed):
    """16 levels in a 4 x 4 arrangement whose steps lie on the padded image's tile borders (tiles 2: every second step; tiles 4:
    every step), 256 values wide each: tiles that touch have no value in common."""
    assert 4 % tiles == 0
    he, we, _, _ = grid(h, w, tiles)
    yy, xx = np.mgrid[0:h, 0:w]
    level = (yy * 4 // he) * 4 + xx * 4 // we
    return (2048 + 4000 * level + np.random.default_rng(seed).integers(0, 256, (h, w))).astype(np.uint16)


def byte_edges(h, w, seed):
    """Only multiples of 256 and multiples of 256 less one."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 256, (h, w)) * 256 - rng.integers(0, 2, (h, w))).astype(np.uint16)


def constant(h, w, value=30000):
    return np.full((h, w), value, dtype=np.uint16)


# ---- the case table ------------------------------------------------------------------------------------------------------------
A, A1 = (200, 304), (201, 305)
B, B1, B2, B3 = (520, 528), (521, 528), (520, 529), (521, 529)
C = (1000, 1048)
KNOBS = ('SHG_CLAHE_SAT', 'SHG_CLAHE_SAT_PX', 'SHG_SELECT_WINDOW', 'SHG_CONTRAST_BATCH', 'SHG_INTERP_SHAPE', 'SHG_FUSE_SCALE')
ROUTES = {0: 'atomics8', 1: 'atomics16', 2: 'u16', 3: 'byte', 4: 'nibble'}


def pitch_of(w):
    return (w + 63) // 64 * 64


def discs(h, w):
    """none, inside, covering the image, off it, a single pixel's radius."""
    return {'none': None, 'inside': (w // 2, h // 2, int(0.3 * h)), 'cover': (w // 2, h // 2, h + w), 'off': (-400, h // 2, 90), 'r1': (w - 1, 0, 1)}


CASES = []


def case(id, shape, k, clip, kind, tiles=2, trans=False, crop=None, disc='inside', keep=False, env=None, expect=None, fallback=None,
         fails=False, seed=0, **facts):
    """clip: pixels a bin on the tiles of the image CLAHE sees (None: clip limit 0).  kind: (builder name, arguments...).  expect: what
    the plan must say.  fallback: how many disks select their frame percentile over the image (None: not claimed).  facts: what the
    CPU test checks of the images."""
    h, w = shape
    out_w = crop[0] if crop else w
    _, _, th, tw = grid(h, out_w, tiles)
    CASES.append(dict(id=id, shape=shape, k=k, tiles=tiles, clip=clip, clip_limit=clip_limit_for(clip, th * tw) if clip else 0.0, kind=kind,
                      trans=trans, crop=crop, disc=discs(h, out_w)[disc], keep=keep, env=dict(env or {}), expect=dict(expect or {}),
                      fallback=fallback, fails=fails, seed=seed, out_w=out_w, area=th * tw, facts=facts))
    assert set(CASES[-1]['env']) <= set(KNOBS)


def frames_of(c):
    """The k images of a case, built afresh (deterministic)."""
    (h, w), k, name, args, seed = c['shape'], c['k'], c['kind'][0], c['kind'][1:], c['seed']
    if name == 'solar':
        return [solar(h, w, 100 + seed + i, flat_top=bool(args and args[0]) and i % 2 == 0) for i in range(k)]
    if name == 'planted':
        target, layout = args
        return [planted(h, w, c['tiles'], c['clip'], target, layout, seed + i) for i in range(k)]
    if name == 'top':                                    # every second disk has the planted top, the others are plain
        count, place, second = args
        return [top_image(h, w, seed + i, count, place, second) if i % 2 == 0 else np.minimum(solar(h, w, seed + i), 60000).astype(np.uint16)
                for i in range(k)]
    if name == 'levels':                                 # a stack of different brightness
        return [solar(h, w, 100 + seed + i, sky=sky, gain=gain) for i, (sky, gain) in enumerate(args[0])]
    one = {'noise': lambda i: full_noise(h, w, seed + i), 'binary': lambda i: binary(h, w, seed + i),
           'stairs': lambda i: staircase(h, w, c['tiles'], seed + i), 'bytes': lambda i: byte_edges(h, w, seed + i),
           'const': lambda i: constant(h, w), 'zero': lambda i: constant(h, w, 0)}
    if name in one:
        return [one[name](i) for i in range(k)]
    if name == 'one_bad':                                # good disks with a failing one among them
        return [(constant(h, w) if args[0] == 'const' else constant(h, w, 0)) if i == 1 else solar(h, w, 100 + seed + i) for i in range(k)]
    raise ValueError(name)


def transversalium_of(h, w):
    """(circle, borders, window) as the existing fused test passes them."""
    return (w / 2.0, h / 2.0, 0.4 * h), [0.0, 0.05 * h, w - 1.0, 0.95 * h], min(61, (int(0.8 * h) // 2) * 2 - 1)


def _table():
    batched = dict(batched=1)
    # -- counters and disk counts, on the solar family
    case('u16-ktop-A-k2', A, 2, 1, ('solar',), expect=dict(batched, route='u16', slices=1, from_top=0, blend_px=4, window=0, lut_all=0))
    case('nibble2-B-k1', B, 1, 2, ('solar',), disc='none', expect=dict(batched, route='nibble', from_top=1, several_slices=1))
    case('nibble15-B3-k2-trans', B3, 2, 15, ('solar',), trans=True, disc='cover', expect=dict(batched, route='nibble', from_top=1))
    case('byte16-B-k4', B, 4, 16, ('solar', True), disc='off', expect=dict(batched, route='byte', from_top=1, blend_px=8, window=1, lut_all=0))
    case('byte255-B1-k5', B1, 5, 255, ('solar',), disc='r1', expect=dict(batched, route='byte', from_top=1, blend_px=8, window=1), fallback=0)
    case('byte-forced-A-k2', A, 2, 2, ('solar',), env={'SHG_CLAHE_SAT': '8'}, expect=dict(batched, route='byte', from_top=1))
    case('u16-clip256-B-k2', B, 2, 256, ('solar',), expect=dict(batched, route='u16', several_slices=1, from_top=0, big=0))
    case('u16-clip256-B2-k4-big', B2, 4, 256, ('solar',), disc='none', expect=dict(batched, route='u16', several_slices=1, big=1, blend_px=8))
    case('u16-sat0-B-k2', B, 2, 8, ('solar',), env={'SHG_CLAHE_SAT': '0'}, expect=dict(batched, route='u16', from_top=0))
    case('noclip-A-k2', A, 2, None, ('solar',), expect=dict(batched=0, route='atomics16'))
    case('noclip-B3-k1-keep', B3, 1, None, ('solar',), trans=True, keep=True, disc='cover', expect=dict(batched=0, route='atomics16'))
    case('nibble-A1-k8-lutall', A1, 8, 2, ('solar',), disc='r1', expect=dict(batched, route='nibble', lut_all=1, blend_px=8, window=1), fallback=0)
    case('u16-A-k8-lutall', A, 8, 1, ('solar',), disc='off', expect=dict(batched, route='u16', lut_all=1, window=1))
    case('byte-B-k2-unbatched', B, 2, 20, ('solar',), env={'SHG_CONTRAST_BATCH': '0'}, expect=dict(batched=0, route='u16', from_top=0))
    case('nibble-A-k5-4px', A, 5, 2, ('solar',), env={'SHG_INTERP_SHAPE': '34'}, expect=dict(batched, route='nibble', blend_px=4, window=1))
    case('nibble-A-k2-8px', A, 2, 2, ('solar',), env={'SHG_INTERP_SHAPE': str(2 | 2 << 4 | 1 << 8)}, expect=dict(batched, route='nibble', blend_px=8, window=0))
    case('nibble-A-k1-window', A, 1, 2, ('solar',), env={'SHG_SELECT_WINDOW': '1'}, expect=dict(batched, route='nibble', window=1))
    case('byte-B-k4-nowindow', B, 4, 20, ('solar',), env={'SHG_SELECT_WINDOW': '0'}, expect=dict(batched, route='byte', window=0, blend_px=8))
    # -- slices and chunks, on planted histograms: one per row (slices below clip), clamps between the chunks of one long slice
    case('byte-short-B-k2-rows5', B, 2, 255, ('planted', 5, 'rows'), env={'SHG_CLAHE_SAT_PX': '5000'}, disc='none',
         expect=dict(batched, route='byte', several_slices=1), slices_below_clip=True)
    case('nibble-short-B-k2-rows245', B, 2, 15, ('planted', 245, 'rows'), env={'SHG_CLAHE_SAT_PX': '5000'}, expect=dict(batched, route='nibble', several_slices=1))
    case('byte-chunks-B-k2-rows32768', B, 2, 100, ('planted', 32768, 'rows'), env={'SHG_CLAHE_SAT_PX': '70000'}, disc='off',
         expect=dict(batched, route='byte', slices=1, several_chunks=1))
    case('nibble-chunks-B3-k1-mirror32769', B3, 1, 15, ('planted', 32769, 'mirror'), env={'SHG_CLAHE_SAT_PX': '70000'}, disc='r1',
         expect=dict(batched, route='nibble', slices=1, several_chunks=1))
    # -- every target, the layouts and the counters in turn (a Latin square); 'mirror' on the size the grid does not divide
    counters = (('nibble', 2), ('byte', 16), ('u16', 256))
    for i, target in enumerate(TARGETS):
        layout = LAYOUTS[i % 3]
        route, clip = counters[(i + i // 3) % 3]
        shape, name = (B3, 'B3') if layout == 'mirror' else (B, 'B')
        if layout == 'mirror' and clip < 4:
            clip = 4                                     # (the corner pixel of the mirrored row and column counts four times)
        case('%s%d-%s-k%d-%s%d' % (route, clip, name, 1 + i % 2, layout, target), shape, 1 + i % 2, clip, ('planted', target, layout),
             disc=('none', 'inside', 'cover', 'off', 'r1')[i % 5], expect=dict(batched, route=route))
    case('u16-A-k2-band1', A, 2, 1, ('planted', 1, 'band'), expect=dict(batched, route='u16', slices=1))         # a count of exactly clip + 1 = 2
    case('nibble4-A1-k1-mirror2', A1, 1, 4, ('planted', 2, 'mirror'), disc='none', expect=dict(batched, route='nibble'))
    # -- image formation: fused or not, with and without row factors, the crops; -- tile grids 1 to 4, dividing or not
    left, right, odd = (352, 0, 48, 304), (352, 0, 0, 304), (299, 3, 0, 299)
    case('fused-trans-A-k2', A, 2, 2, ('solar',), trans=True, expect=dict(batched, fused=1, route='nibble'))
    case('fused-plain-left-A-k2', A, 2, 2, ('solar',), crop=left, disc='none', expect=dict(batched, fused=1, route='nibble'))
    case('fused-trans-right-A-k1', A, 1, 2, ('solar',), trans=True, crop=right, disc='cover', expect=dict(batched, fused=1, route='nibble'))
    case('fused-plain-odd-A-k2', A, 2, 2, ('solar',), crop=odd, disc='off', expect=dict(batched, fused=1, route='nibble'))
    case('fused-trans-odd-A1-k4', A1, 4, 2, ('solar',), trans=True, crop=(303, 0, 1, 302), disc='r1', expect=dict(batched, fused=1, route='nibble'))
    case('kept-trans-left-A-k2', A, 2, 2, ('solar',), trans=True, crop=left, keep=True, expect=dict(batched, fused=0, route='nibble'))
    case('kept-trans-odd-A-k1', A, 1, 2, ('solar',), trans=True, crop=odd, keep=True, disc='none', expect=dict(batched=0, fused=0, route='u16'))
    case('kept-trans-B3-k2', B3, 2, 8, ('solar',), trans=True, keep=True, disc='cover', expect=dict(batched, fused=0, route='nibble'))
    case('unfused-plain-A-k2', A, 2, 2, ('solar',), env={'SHG_FUSE_SCALE': '0'}, disc='off', expect=dict(batched, fused=0, route='nibble'))
    case('unfused-plain-right-A1-k1', A1, 1, 2, ('solar',), crop=(353, 0, 0, 305), env={'SHG_FUSE_SCALE': '0'}, disc='r1', expect=dict(batched=0, fused=0, route='u16'))
    case('unfused-trans-left-A-k2', A, 2, 2, ('solar',), trans=True, crop=left, env={'SHG_FUSE_SCALE': '0'}, expect=dict(batched, fused=0, route='nibble'))
    case('tiles1-A-k2', A, 2, 3, ('solar',), tiles=1, disc='none', expect=dict(batched, route='nibble'))
    case('tiles1-B3-k1', B3, 1, 40, ('solar',), tiles=1, trans=True, expect=dict(batched, route='byte'))
    case('tiles2-B1-k2-h', B1, 2, 8, ('solar',), disc='cover', expect=dict(batched, route='nibble'))
    case('tiles2-B2-k2-w', B2, 2, 8, ('solar',), disc='off', expect=dict(batched, route='nibble'))
    case('tiles3-A1-k2-divides', A1, 2, 2, ('solar',), tiles=3, crop=(306, 0, 0, 305), disc='r1', expect=dict(batched, route='nibble'))
    case('tiles3-B-k2-h', B, 2, 4, ('solar',), tiles=3, expect=dict(batched, route='nibble'))
    case('tiles3-A1-k1-w', A1, 1, 2, ('solar',), tiles=3, trans=True, disc='none', expect=dict(batched, route='nibble'))
    case('tiles3-B2-k2-both', B2, 2, 20, ('solar',), tiles=3, disc='cover', expect=dict(batched, route='byte'))
    case('tiles4-A-k2-divides', A, 2, 2, ('solar',), tiles=4, disc='off', expect=dict(batched, route='nibble'))
    case('tiles4-B1-k2-h', B1, 2, 2, ('solar',), tiles=4, trans=True, disc='r1', expect=dict(batched, route='nibble'))
    case('tiles4-B2-k1-w', B2, 1, 3, ('solar',), tiles=4, expect=dict(batched, route='nibble'))
    case('tiles4-A1-k5-both', A1, 5, 2, ('solar',), tiles=4, disc='none', expect=dict(batched, route='nibble', blend_px=8))
    # -- the top of the histogram: the frame percentile from the k-th largest, and the fall-back select
    case('top-B-k1-below-adjacent', B, 1, 8, ('top', 1, 'scatter', (TOP - 1, 3)), expect=dict(batched, route='nibble', from_top=1), fallback=0, top='adjacent')
    case('top-B-k3-ktop-onebin', B, 3, 8, ('top', 2, 'scatter', None), expect=dict(batched, route='nibble', from_top=1), fallback=0, top='one')
    case('top-B-k2-clip', B, 2, 8, ('top', 8, 'scatter', None), disc='none', expect=dict(batched, route='nibble', from_top=1), fallback=0, top='one')
    case('top-B-k1-clip+1', B, 1, 20, ('top', 21, 'scatter', None), disc='cover', expect=dict(batched, route='byte', from_top=1), fallback=0, top='one')
    # (a burnt-out core is served even beside a border: every tile's top bin is clamped, 4 x 20 less the dozen border pixels still reaches k)
    case('top-B3-k3-burnt', B3, 3, 20, ('top', 3000, 'scatter', None), disc='off', expect=dict(batched, route='byte', from_top=1), fallback=0, top='one')
    case('top-B3-k1-row-clip', B3, 1, 8, ('top', 8, 'mirror_row', None), disc='r1', expect=dict(batched, route='nibble', from_top=1), fallback=1, top='one')
    case('top-B3-k3-row-clip+1', B3, 3, 20, ('top', 21, 'mirror_row', None), expect=dict(batched, route='byte', from_top=1), fallback=2, top='one')
    case('top-B3-k1-col-clip+1', B3, 1, 8, ('top', 9, 'mirror_col', None), disc='none', expect=dict(batched, route='nibble', from_top=1), fallback=1, top='one')
    case('top-B1-k2-row-ktop', B1, 2, 8, ('top', 2, 'mirror_row', None), disc='cover', expect=dict(batched, route='nibble', from_top=1), fallback=0, top='one')
    case('top-B2-k1-col-below', B2, 1, 8, ('top', 1, 'mirror_col', (TOP - 1, 2)), disc='off', expect=dict(batched, route='nibble', from_top=1), fallback=0, top='adjacent')
    case('top-C-k1-ktop3', C, 1, 3, ('top', 3, 'scatter', None), disc='r1', expect=dict(batched, route='nibble', from_top=1, ktop=3), fallback=0, top='one')
    # -- value extremes
    case('noise-B-k1-clip1', B, 1, 1, ('noise',), expect=dict(batched, route='u16'), all_bins=True)
    case('noise-B3-k2-clip2', B3, 2, 2, ('noise',), disc='none', expect=dict(batched, route='nibble'), all_bins=True)
    case('binary-B-k2', B, 2, 16, ('binary',), disc='cover', expect=dict(batched, route='byte'), values=(0, 65535))
    case('binary-A1-k1', A1, 1, 1, ('binary',), disc='off', expect=dict(batched, route='u16'), values=(0, 65535))
    case('stairs-A-k2-tiles4', A, 2, 2, ('stairs',), tiles=4, disc='r1', expect=dict(batched, route='nibble'), disjoint=True)
    case('stairs-B3-k1-tiles2', B3, 1, 8, ('stairs',), expect=dict(batched, route='nibble'), disjoint=True)
    case('bytes-B-k4', B, 4, 15, ('bytes',), disc='none', expect=dict(batched, route='nibble', window=1), byte_edges=True)
    case('bytes-A1-k1-window', A1, 1, 2, ('bytes',), env={'SHG_SELECT_WINDOW': '1'}, disc='cover', expect=dict(batched, route='nibble', window=1), byte_edges=True)
    # -- stages that must fail alike
    case('fails-const-B-k1', B, 1, 8, ('const',), fails=True)
    case('fails-zero-A-k1', A, 1, 2, ('zero',), fails=True)
    case('fails-const-in-stack-A-k3', A, 3, 2, ('one_bad', 'const'), fails=True)
    case('fails-zero-in-stack-B3-k2-unbatched', B3, 2, None, ('one_bad', 'zero'), fails=True)


_table()
IDS = [c['id'] for c in CASES]

# One workspace, call after call (the percentile window's carried state): the same image twice, a much brighter one, a much darker
# one, back, then a stack of mixed levels, then the single image again.  (sky, gain) per disk.
SERIES_SHAPE, SERIES_CLIP = B, 8
SERIES = [[(0.01, 1.0)], [(0.01, 1.0)], [(0.30, 1.0)], [(0.001, 0.2)], [(0.01, 1.0)], [(0.01, 1.0), (0.25, 0.9), (0.002, 0.3), (0.05, 0.6)], [(0.01, 1.0)]]


def series_frames(step):
    h, w = SERIES_SHAPE
    return [solar(h, w, 1 if (sky, gain) == (0.01, 1.0) else 10 * step + i, sky=sky, gain=gain) for i, (sky, gain) in enumerate(SERIES[step])]


# The planted combinations no tile can hold, for the record (the CPU test holds the list to what planted() refuses).
def planted_table():
    """-> [(shape, tiles, clip, target, layout, 'ok' | why not)] over the shapes and clips the planted cases use."""
    rows = []
    for shape, clip in ((A, 1), (A1, 4), (B, 2), (B, 16), (B, 256), (B3, 4), (B3, 16), (B3, 256)):
        for target in TARGETS:
            for layout in LAYOUTS:
                if layout == 'mirror' and shape in (A, B):
                    continue
                try:
                    planted(shape[0], shape[1], 2, clip, target, layout)
                    rows.append((shape, 2, clip, target, layout, 'ok'))
                except Infeasible as e:
                    rows.append((shape, 2, clip, target, layout, str(e)))
    return rows
