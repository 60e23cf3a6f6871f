"""NumPy restatement of shg_derotate_u16 and of derotate.py's host steps, written from the arithmetic include/shg_hip.h and the
docstrings state, not from the kernel: every per-pixel step on whole arrays in float64, one NumPy operation an IEEE operation (NumPy
fuses nothing), np.sqrt and / correctly rounded, the integers in int64.  Also the scene the accuracy is measured on -- spots fixed
to a differentially rotating sphere under a limb darkening fixed to the view, supersampled, at any epoch --, the measures and the
bounds (TOLERANCE)."""
import math

import numpy as np

from tests import flatten_ref as fr

S = (None, None, None, -0.16666666666666666, None, 0.008333333333333333, None, -0.0001984126984126984, None, 2.7557319223985893e-06, None,
     -2.505210838544172e-08, None, 1.6059043836821613e-10, None, -7.647163731819816e-13)
C = (None, None, -0.5, None, 0.041666666666666664, None, -0.001388888888888889, None, 2.48015873015873e-05, None, -2.755731922398589e-07,
     None, 2.08767569878681e-09, None, -1.1470745597729725e-11, None, 4.779477332387385e-14)


def coefficients_are_the_nearest_doubles():
    """The header's sixteen constants are the float64 nearest to +-1 / k! (Fraction -> float rounds correctly)."""
    from fractions import Fraction
    for k in range(2, 17):
        want = float(Fraction(-1 if (k // 2) % 2 else 1, math.factorial(k)))
        if (S if k % 2 else C)[k] != want:
            return False
    return True


def sin_cos(a):
    """(a P(a2), Q(a2)): the header's two Horner forms."""
    a2 = a * a
    p = np.full_like(a, S[15])
    for k in (13, 11, 9, 7, 5, 3):
        p = p * a2 + S[k]
    p = p * a2 + 1.0
    q = np.full_like(a, C[16])
    for k in (14, 12, 10, 8, 6, 4, 2):
        q = q * a2 + C[k]
    q = q * a2 + 1.0
    return a * p, q


def keys_q14(t):
    """The four Q14 Keys weights of the fractions t -> int64 [..., 4]."""
    tt = t * t
    k = np.stack([((-0.5 * t + 1.0) * t - 0.5) * t, (1.5 * t - 2.5) * tt + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, (0.5 * t - 0.5) * tt], axis=-1)
    q = np.rint(k * 16384.0).astype(np.int64)
    q[..., 1] += 16384 - q.sum(axis=-1)
    return q


def table_at(table, rho):
    """shg_ring_flatten_u16's rule on the table at the radii rho."""
    kk = table.shape[0]
    u = rho - 0.5
    j = np.clip(np.trunc(u), 0, max(kk - 2, 0)).astype(np.int64)
    g0, g1 = table[j], table[np.minimum(j + 1, kk - 1)]
    g = g0 + (g1 - g0) * (u - j.astype(np.float64))
    return np.where(u <= 0.0, table[0], np.where(u >= np.float64(kk - 1), table[kk - 1], g))


def derotate(img, circle, matrix, rate3, clv=None, parts=False):
    """shg_derotate_u16 -> out uint16 [h, w]; parts: also {'moved' (the pixels resampled), 'behind' (on the disk, a != 0, source behind
    the limb), 'a' (the angle where on the disk), 'shift' (the displacement in px where moved)}."""
    img = np.asarray(img, dtype=np.uint16)
    h, w = img.shape
    cx, cy, rad = (np.float64(v) for v in circle)
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
    k0, k1, k2 = (np.float64(v) for v in rate3)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = np.broadcast_to(((np.arange(w, dtype=np.float64) - cx) / rad)[None, :], (h, w))
        v = np.broadcast_to(((cy - np.arange(h, dtype=np.float64)) / rad)[:, None], (h, w))
        d2 = u * u + v * v
        on = d2 < 1.0
        u, v, d2 = np.where(on, u, 0.0), np.where(on, v, 0.0), np.where(on, d2, 0.0)
    z = np.sqrt(1.0 - d2)
    qx, qy, qz = ((m[i, 0] * u + m[i, 1] * v) + m[i, 2] * z for i in range(3))
    s2 = qy * qy
    a = (k2 * s2 + k1) * s2 + k0
    sa, ca = sin_cos(a)
    sx, sz, sy = qx * ca - qz * sa, qx * sa + qz * ca, qy
    pu, pv, pz = ((m[0, i] * sx + m[1, i] * sy) + m[2, i] * sz for i in range(3))
    turned = on & (a != 0.0)
    moved = turned & (pz > 0.0)
    x, y = cx + pu * rad, cy - pv * rad
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = keys_q14(x - x0), keys_q14(y - y0)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    wide = img.astype(np.int64)
    total = np.zeros((h, w), np.int64)
    for j in range(4):
        rows = np.clip(y0 + (j - 1), 0, h - 1)
        acc = np.zeros((h, w), np.int64)
        for k in range(4):
            acc = acc + wx[..., k] * wide[rows, np.clip(x0 + (k - 1), 0, w - 1)]
        total = total + wy[..., j] * acc
    val = (total + (1 << 27)) >> 28
    if clv is None:
        new = np.clip(val, 0, 65535)
    else:
        table = np.asarray(clv, dtype=np.float64)
        assert table.shape == (fr.n_rings(circle),) and (table > 0).all() and np.isfinite(table).all()
        g_out = table_at(table, np.sqrt(d2) * rad)
        g_src = table_at(table, np.sqrt(pu * pu + pv * pv) * rad)
        new = np.clip(np.rint(val.astype(np.float64) * (g_out / g_src)), 0.0, 65535.0)
    out = np.where(moved, new, img).astype(np.uint16)
    if not parts:
        return out
    shift = np.where(moved, np.sqrt((x - (cx + u * rad)) ** 2 + (y - (cy - v * rad)) ** 2), 0.0)
    return out, {'moved': moved, 'behind': turned & ~moved, 'a': np.where(on, a, 0.0), 'shift': shift}


# ---- the host steps ----
def orientation(north_deg, b0_deg, mirror=False):
    """M = T(b0) F R(north), the three factors multiplied out by hand: north is the angle in the image as given, mirrored or not."""
    p, b = math.radians(north_deg), math.radians(b0_deg)
    f = -1.0 if mirror else 1.0
    cp, sp, cb, sb = math.cos(p), math.sin(p), math.cos(b), math.sin(b)
    return np.array([[f * cp, f * sp, 0.0], [-cb * sp, cb * cp, sb], [sb * sp, -sb * cp, cb]])


def rates(dt_days, law=(14.71 - 0.9856, -2.39, -1.78)):
    """(k0, k1, k2): the law in degrees a day as seen, in radians, times the days."""
    return tuple(math.radians(v) * dt_days for v in law)


def measured_clv(img, circle, smooth=1):
    """derotate.measured_clv on the restatement of the ring medians."""
    from solex_ser_recon_en_amd import flatten
    return np.maximum(flatten.filled_profile(fr.profile_of(*fr.ring_medians(img, circle)), smooth), 1.0)


# ---- the scene ----
SCENE = {'h': 250, 'w': 260, 'circle': (131.3, 122.6, 100.4), 'north': 17.0, 'b0': -5.2, 'level': 40000.0, 'sky': 300.0, 'spots': 12,
         'law': (14.71 - 0.9856, -2.39, -1.78)}


def spots(count=SCENE['spots'], seed=5):
    """(latitude, longitude at epoch 0, angular radius, depth) of every spot, radians: within 40 degrees of the equator, spread over
    the visible hemisphere's middle, none within 0.2 rad of the disk's centre at epoch 0."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        lat, lon = rng.uniform(-0.7, 0.7), rng.uniform(-0.9, 0.9)
        if math.hypot(lat - math.radians(SCENE['b0']), lon) < 0.2:
            continue
        out.append((lat, lon, rng.uniform(0.025, 0.05), rng.uniform(0.2, 0.6)))
    return out


def scene(dt_days=0.0, circle=None, north=None, b0=None, mirror=False, shape=None, sub=3, with_spots=True, parts=False):
    """The scene at the epoch dt_days as uint16 [h, w]: level * (0.4 + 0.6 mu) on the disk, mu the cosine of the angle to the observer
    (fixed to the view), times 1 - depth exp(-d^2 / 2 s^2) for every spot, d the angle on the sphere to the spot's centre, which sits
    at its latitude and at longitude0 + rate(latitude of the POINT) * dt -- the pattern is carried along by the differential rotation
    of every point, sheared as the Sun shears it; sky outside; the mean of sub x sub samples a pixel.  parts: also the share of every
    pixel's samples that a spot darkens by more than 1 %."""
    circle = SCENE['circle'] if circle is None else circle
    h, w = (SCENE['h'], SCENE['w']) if shape is None else shape
    m = orientation(SCENE['north'] if north is None else north, SCENE['b0'] if b0 is None else b0, mirror)
    cx, cy, rad = circle
    k = rates(dt_days, SCENE['law'])
    off = (np.arange(sub, dtype=np.float64) + 0.5) / sub - 0.5
    xs = (np.arange(w, dtype=np.float64)[:, None] + off[None, :]).reshape(-1)
    ys = (np.arange(h, dtype=np.float64)[:, None] + off[None, :]).reshape(-1)
    u, v = ((xs - cx) / rad)[None, :], ((cy - ys) / rad)[:, None]
    d2 = u * u + v * v
    on = d2 < 1.0
    z = np.sqrt(np.where(on, 1.0 - d2, 0.0))
    q = [m[i, 0] * u + m[i, 1] * v + m[i, 2] * z for i in range(3)]
    lat = np.arcsin(np.clip(q[1], -1.0, 1.0))
    s2 = q[1] * q[1]
    lon0 = np.arctan2(q[0], q[2]) - ((k[2] * s2 + k[1]) * s2 + k[0])          # where the point was at epoch 0
    value = SCENE['level'] * (0.4 + 0.6 * z)
    dark = np.zeros(d2.shape, bool)
    if with_spots:
        for s_lat, s_lon, s_rad, depth in spots():
            cosd = np.sin(lat) * math.sin(s_lat) + np.cos(lat) * math.cos(s_lat) * np.cos(lon0 - s_lon)
            d = np.arccos(np.clip(cosd, -1.0, 1.0))
            factor = 1.0 - depth * np.exp(-0.5 * (d / s_rad) ** 2)
            value = value * factor
            dark |= factor < 0.99
    value = np.where(on, value, SCENE['sky'])
    img = np.clip(np.rint(value.reshape(h, sub, w, sub).mean(axis=(1, 3))), 0, 65535).astype(np.uint16)
    if parts:
        return img, (dark & on).reshape(h, sub, w, sub).mean(axis=(1, 3))
    return img


def inner(shape, circle, fraction=0.9):
    return fr.rings(shape[0], shape[1], (circle[0], circle[1], fraction * circle[2]))[0]


def rms(a, b, mask):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d[mask] ** 2)))


def spot_share_of_rings(dt_days=0.0):
    """The largest share of a ring's pixels that a spot touches, over the rings of the scene's disk."""
    img, dark = scene(dt_days, parts=True)
    on, ring, _ = fr.rings(img.shape[0], img.shape[1], SCENE['circle'])
    kk = fr.n_rings(SCENE['circle'])
    touched = np.bincount(ring[on], weights=(dark[on] > 0).astype(np.float64), minlength=kk)
    return float((touched / np.maximum(np.bincount(ring[on], minlength=kk), 1)).max())


def accuracy(hours, derotate_fn=None):
    """The scene at epoch 0 carried to `hours` later, against the scene rendered at that epoch: the rms difference in counts over the
    inner 0.9 R -> {'before' (nothing done), 'geometry' (clv None), 'measured' (the ring medians' profile), 'round_trip' (there and
    back with the measured profile, against the scene at epoch 0), 'behind' (pixels whose source lies behind the limb)}.
    derotate_fn(img, circle, matrix, rate3, clv) -> image: the restatement by default."""
    run = derotate if derotate_fn is None else derotate_fn
    circle = SCENE['circle']
    m = orientation(SCENE['north'], SCENE['b0'])
    first, then = scene(0.0), scene(hours / 24.0)
    mask = inner(first.shape, circle)
    k = rates(hours / 24.0, SCENE['law'])
    back = tuple(-v for v in k)
    table = measured_clv(first, circle)
    there = run(first, circle, m, k, table)
    again = run(there, circle, m, back, measured_clv(there, circle))
    return {'before': rms(first, then, mask), 'geometry': rms(run(first, circle, m, k, None), then, mask), 'measured': rms(there, then, mask),
            'round_trip': rms(again, first, mask), 'behind': int(derotate(first, circle, m, k, None, parts=True)[1]['behind'].sum())}


# Measured on the scene (counts rms over the inner 0.9 R of a disk of 40000 counts at its centre), the restatement on the CPU:
#   1 h: before 301.84, geometry only 102.60, measured profile 2.854, there and back 3.448; 1 pixel from behind the limb
#   6 h: before 1578.32, geometry only 615.94, measured profile 6.531, there and back 4.314; 32 pixels from behind the limb
# The bounds are the measured values plus a quarter, rounded up to two digits (DESIGN.md section 17's rule).
TOLERANCE = {1.0: {'geometry': 130.0, 'measured': 3.6, 'round_trip': 4.4},
             6.0: {'geometry': 770.0, 'measured': 8.2, 'round_trip': 5.4}}
