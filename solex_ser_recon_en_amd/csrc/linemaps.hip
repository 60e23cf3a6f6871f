// Line maps: where the line core sits (the Dopplergram, shg_line_core_shift), five planes of the line's profile (shg_line_profile:
// the core's position, its intensity, the line's width (FWHM), its centre of gravity and its equivalent width within the window) and
// the line's bisector and chord at K levels (shg_line_bisector) in every (slit row, frame) of a scan, and those raw maps taken to the
// products' geometry (shg_doppler_finish, shg_line_profile_finish, shg_line_bisector_finish).  Not a reference stage: the arithmetic
// is the one include/shg_hip.h states and tests/linemaps_ref.py restates in NumPy, bit for bit.
// The three maps share one core: the window, walk 1 and the vertex (core_d_of, level_of, thr_of), one walk-2 crossing state and
// interpolation (Cross, crossings: the profile's width is the chord at half), one argument struct (MapArgs), the band walk, the
// write-out of an LDS phase tile (write_tile), the plain kernels' prologue (plain_row), one launch and one set of checks.
//
// Rotated files (the usual layout): the samples of one wavelength column are one contiguous raw row across the slit, so a lane owns
// eight consecutive raw columns (eight slit rows), loads them as ONE 16-byte piece (8 bytes for 8-bit files) per raw row, and a
// wave's 64 lanes read 1 KiB of the row at once.  A walk covers the band [min lo, max hi] of the wave's 512 slit rows row by row
// (wave-uniform j: every load instruction covers one contiguous stretch), eight rows in flight; a lane skips the rows outside its
// own eight windows.  Each slit row keeps a streaming state, so nothing but the band is read.
// k_line_core_rot: one walk with the vertex state (minimum, its position, the samples either side).  A workgroup (eight waves, two
// frames each) does 16 frames of the same 512 rows and writes the map through LDS: 16 consecutive columns (64 bytes) of a row at a
// time instead of one scattered float per row and frame.  Measured (rocprofv3, MI355X, H = 5): 37.8 us at C2 (2000 x 2000x200,
// 16-bit: 0.56 of 8 TB/s on the band's bytes), 88.8 us at C5's frame shape (0.75); four waves of four frames each gave 43.1 / 96.3 us
// (too few waves in flight at C2: 2000 for 1024 SIMDs).
// k_line_profile_rot: walk 1 carries the vertex state, Σp, Σ(j - lo)p and p(lo) + p(hi); after it the half level is known, and
// walk 2 reads the same band again for the half-level crossings.  The wave has just read those rows (about 1 KiB per band row), so
// walk 2 is served on-die (L2, else the Infinity Cache): the profile samples do not fit in LDS at 8 waves (512 rows x up to 65
// samples x 2 B per wave) nor in registers.  A workgroup is eight waves x two phases of eight frames (16 frames of the same 512
// rows); each phase leaves through an LDS tile [5][8][512] as 32-byte runs of map rows, the two phases completing 64-byte runs in
// the same L2.  No atomics.
// k_line_core_plain, k_line_profile_plain (un-rotated files): a wave is one slit row of 64 frames, the window wave-uniform, each lane
// walks its window (twice for the profile), the stores coalesced.
// k_line_bisector_rot (shg_line_bisector, K <= 8 levels): the profile's shape and walk 1, of which it reads the vertex and C2.  Walk 2
// for K levels at once would hold 8 rows x K levels x (jl, jr, two packed sample pairs, the level's threshold) = 40 K registers, and
// an output tile [2K][8][512] floats is 256 KiB at K = 8.  So the levels go in passes of kLevelsPerPass = 2: each pass walks the band
// again (served on-die, as the profile's walk 2) for two levels, with 8 rows x 2 levels x 5 = 80 registers of crossing state (the
// sample pairs packed as the profile's, the crossings interpolated once, after the walk), and leaves through a [4][8][512] tile
// (64 KiB).  A level's decisions stay its own: its planes do not depend on the other levels requested.  The kernel keeps 252-255 VGPRs
// without spills (two waves per SIMD, one workgroup per CU, as the profile's 190); four waves per SIMD would spill about 400
// registers, and passes of four levels would not fit 256.  k_line_bisector_plain: the profile's plain kernel, one walk of the
// lane's window per level.
// k_map_finish<1> (the Dopplergram's), k_map_finish<5> (the profile's), k_map_finish<2K, K> (the bisectors'): the ellipse -> circle
// resample of k_warp_rows with NaN for taps outside, the limb mask, the crop / pad of crop_plan, and the 16-bit display planes; one
// thread per output pixel, all planes of it.
// Emission maps (shg_line_emission, shg_line_emission_finish): the profile's kernels with the polarity EMIT (first maximum, the
// crossings downward, the sums' sign, the gate on the peak's excess over the background), the same walks, state and tile;
// k_map_finish<5, 0, RING> masks with a ring around the limb instead of the disk's circle.
#include "shg_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kPlanes = 5;                     // shift, core, width, cog, ew
constexpr int kMaxHalfWidth = 32;
constexpr int kRowsPerLane = 8;
constexpr int kTileRows = 64 * kRowsPerLane;   // slit rows of a workgroup
constexpr int kWaves = 8;
constexpr int kTileFrames = 16;                // frames of a workgroup: two a wave
constexpr int kPhases = kTileFrames / kWaves;  // the profile's: one frame a wave at a time
constexpr int kInFlight = 8;                   // raw rows a lane has loads in flight for
constexpr int kMaxLevels = 8;                  // bisector levels of one call
constexpr int kLevelsPerPass = 2;              // bisector levels of one walk 2 (see the top of the file)

// The map kernels' one argument: the Dopplergram passes shift 0 and its one plane; nl and f are the bisectors' alone.
struct MapArgs {
    const void* stack;
    int n;
    int64_t height, width, fstride;            // file layout
    const double* fit;                         // [ih][4]
    int hw, shift;
    float* planes;
    int64_t plane_stride, pitch, n_cols, k_offset;
    int flip_x;
    int nl;                                    // bisectors: K, planes 0 .. K-1 bisectors, K .. 2K-1 chords
    double f[kMaxLevels];                      // the levels' fractions
    double min_excess;                         // the emission maps' gate
};

// Window of a slit row around fit[y][0] + S: lo > hi when the row has none (then its shift, and every plane, is NaN).
__device__ __forceinline__ void window_of(double f0, int s, int hw, int iw, int& lo, int& hi) {
    lo = 1;
    hi = 0;
    if (!isfinite(f0)) return;
    const int c = (int)fmin(fmax(f0 + (double)s, -0x1p+30), 0x1p+30);   // truncation toward zero (a5); beyond 2^30 no window survives
    const int l = max(c - hw, 1), h = min(c + hw, iw - 2);
    if (h - l < 2) return;
    lo = l;
    hi = h;
}

// The streaming arg-minimum of one slit row: the first minimum of p over [lo, hi] and the samples either side of it.  EMIT (the
// emission maps' polarity, here and below): the first maximum.
struct Core {
    int best, jb, a, e, prev;
};

template <bool EMIT = false>
__device__ __forceinline__ void core_init(Core& s) {
    s.best = EMIT ? INT_MIN : INT_MAX;
    s.jb = -2;
    s.a = s.e = s.prev = 0;
}

// in_window() runs for the samples inside [lo, hi] (walk 1 of the profile adds its sums there).
template <bool EMIT = false, typename F = void (*)()>
__device__ __forceinline__ void core_step(Core& s, int j, int p, int lo, int hi, F&& in_window = [] {}) {
    if (j == s.jb + 1) s.e = p;
    if (j >= lo && j <= hi) {
        if (EMIT ? p > s.best : p < s.best) {
            s.best = p;
            s.jb = j;
            s.a = s.prev;
        }
        in_window();
    }
    s.prev = p;
}

// d = (float)(((double)j* + delta) - ref), NaN unless lo < j* < hi.  a > b strictly (first occurrence) and e >= b, so the
// denominator is positive (at a first maximum a < b and e <= b: negative); every integer is exact in float64 and the quotient is
// one IEEE division.
__device__ __forceinline__ float core_shift(const Core& s, int lo, int hi, double ref) {
    if (!(s.jb > lo && s.jb < hi)) return __builtin_nanf("");
    const double delta = (double)(s.a - s.e) / (double)(2 * (s.a + s.e - 2 * s.best));
    return (float)(((double)s.jb + delta) - ref);
}

// Walk 1: the line core's state, Σp, Σ(j - lo) p and p(lo) + p(hi).  Σ(j - lo) p <= 64 * 65 / 2 * 65535 < 2^31.  (The bisectors read
// only the core's state and C2: the compiler drops the two sums there.)
struct Walk1 {
    Core c;
    int sp, st, c2;
};

template <bool EMIT = false>
__device__ __forceinline__ void walk1_init(Walk1& s) {
    core_init<EMIT>(s.c);
    s.sp = s.st = s.c2 = 0;
}

template <bool EMIT = false>
__device__ __forceinline__ void walk1_step(Walk1& s, int j, int p, int lo, int hi) {
    core_step<EMIT>(s.c, j, p, lo, hi, [&] {
        s.sp += p;
        s.st += (j - lo) * p;
        if (j == lo || j == hi) s.c2 += p;
    });
}

// core_d of a row with a vertex (lo < j* < hi): the parabola's value at its vertex.  den > 0: a > b (first minimum), e >= b (the
// emission maps' peak_d: den < 0).
__device__ __forceinline__ double core_d_of(const Core& c) {
    const int den = c.a + c.e - 2 * c.best;
    const int64_t d = c.a - c.e;
    return (double)c.best - (double)(d * d) / (8.0 * (double)den);
}

// level = ((1 - f) core_d) + (f (0.5 C2)), one IEEE operation a step (f = 0.5: the profile's half, bit for bit).
__device__ __forceinline__ double level_of(double f, double core_d, int c2) { return ((1.0 - f) * core_d) + (f * (0.5 * (double)c2)); }

// The crossing threshold ceil(level) of a row with a vertex, INT_MAX when p(j*) >= level (|level| < 2^30: core_d > -2^30, C2 < 2^17).
// EMIT: floor(level), INT_MIN when p(j*) <= level (the crossings are the samples <= level).  no_cross<EMIT>: that sentinel.
template <bool EMIT = false>
constexpr int no_cross = EMIT ? INT_MIN : INT_MAX;

template <bool EMIT = false>
__device__ __forceinline__ int thr_of(double level, int best) {
    if constexpr (EMIT) return (double)best > level ? (int)floor(level) : INT_MIN;
    return (double)best < level ? (int)ceil(level) : INT_MAX;
}

// The planes walk 1 decides (shift, core, cog, ew), and the half level of the width: see include/shg_hip.h.
struct Vertex {
    float shift, core, cog, ew;
    double half;
    int thr;                                   // INT_MAX: no width
};

// EMIT (shg_line_emission): shift, peak = the excess over the background C2 / 2, cog and flux of p - C2 / 2 (S0 and S1 with the other
// sign), every plane NaN unless the first maximum is bracketed and its excess reaches min_excess.
template <bool EMIT = false>
__device__ __forceinline__ Vertex vertex_of(const Walk1& s, int lo, int hi, double ref, double min_excess = 0.0) {
    const float nan = __builtin_nanf("");
    Vertex v{nan, nan, nan, nan, 0.0, no_cross<EMIT>};
    if (lo > hi) return v;
    const int64_t n = hi - lo + 1, c2 = s.c2;
    const int64_t s0 = n * c2 - 2 * (int64_t)s.sp;
    const int64_t sj = n * (int64_t)(lo + hi) / 2;                       // Σj over [lo, hi] (n (lo + hi) is even)
    const int64_t s1 = c2 * sj - 2 * ((int64_t)lo * s.sp + (int64_t)s.st);
    if constexpr (EMIT) {
        if (!(s.c.jb > lo && s.c.jb < hi)) return v;
        const double peak = core_d_of(s.c);
        const double excess = peak - 0.5 * (double)s.c2;
        if (!(excess >= min_excess)) return v;
        v.shift = core_shift(s.c, lo, hi, ref);
        v.core = (float)excess;
        if (s0 < 0) {
            v.cog = (float)((double)-s1 / (double)-s0 - ref);
            v.ew = (float)(0.5 * (double)-s0);
        }
        v.half = level_of(0.5, peak, s.c2);
        v.thr = thr_of<true>(v.half, s.c.best);
        return v;
    }
    if (s0 > 0) v.cog = (float)((double)s1 / (double)s0 - ref);
    if (c2 != 0) v.ew = (float)((double)s0 / (double)c2);
    if (!(s.c.jb > lo && s.c.jb < hi)) return v;
    v.shift = core_shift(s.c, lo, hi, ref);
    const double core = core_d_of(s.c);
    v.core = (float)core;
    v.half = level_of(0.5, core, s.c2);
    v.thr = thr_of(v.half, s.c.best);
    return v;
}

// Walk 2's crossing state of one (slit row, level): jl = the largest j in [lo, j*) with p(j) >= level, jr = the smallest j in
// (j*, hi] with p(j) >= level (p(j) >= level <=> p(j) >= thr = ceil(level) for integer p; thr = INT_MAX when the row has no
// crossings).  The sample pairs either side of a crossing are kept as p | p' << 16 (samples < 2^16).  The previous sample is the
// caller's, kept beside the state (one for all of a row's levels).  EMIT: p(j) <= level <=> p(j) <= thr = floor(level).
struct Cross {
    int jl, jr;
    uint32_t l, r;
};

__device__ __forceinline__ void cross_init(Cross& s) {
    s.jl = s.jr = -1;
    s.l = s.r = 0;
}

template <bool EMIT = false>
__device__ __forceinline__ void cross_step(Cross& s, int j, int p, int prev, int lo, int hi, int jb, int thr) {
    if (j > lo && j <= jb && (EMIT ? prev <= thr : prev >= thr)) {
        s.jl = j - 1;
        s.l = (uint32_t)prev | ((uint32_t)p << 16);      // p(jl), p(jl + 1)
    }
    if (j > jb && j <= hi && s.jr < 0 && (EMIT ? p <= thr : p >= thr)) {
        s.jr = j;
        s.r = (uint32_t)p | ((uint32_t)prev << 16);      // p(jr), p(jr - 1)
    }
}

// The crossings xl, xr of walk 2's state at `level`, each interpolated linearly with its inner neighbour: bis = their midpoint
// - ref and len = the chord xr - xl (at half: the profile's width); both NaN when the row has no crossing pair.  EMIT: the header
// writes (level - p(jl)) / (p(jl + 1) - p(jl)), both operands of the quotient below negated, which is the same float64.
struct Chord {
    float bis, len;
};

template <bool EMIT = false>
__device__ __forceinline__ Chord crossings(const Cross& s, double level, int thr, double ref) {
    Chord c{__builtin_nanf(""), __builtin_nanf("")};
    if (thr == no_cross<EMIT> || s.jl < 0 || s.jr < 0) return c;
    const int pl = (int)(s.l & 0xffffu), pl1 = (int)(s.l >> 16), pr = (int)(s.r & 0xffffu), pr1 = (int)(s.r >> 16);
    const double xl = (double)s.jl + ((double)pl - level) / (double)(pl - pl1);
    const double xr = (double)s.jr - ((double)pr - level) / (double)(pr - pr1);
    c.bis = (float)((0.5 * (xl + xr)) - ref);
    c.len = (float)(xr - xl);
    return c;
}

// eight samples of one raw row, as four dwords of u16 pairs (sample r in the (r & 1) half of dword r >> 1)
struct Row8 {
    uint32_t w[4];
};

template <typename T, bool VEC>
__device__ __forceinline__ Row8 load_row8(const char* frame, uint32_t off, int64_t x0, int64_t width) {
    Row8 v;
    if (VEC) {
        if (sizeof(T) == 2) {
            const uint4 q = *reinterpret_cast<const uint4*>(frame + off);
            v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
        } else {
            const uint2 q = *reinterpret_cast<const uint2*>(frame + off);
            v.w[0] = (q.x & 0xffu) | ((q.x << 8) & 0xff0000u);
            v.w[1] = ((q.x >> 16) & 0xffu) | ((q.x >> 8) & 0xff0000u);
            v.w[2] = (q.y & 0xffu) | ((q.y << 8) & 0xff0000u);
            v.w[3] = ((q.y >> 16) & 0xffu) | ((q.y >> 8) & 0xff0000u);
        }
    } else {
        const T* p = reinterpret_cast<const T*>(frame + off);
        uint32_t s[kRowsPerLane];
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) s[r] = x0 + r < width ? (uint32_t)p[r] : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) v.w[i] = s[2 * i] | (s[2 * i + 1] << 16);
    }
    return v;
}

// A rotated kernel's lane: its eight slit rows (raw columns x0 .. x0 + 7), their windows around fit[y][0] + S, the rows [llo, lhi]
// those windows span (INT_MAX / INT_MIN when none has one) and the wave's band [wlo, whi] (wave-uniform).
struct Band {
    int64_t x0, width;                         // width = ih
    uint32_t rowb, colb;                       // bytes of a raw row, x0's byte offset in it
    int lo[kRowsPerLane], hi[kRowsPerLane];
    int llo, lhi, wlo, whi;
};

template <typename T, typename Args>
__device__ __forceinline__ Band band_of(const Args& a, int s) {
    Band b;
    b.width = a.width;
    b.x0 = (int64_t)blockIdx.x * kTileRows + (threadIdx.x & 63) * kRowsPerLane;
    b.llo = INT_MAX;
    b.lhi = INT_MIN;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
        const int64_t x = b.x0 + r;
        const int64_t y = b.width - 1 - x;                          // a1: out[i, j] = raw[j, W - 1 - i]
        window_of(x < b.width ? a.fit[y * 4] : (double)NAN, s, a.hw, (int)a.height, b.lo[r], b.hi[r]);
        if (b.lo[r] <= b.hi[r]) {
            b.llo = min(b.llo, b.lo[r]);
            b.lhi = max(b.lhi, b.hi[r]);
        }
    }
    int wlo = b.llo, whi = b.lhi;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        wlo = min(wlo, __shfl_xor(wlo, d));
        whi = max(whi, __shfl_xor(whi, d));
    }
    b.wlo = __builtin_amdgcn_readfirstlane(wlo);
    b.whi = __builtin_amdgcn_readfirstlane(whi);
    b.rowb = (uint32_t)(b.width * (int64_t)sizeof(T));             // (the entry point checks a frame's bytes < 4 GiB)
    b.colb = (uint32_t)(b.x0 * (int64_t)sizeof(T));
    return b;
}

// One walk of the band [wlo, whi] by a lane: step(j, r, p) for its eight slit rows r; rows outside the lane's [llo, lhi] read as 0.
template <typename T, bool VEC, typename Step>
__device__ __forceinline__ void walk_band(const char* frame, const Band& b, Step&& step) {
    constexpr int scale = sizeof(T) == 1 ? 256 : 1;                  // video_reader.py:121-122
    for (int j0 = b.wlo; j0 <= b.whi; j0 += kInFlight) {
        Row8 v[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int j = j0 + u;
            if (j <= b.whi && j >= b.llo && j <= b.lhi) {
                v[u] = load_row8<T, VEC>(frame, (uint32_t)j * b.rowb + b.colb, b.x0, b.width);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[u].w[q] = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int j = j0 + u;
            if (j > b.lhi) break;
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) step(j, r, (int)((v[u].w[r >> 1] >> (16 * (r & 1))) & 0xffffu) * scale);
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void k_line_core_rot(const MapArgs a) {
    __shared__ float tile[kTileRows][kTileFrames + 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Band b = band_of<T>(a, 0);
    double f3[kRowsPerLane];
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) f3[r] = b.x0 + r < b.width ? a.fit[(b.width - 1 - b.x0 - r) * 4 + 3] : 0.0;
    for (int i = 0; i < kTileFrames / kWaves; ++i) {
        const int f = wave + kWaves * i;
        const int64_t k = (int64_t)blockIdx.y * kTileFrames + f;
        if (k >= a.n) break;
        const char* frame = static_cast<const char*>(a.stack) + k * a.fstride * (int64_t)sizeof(T);
        Core s[kRowsPerLane];
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) core_init(s[r]);
        walk_band<T, VEC>(frame, b, [&](int j, int r, int p) { core_step(s[r], j, p, b.lo[r], b.hi[r]); });
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) tile[lane * kRowsPerLane + r][f] = core_shift(s[r], b.lo[r], b.hi[r], f3[r]);
    }
    __syncthreads();
    // 16 threads write 16 consecutive columns of one map row
    const int64_t kb = (int64_t)blockIdx.y * kTileFrames;
    for (int idx = threadIdx.x; idx < kTileRows * kTileFrames; idx += 64 * kWaves) {
        const int rl = idx / kTileFrames, f = idx % kTileFrames;
        const int64_t x = (int64_t)blockIdx.x * kTileRows + rl, k = kb + f;
        if (x < b.width && k < a.n) {
            const int64_t c = a.k_offset + k;
            a.planes[(b.width - 1 - x) * a.pitch + (a.flip_x ? a.n_cols - 1 - c : c)] = tile[rl][f];
        }
    }
}

// LDS tile [plane][frame of the phase][slit row]: row index XOR 4 x frame, so that the read-out (8 frames x 4 rows per 32 lanes)
// hits 32 banks and a lane's four consecutive rows stay one aligned float4.
__device__ __forceinline__ int tile_at(int q, int f, int row) { return (q * kWaves + f) * kTileRows + (row ^ (f << 2)); }

// A phase's Q-plane tile to the planes, from frame kb on: 8 threads write 8 consecutive columns of one map row of one plane.  Tile
// plane qt goes to plane plane_of(qt), nowhere when that is < 0.
template <int Q, typename PlaneOf>
__device__ __forceinline__ void write_tile(const MapArgs& a, const float* tile, int64_t kb, PlaneOf&& plane_of) {
    for (int idx = threadIdx.x; idx < Q * kTileRows * kWaves; idx += 64 * kWaves) {
        const int qt = idx / (kTileRows * kWaves), rl = (idx / kWaves) % kTileRows, f = idx % kWaves;
        const int64_t q = plane_of(qt);
        const int64_t x = (int64_t)blockIdx.x * kTileRows + rl, kf = kb + f;
        if (q >= 0 && x < a.width && kf < a.n) {
            const int64_t c = a.k_offset + kf;
            a.planes[q * a.plane_stride + (a.width - 1 - x) * a.pitch + (a.flip_x ? a.n_cols - 1 - c : c)] = tile[tile_at(qt, f, rl)];
        }
    }
}

template <typename T, bool VEC, bool EMIT = false>
__global__ __launch_bounds__(64 * kWaves) void k_line_profile_rot(const MapArgs a) {
    __shared__ float tile[kPlanes * kWaves * kTileRows];            // 80 KiB: two workgroups per CU
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Band b = band_of<T>(a, a.shift);
    for (int ph = 0; ph < kPhases; ++ph) {
        const int64_t kb = (int64_t)blockIdx.y * kTileFrames + ph * kWaves;
        const int64_t k = kb + wave;
        if (k < a.n) {
            const char* frame = static_cast<const char*>(a.stack) + k * a.fstride * (int64_t)sizeof(T);
            Walk1 s[kRowsPerLane];
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) walk1_init<EMIT>(s[r]);
            walk_band<T, VEC>(frame, b, [&](int j, int r, int p) { walk1_step<EMIT>(s[r], j, p, b.lo[r], b.hi[r]); });
            double half[kRowsPerLane];
            int thr[kRowsPerLane], jb[kRowsPerLane];
#pragma unroll
            for (int h = 0; h < kRowsPerLane; h += 4) {
                Vertex v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t x = b.x0 + h + r;
                    const double ref = x < b.width ? a.fit[(b.width - 1 - x) * 4 + 3] + (double)a.shift : 0.0;
                    v[r] = vertex_of<EMIT>(s[h + r], b.lo[h + r], b.hi[h + r], ref, a.min_excess);
                    half[h + r] = v[r].half;
                    thr[h + r] = v[r].thr;
                    jb[h + r] = s[h + r].c.jb;
                }
                const int row = lane * kRowsPerLane + h;
                *reinterpret_cast<float4*>(&tile[tile_at(0, wave, row)]) = make_float4(v[0].shift, v[1].shift, v[2].shift, v[3].shift);
                *reinterpret_cast<float4*>(&tile[tile_at(1, wave, row)]) = make_float4(v[0].core, v[1].core, v[2].core, v[3].core);
                *reinterpret_cast<float4*>(&tile[tile_at(3, wave, row)]) = make_float4(v[0].cog, v[1].cog, v[2].cog, v[3].cog);
                *reinterpret_cast<float4*>(&tile[tile_at(4, wave, row)]) = make_float4(v[0].ew, v[1].ew, v[2].ew, v[3].ew);
            }
            Cross t[kRowsPerLane];
            int prev[kRowsPerLane];
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) {
                cross_init(t[r]);
                prev[r] = 0;
            }
            walk_band<T, VEC>(frame, b, [&](int j, int r, int p) {
                cross_step<EMIT>(t[r], j, p, prev[r], b.lo[r], b.hi[r], jb[r], thr[r]);
                prev[r] = p;
            });
#pragma unroll
            for (int h = 0; h < kRowsPerLane; h += 4)
                *reinterpret_cast<float4*>(&tile[tile_at(2, wave, lane * kRowsPerLane + h)]) = make_float4(
                    crossings<EMIT>(t[h], half[h], thr[h], 0.0).len, crossings<EMIT>(t[h + 1], half[h + 1], thr[h + 1], 0.0).len,
                    crossings<EMIT>(t[h + 2], half[h + 2], thr[h + 2], 0.0).len, crossings<EMIT>(t[h + 3], half[h + 3], thr[h + 3], 0.0).len);
        }
        __syncthreads();
        write_tile<kPlanes>(a, tile, kb, [](int qt) { return (int64_t)qt; });
        __syncthreads();
    }
}

// A plain kernel's thread (a wave: one slit row y of 64 frames k): the window around fit[y][0] + S, the row's samples p(j) and the
// output (plane 0) of (y, k).  plain_row() is false outside the map.
template <typename T>
struct PlainRow {
    int64_t y;
    int lo, hi;
    const T* row;
    float* out;
    __device__ int p(int j) const { return (int)row[j] * (sizeof(T) == 1 ? 256 : 1); }   // video_reader.py:121-122
};

template <typename T>
__device__ __forceinline__ bool plain_row(const MapArgs& a, PlainRow<T>& t) {
    t.y = (int64_t)blockIdx.y * kWaves + (threadIdx.x >> 6);
    const int64_t k = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    if (t.y >= a.height || k >= a.n) return false;
    window_of(a.fit[t.y * 4], a.shift, a.hw, (int)a.width, t.lo, t.hi);
    t.row = static_cast<const T*>(a.stack) + k * a.fstride + t.y * a.width;
    const int64_t c = a.k_offset + k;
    t.out = a.planes + t.y * a.pitch + (a.flip_x ? a.n_cols - 1 - c : c);
    return true;
}

// Walk 2 of a plain kernel's row at one level (none when thr = INT_MAX: no crossing can be found).
template <typename T, bool EMIT = false>
__device__ __forceinline__ Cross cross_row(const PlainRow<T>& t, int jb, int thr) {
    Cross s;
    cross_init(s);
    if (thr == no_cross<EMIT>) return s;
    for (int j = t.lo, prev = 0; j <= t.hi; ++j) {
        const int p = t.p(j);
        cross_step<EMIT>(s, j, p, prev, t.lo, t.hi, jb, thr);
        prev = p;
    }
    return s;
}

template <typename T>
__global__ __launch_bounds__(64 * kWaves) void k_line_core_plain(const MapArgs a) {
    PlainRow<T> t;
    if (!plain_row(a, t)) return;
    Core s;
    core_init(s);
    for (int j = t.lo; j <= t.hi; ++j) core_step(s, j, t.p(j), t.lo, t.hi);
    t.out[0] = core_shift(s, t.lo, t.hi, a.fit[t.y * 4 + 3]);
}

template <typename T, bool EMIT = false>
__global__ __launch_bounds__(64 * kWaves) void k_line_profile_plain(const MapArgs a) {
    PlainRow<T> t;
    if (!plain_row(a, t)) return;
    Walk1 s;
    walk1_init<EMIT>(s);
    for (int j = t.lo; j <= t.hi; ++j) walk1_step<EMIT>(s, j, t.p(j), t.lo, t.hi);
    const Vertex v = vertex_of<EMIT>(s, t.lo, t.hi, a.fit[t.y * 4 + 3] + (double)a.shift, a.min_excess);
    t.out[0] = v.shift;
    t.out[a.plane_stride] = v.core;
    t.out[2 * a.plane_stride] = crossings<EMIT>(cross_row<T, EMIT>(t, s.c.jb, v.thr), v.half, v.thr, 0.0).len;
    t.out[3 * a.plane_stride] = v.cog;
    t.out[4 * a.plane_stride] = v.ew;
}

// ---- line bisectors (shg_line_bisector) ----
template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void k_line_bisector_rot(const MapArgs a) {
    constexpr int L = kLevelsPerPass;
    __shared__ float tile[2 * L * kWaves * kTileRows];              // 64 KiB: two workgroups per CU
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Band b = band_of<T>(a, a.shift);
    const int passes = (a.nl + L - 1) / L;
    for (int ph = 0; ph < kPhases; ++ph) {
        const int64_t kb = (int64_t)blockIdx.y * kTileFrames + ph * kWaves;
        const int64_t k = kb + wave;
        const char* frame = static_cast<const char*>(a.stack) + k * a.fstride * (int64_t)sizeof(T);
        double core[kRowsPerLane];
        int c2[kRowsPerLane], best[kRowsPerLane], jb[kRowsPerLane];
        if (k < a.n) {
            Walk1 s[kRowsPerLane];
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) walk1_init(s[r]);
            walk_band<T, VEC>(frame, b, [&](int j, int r, int p) { walk1_step(s[r], j, p, b.lo[r], b.hi[r]); });
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) {
                const bool vertex = s[r].c.jb > b.lo[r] && s[r].c.jb < b.hi[r];     // (false without a window: lo > hi)
                core[r] = vertex ? core_d_of(s[r].c) : 0.0;
                c2[r] = s[r].c2;
                best[r] = s[r].c.best;
                jb[r] = vertex ? s[r].c.jb : -1;
            }
        }
        for (int ps = 0; ps < passes; ++ps) {
            const int l0 = ps * L, nl = min(L, a.nl - l0);
            if (k < a.n) {
                Cross t[kRowsPerLane][L];
                int thr[kRowsPerLane][L], prev[kRowsPerLane];
#pragma unroll
                for (int r = 0; r < kRowsPerLane; ++r) {
                    prev[r] = 0;
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        thr[r][l] = jb[r] >= 0 && l < nl ? thr_of(level_of(a.f[l0 + l], core[r], c2[r]), best[r]) : INT_MAX;
                        cross_init(t[r][l]);
                    }
                }
                walk_band<T, VEC>(frame, b, [&](int j, int r, int p) {
#pragma unroll
                    for (int l = 0; l < L; ++l)
                        if (l < nl) cross_step(t[r][l], j, p, prev[r], b.lo[r], b.hi[r], jb[r], thr[r][l]);
                    prev[r] = p;
                });
#pragma unroll
                for (int h = 0; h < kRowsPerLane; h += 4) {
#pragma unroll
                    for (int l = 0; l < L; ++l) {
                        Chord c[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int64_t x = b.x0 + h + r;
                            const double ref = x < b.width ? a.fit[(b.width - 1 - x) * 4 + 3] + (double)a.shift : 0.0;
                            c[r] = crossings(t[h + r][l], l < nl ? level_of(a.f[l0 + l], core[h + r], c2[h + r]) : 0.0, thr[h + r][l], ref);
                        }
                        const int row = lane * kRowsPerLane + h;
                        *reinterpret_cast<float4*>(&tile[tile_at(l, wave, row)]) = make_float4(c[0].bis, c[1].bis, c[2].bis, c[3].bis);
                        *reinterpret_cast<float4*>(&tile[tile_at(L + l, wave, row)]) = make_float4(c[0].len, c[1].len, c[2].len, c[3].len);
                    }
                }
            }
            __syncthreads();
            // tile plane qt < L is level l0 + qt's bisector, L + i its chord
            write_tile<2 * L>(a, tile, kb, [&](int qt) {
                const int li = qt % L;
                return li < nl ? (int64_t)((qt < L ? 0 : a.nl) + l0 + li) : (int64_t)-1;
            });
            __syncthreads();
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kWaves) void k_line_bisector_plain(const MapArgs a) {
    PlainRow<T> t;
    if (!plain_row(a, t)) return;
    Walk1 s;
    walk1_init(s);
    for (int j = t.lo; j <= t.hi; ++j) walk1_step(s, j, t.p(j), t.lo, t.hi);
    const bool vertex = s.c.jb > t.lo && s.c.jb < t.hi;
    const double core = vertex ? core_d_of(s.c) : 0.0;
    const double ref = a.fit[t.y * 4 + 3] + (double)a.shift;
    for (int i = 0; i < a.nl; ++i) {
        const double level = level_of(a.f[i], core, s.c2);
        const int thr = vertex ? thr_of(level, s.c.best) : INT_MAX;
        const Chord c = crossings(cross_row(t, s.c.jb, thr), level, thr, ref);
        t.out[i * a.plane_stride] = c.bis;
        t.out[(a.nl + i) * a.plane_stride] = c.len;
    }
}

struct FinishArgs {
    const float* raw;
    int64_t raw_plane, h, w, raw_pitch;
    double h00, h01, h02;
    int64_t out_h, out_w;
    int masked;
    double cx, cy, rad;
    int64_t nw, lo, dx0, n;                    // crop_plan: new[:, dx0:dx0+n] = img[:, lo:lo+n]
    float* map;
    int64_t map_plane, map_pitch;
    uint16_t* png;
    int64_t png_plane, png_pitch;
    double shift_scale, width_scale;           // 32767 / R, 65534 / (2H + 1)
    double rin, flux_div;                      // the emission maps': the ring's inner radius (rad: its outer one), 2H + 1
};

// One thread per output pixel, its P planes: P = 1 for the Dopplergram's shift map, kPlanes for the profile's, 2 KB for KB bisector
// levels.  Display planes: shift and cog around 32768, core as it is, width and ew from 1 up; with KB > 0, planes q < KB (the
// bisectors) around 32768 and the chords from 1 up.  RING (the emission maps' mask policy): NaN on and inside the circle of radius
// rin (none when rin < 0) and outside the one of radius rad, and the flux plane (4) divided by 2H + 1.
template <int P, int KB = 0, bool RING = false>
__global__ __launch_bounds__(256) void k_map_finish(const FinishArgs a) {
    const int64_t oc = (int64_t)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (oc >= a.nw) return;
    const int64_t c = oc - a.dx0 + a.lo;
    const bool inside = oc >= a.dx0 && oc < a.dx0 + a.n && r < a.h;
    double t = 0.0;
    int64_t i0 = -1, i1 = -1;                  // the taps, -1 outside [0, w)
    bool off = !inside;
    if (inside) {
        const double x = (a.h00 * (double)c + a.h01 * (double)r) + a.h02;
        const double x0 = floor(x), x1 = ceil(x);
        t = x - x0;
        const double w = (double)a.w;
        if (x0 >= 0.0 && x0 < w) i0 = (int64_t)x0;
        if (x1 >= 0.0 && x1 < w) i1 = (int64_t)x1;
        if (a.masked) {
            const double dx = (double)c - a.cx, dy = (double)r - a.cy;
            const double d2 = dx * dx + dy * dy;
            off = d2 > a.rad * a.rad;
            if (RING) off = off || (a.rin >= 0.0 && d2 <= a.rin * a.rin);
        }
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
        float v = __builtin_nanf("");
        if (!off) {
            const float* row = a.raw + q * a.raw_plane + r * a.raw_pitch;
            const double left = i0 >= 0 ? (double)row[i0] : (double)NAN;
            const double right = i1 >= 0 ? (double)row[i1] : (double)NAN;
            v = (float)((1.0 - t) * left + t * right);
        }
        a.map[q * a.map_plane + r * a.map_pitch + oc] = v;
        if (a.png) {
            uint16_t d = 0;
            if (!isnan(v)) {
                const double e = KB > 0 ? (q < KB ? 32768.0 + (double)v * a.shift_scale : 1.0 + (double)v * a.width_scale)
                                 : q == 0 || q == 3 ? 32768.0 + (double)v * a.shift_scale
                                 : q == 1           ? (double)v
                                 : RING && q == 4   ? (double)v / a.flux_div
                                                    : 1.0 + (double)v * a.width_scale;
                d = (uint16_t)fmin(fmax(rint(e), 1.0), 65535.0);
            }
            a.png[q * a.png_plane + r * a.png_pitch + oc] = d;
        }
    }
}

// The checks the three maps share; `fn` names the entry point in the messages.  Beyond the Dopplergram's one plane (planes = 1,
// measured at the fitted line) also the plane stride and the shift.
int check_map_args(const char* fn, const void* stack, const double* fit, const float* out, int64_t n_frames, int64_t height,
                   int64_t width, int bytes_per_px, int64_t frame_stride_px, int half_width, int shift, int planes, int64_t plane_stride,
                   int64_t row_pitch, int64_t n_cols, int64_t k_offset) {
    SHG_REQUIRE(stack && fit && out, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(n_frames > 0 && height > 0 && width > 0, SHG_E_ARG, "%s: empty input", fn);
    SHG_REQUIRE(bytes_per_px == 1 || bytes_per_px == 2, SHG_E_ARG, "%s: bytes_per_px must be 1 or 2", fn);
    SHG_REQUIRE(half_width >= 1 && half_width <= kMaxHalfWidth, SHG_E_UNSUPPORTED, "%s: half-width %d outside [1, %d]", fn, half_width,
                kMaxHalfWidth);
    SHG_REQUIRE(n_frames < (1ll << 31) && n_cols < (1ll << 31), SHG_E_UNSUPPORTED, "%s: %lld frames / %lld columns", fn,
                (long long)n_frames, (long long)n_cols);
    SHG_REQUIRE(n_cols >= n_frames && k_offset >= 0 && k_offset + n_frames <= n_cols, SHG_E_ARG,
                "%s: frames [%lld, %lld) do not fit %lld columns", fn, (long long)k_offset, (long long)(k_offset + n_frames),
                (long long)n_cols);
    SHG_REQUIRE(row_pitch >= n_cols, SHG_E_ARG, "%s: row_pitch < n_cols", fn);
    SHG_REQUIRE(frame_stride_px == 0 || frame_stride_px >= height * width, SHG_E_ARG, "%s: frame stride smaller than a frame", fn);
    // (the rotated kernels address a sample as `frame base + 32-bit byte offset`, their spectral rows as int)
    SHG_REQUIRE(height * width * bytes_per_px < (1ll << 32) && height < (1ll << 31) && width < (1ll << 31), SHG_E_UNSUPPORTED,
                "%s: a frame of %lld x %lld samples is larger than 4 GiB", fn, (long long)height, (long long)width);
    if (planes != 1) {
        const int64_t ih = width > height ? width : height, iw = width > height ? height : width;
        SHG_REQUIRE(plane_stride >= ih * row_pitch, SHG_E_ARG, "%s: plane stride < %lld x %lld", fn, (long long)ih, (long long)row_pitch);
        // a line at a column in [0, iw) shifted by S has a window of three samples within [1, iw - 2] only when 3 - iw - H < S < iw - 3 + H
        SHG_REQUIRE(shift > 3 - iw - half_width && shift < iw - 3 + half_width, SHG_E_ARG,
                    "%s: shift %d puts every window outside columns [1, %lld]", fn, shift, (long long)(iw - 2));
    }
    return 0;
}

// The launch the three maps share: on rotated files (width > height) the rotated kernel, 512 slit rows x 16 frames a workgroup, with
// 16-byte pieces (8 for 8-bit samples) when every row of every frame starts on that boundary; else the plain kernel, 64 frames x 8
// slit rows a workgroup.  rot(T(), std::bool_constant<VEC>()) and plain(T()) name the kernels' instances.
template <typename Rot, typename Plain>
int launch_map(const MapArgs& a, int bytes_per_px, hipStream_t st, Rot rot, Plain plain, const char* rot_name, const char* plain_name) {
    const int64_t ih = a.width > a.height ? a.width : a.height;
    if (a.width > a.height) {
        const int64_t piece = kRowsPerLane * bytes_per_px;
        const bool vec = (reinterpret_cast<uintptr_t>(a.stack) % piece) == 0 && (a.width * bytes_per_px) % piece == 0 &&
                         (a.fstride * bytes_per_px) % piece == 0;
        const dim3 grid((unsigned)((ih + kTileRows - 1) / kTileRows), (unsigned)((a.n + kTileFrames - 1) / kTileFrames));
        const std::true_type v;
        const std::false_type s;
        if (bytes_per_px == 2) return shg::launch(vec ? rot(uint16_t(), v) : rot(uint16_t(), s), grid, dim3(64 * kWaves), 0, st, a, rot_name);
        return shg::launch(vec ? rot(uint8_t(), v) : rot(uint8_t(), s), grid, dim3(64 * kWaves), 0, st, a, rot_name);
    }
    const dim3 grid((unsigned)((a.n + 63) / 64), (unsigned)((ih + kWaves - 1) / kWaves));
    return shg::launch(bytes_per_px == 2 ? plain(uint16_t()) : plain(uint8_t()), grid, dim3(64 * kWaves), 0, st, a, plain_name);
}

// The checks the finish calls share, and the crop (crop_plan's (nw, lo, dx0, n); none when crop4 is NULL), the mask and the display
// scales resolved into `a`, which holds the caller's planes, strides and warp.  planes = 1: the Dopplergram's one plane, which has
// no width plane (half_width is not read).
int finish_args(const char* fn, int planes, const double* circle3, const int64_t* crop4, int half_width, double display_range,
                FinishArgs& a) {
    SHG_REQUIRE(a.raw && a.map, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(a.h > 0 && a.w > 0 && a.raw_pitch >= a.w && (planes == 1 || a.raw_plane >= a.h * a.raw_pitch) && a.out_h > 0 &&
                    a.out_w > 0,
                SHG_E_ARG, "%s: empty or mis-pitched input", fn);
    SHG_REQUIRE(a.out_h < (1ll << 31), SHG_E_UNSUPPORTED, "%s: %lld output rows", fn, (long long)a.out_h);
    a.nw = a.n = a.out_w;
    a.lo = a.dx0 = 0;
    if (crop4) {
        a.nw = crop4[0];
        a.lo = crop4[1];
        a.dx0 = crop4[2];
        a.n = crop4[3];
        SHG_REQUIRE(a.nw > 0 && a.lo >= 0 && a.dx0 >= 0 && a.n >= 0 && a.dx0 + a.n <= a.nw && a.lo + a.n <= a.out_w, SHG_E_ARG,
                    "%s: crop (%lld, %lld, %lld, %lld) does not fit %lld columns", fn, (long long)a.nw, (long long)a.lo,
                    (long long)a.dx0, (long long)a.n, (long long)a.out_w);
    }
    if (planes == 1) {
        SHG_REQUIRE(a.map_pitch >= a.nw && (!a.png || a.png_pitch >= a.nw), SHG_E_ARG, "%s: output pitch < %lld", fn, (long long)a.nw);
    } else {
        SHG_REQUIRE(a.map_pitch >= a.nw && a.map_plane >= a.out_h * a.map_pitch, SHG_E_ARG, "%s: map pitch < %lld", fn,
                    (long long)a.nw);
        SHG_REQUIRE(!a.png || (a.png_pitch >= a.nw && a.png_plane >= a.out_h * a.png_pitch), SHG_E_ARG, "%s: display pitch < %lld",
                    fn, (long long)a.nw);
    }
    SHG_REQUIRE(!a.png || (isfinite(display_range) && display_range > 0.0), SHG_E_ARG, "%s: display range must be positive", fn);
    a.masked = circle3 && !(circle3[0] == -1.0 && circle3[1] == -1.0 && circle3[2] == -1.0);
    a.cx = a.masked ? circle3[0] : 0.0;
    a.cy = a.masked ? circle3[1] : 0.0;
    a.rad = a.masked ? circle3[2] : 0.0;
    a.shift_scale = a.png ? 32767.0 / display_range : 0.0;
    if (planes != 1) {
        SHG_REQUIRE(!a.png || (half_width >= 1 && half_width <= kMaxHalfWidth), SHG_E_UNSUPPORTED, "%s: half-width %d outside [1, %d]",
                    fn, half_width, kMaxHalfWidth);
        a.width_scale = a.png ? 65534.0 / (double)(2 * half_width + 1) : 0.0;
    }
    return 0;
}

}  // namespace

extern "C" int shg_line_core_shift(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                                   int64_t frame_stride_px, const double* fit, int half_width, int flip_x, float* map,
                                   int64_t row_pitch, int64_t n_cols, int64_t k_offset, shg_stream_t stream) {
    if (const int e = check_map_args("shg_line_core_shift", stack, fit, map, n_frames, height, width, bytes_per_px, frame_stride_px,
                                     half_width, 0, 1, 0, row_pitch, n_cols, k_offset))
        return e;
    const int64_t fstride = frame_stride_px > 0 ? frame_stride_px : height * width;
    MapArgs a{stack, (int)n_frames, height, width, fstride, fit, half_width, 0, map, 0, row_pitch, n_cols, k_offset, flip_x ? 1 : 0, 0, {}};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_core_shift", st);
    return launch_map(
        a, bytes_per_px, st, [](auto t, auto vec) { return k_line_core_rot<decltype(t), decltype(vec)::value>; },
        [](auto t) { return k_line_core_plain<decltype(t)>; }, "k_line_core_rot", "k_line_core_plain");
}

extern "C" int shg_doppler_finish(const float* raw, int64_t h, int64_t w, int64_t raw_pitch, double h00, double h01, double h02,
                                  int64_t out_h, int64_t out_w, const double* circle3, const int64_t* crop4, float* map,
                                  int64_t map_pitch, uint16_t* png, int64_t png_pitch, double display_range, shg_stream_t stream) {
    FinishArgs a{raw, 0, h, w, raw_pitch, h00, h01, h02, out_h, out_w, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, map, 0, map_pitch, png, 0, png_pitch,
                 0.0, 0.0, 0.0, 0.0};
    if (const int e = finish_args("shg_doppler_finish", 1, circle3, crop4, 0, display_range, a)) return e;
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("doppler_finish", st);
    return shg::launch(k_map_finish<1>, dim3((unsigned)((a.nw + 255) / 256), (unsigned)out_h), dim3(256), 0, st, a, "k_map_finish<1>");
}

extern "C" int shg_line_profile(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                                int64_t frame_stride_px, const double* fit, int half_width, int shift, int flip_x, float* planes,
                                int64_t plane_stride, int64_t row_pitch, int64_t n_cols, int64_t k_offset, shg_stream_t stream) {
    if (const int e = check_map_args("shg_line_profile", stack, fit, planes, n_frames, height, width, bytes_per_px, frame_stride_px,
                                     half_width, shift, kPlanes, plane_stride, row_pitch, n_cols, k_offset))
        return e;
    const int64_t fstride = frame_stride_px > 0 ? frame_stride_px : height * width;
    MapArgs a{stack, (int)n_frames, height, width, fstride, fit, half_width, shift, planes, plane_stride, row_pitch, n_cols, k_offset,
              flip_x ? 1 : 0, 0, {}};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_profile", st);
    return launch_map(
        a, bytes_per_px, st, [](auto t, auto vec) { return k_line_profile_rot<decltype(t), decltype(vec)::value>; },
        [](auto t) { return k_line_profile_plain<decltype(t)>; }, "k_line_profile_rot", "k_line_profile_plain");
}

extern "C" int shg_line_profile_finish(const float* raw, int64_t raw_plane_stride, int64_t h, int64_t w, int64_t raw_pitch, double h00,
                                       double h01, double h02, int64_t out_h, int64_t out_w, const double* circle3, const int64_t* crop4,
                                       float* maps, int64_t map_plane_stride, int64_t map_pitch, uint16_t* png, int64_t png_plane_stride,
                                       int64_t png_pitch, int half_width, double display_range, shg_stream_t stream) {
    FinishArgs a{raw, raw_plane_stride, h, w, raw_pitch, h00, h01, h02, out_h, out_w, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, maps,
                 map_plane_stride, map_pitch, png, png_plane_stride, png_pitch, 0.0, 0.0, 0.0, 0.0};
    if (const int e = finish_args("shg_line_profile_finish", kPlanes, circle3, crop4, half_width, display_range, a)) return e;
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_profile_finish", st);
    return shg::launch(k_map_finish<kPlanes>, dim3((unsigned)((a.nw + 255) / 256), (unsigned)out_h), dim3(256), 0, st, a,
                       "k_map_finish<5>");
}

extern "C" int shg_line_emission(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                                 int64_t frame_stride_px, const double* fit, int half_width, int shift, double min_excess, int flip_x,
                                 float* planes, int64_t plane_stride, int64_t row_pitch, int64_t n_cols, int64_t k_offset,
                                 shg_stream_t stream) {
    if (const int e = check_map_args("shg_line_emission", stack, fit, planes, n_frames, height, width, bytes_per_px, frame_stride_px,
                                     half_width, shift, kPlanes, plane_stride, row_pitch, n_cols, k_offset))
        return e;
    SHG_REQUIRE(isfinite(min_excess) && min_excess >= 0.0, SHG_E_ARG, "shg_line_emission: min_excess %g must be finite and >= 0",
                min_excess);
    const int64_t fstride = frame_stride_px > 0 ? frame_stride_px : height * width;
    MapArgs a{stack, (int)n_frames, height, width, fstride, fit, half_width, shift, planes, plane_stride, row_pitch, n_cols, k_offset,
              flip_x ? 1 : 0, 0, {}, min_excess};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_emission", st);
    return launch_map(
        a, bytes_per_px, st, [](auto t, auto vec) { return k_line_profile_rot<decltype(t), decltype(vec)::value, true>; },
        [](auto t) { return k_line_profile_plain<decltype(t), true>; }, "k_line_profile_rot<emission>", "k_line_profile_plain<emission>");
}

extern "C" int shg_line_emission_finish(const float* raw, int64_t raw_plane_stride, int64_t h, int64_t w, int64_t raw_pitch, double h00,
                                        double h01, double h02, int64_t out_h, int64_t out_w, const double* ring4, const int64_t* crop4,
                                        float* maps, int64_t map_plane_stride, int64_t map_pitch, uint16_t* png, int64_t png_plane_stride,
                                        int64_t png_pitch, int half_width, double display_range, shg_stream_t stream) {
    FinishArgs a{raw, raw_plane_stride, h, w, raw_pitch, h00, h01, h02, out_h, out_w, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, maps,
                 map_plane_stride, map_pitch, png, png_plane_stride, png_pitch, 0.0, 0.0, 0.0, 0.0};
    if (const int e = finish_args("shg_line_emission_finish", kPlanes, nullptr, crop4, half_width, display_range, a)) return e;
    if (ring4) {
        SHG_REQUIRE(!isnan(ring4[0]) && !isnan(ring4[1]) && !isnan(ring4[2]) && !isnan(ring4[3]) && ring4[3] >= 0.0 &&
                        ring4[3] >= ring4[2],
                    SHG_E_ARG, "shg_line_emission_finish: ring (%g, %g, %g, %g) needs numbers and 0 <= r_out >= r_in", ring4[0], ring4[1],
                    ring4[2], ring4[3]);
        a.masked = 1;
        a.cx = ring4[0];
        a.cy = ring4[1];
        a.rin = ring4[2];
        a.rad = ring4[3];
    }
    a.flux_div = (double)(2 * half_width + 1);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_emission_finish", st);
    return shg::launch(k_map_finish<kPlanes, 0, true>, dim3((unsigned)((a.nw + 255) / 256), (unsigned)out_h), dim3(256), 0, st, a,
                       "k_map_finish<5, ring>");
}

extern "C" int shg_line_bisector(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                                 int64_t frame_stride_px, const double* fit, int half_width, int shift, const double* levels, int n_levels,
                                 int flip_x, float* planes, int64_t plane_stride, int64_t row_pitch, int64_t n_cols, int64_t k_offset,
                                 shg_stream_t stream) {
    if (const int e = check_map_args("shg_line_bisector", stack, fit, planes, n_frames, height, width, bytes_per_px, frame_stride_px,
                                     half_width, shift, 2 * n_levels, plane_stride, row_pitch, n_cols, k_offset))
        return e;
    SHG_REQUIRE(levels && n_levels >= 1 && n_levels <= kMaxLevels, SHG_E_ARG, "shg_line_bisector: %d levels (1 to %d)", n_levels,
                kMaxLevels);
    for (int i = 0; i < n_levels; ++i)
        SHG_REQUIRE(isfinite(levels[i]) && levels[i] > 0.0 && levels[i] < 1.0 && (i == 0 || levels[i] > levels[i - 1]), SHG_E_ARG,
                    "shg_line_bisector: levels must be finite, strictly increasing and inside (0, 1) (level %d is %g)", i, levels[i]);
    const int64_t fstride = frame_stride_px > 0 ? frame_stride_px : height * width;
    MapArgs a{stack, (int)n_frames, height, width, fstride, fit, half_width, shift, planes, plane_stride, row_pitch, n_cols, k_offset,
              flip_x ? 1 : 0, n_levels, {}};
    for (int i = 0; i < n_levels; ++i) a.f[i] = levels[i];
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_bisector", st);
    return launch_map(
        a, bytes_per_px, st, [](auto t, auto vec) { return k_line_bisector_rot<decltype(t), decltype(vec)::value>; },
        [](auto t) { return k_line_bisector_plain<decltype(t)>; }, "k_line_bisector_rot", "k_line_bisector_plain");
}

namespace {
template <int K>
int launch_bisector_finish(int n_levels, const FinishArgs& a, hipStream_t st) {
    if (n_levels != K) return launch_bisector_finish<K - 1>(n_levels, a, st);
    return shg::launch(k_map_finish<2 * K, K>, dim3((unsigned)((a.nw + 255) / 256), (unsigned)a.out_h), dim3(256), 0, st, a,
                       "k_map_finish<2K, K>");
}

template <>
int launch_bisector_finish<0>(int, const FinishArgs&, hipStream_t) {
    return SHG_E_ARG;
}
}  // namespace

extern "C" int shg_line_bisector_finish(const float* raw, int64_t raw_plane_stride, int n_levels, int64_t h, int64_t w,
                                        int64_t raw_pitch, double h00, double h01, double h02, int64_t out_h, int64_t out_w,
                                        const double* circle3, const int64_t* crop4, float* maps, int64_t map_plane_stride,
                                        int64_t map_pitch, uint16_t* png, int64_t png_plane_stride, int64_t png_pitch, int half_width,
                                        double display_range, shg_stream_t stream) {
    SHG_REQUIRE(n_levels >= 1 && n_levels <= kMaxLevels, SHG_E_ARG, "shg_line_bisector_finish: %d levels (1 to %d)", n_levels,
                kMaxLevels);
    FinishArgs a{raw, raw_plane_stride, h, w, raw_pitch, h00, h01, h02, out_h, out_w, 0, 0.0, 0.0, 0.0, 0, 0, 0, 0, maps,
                 map_plane_stride, map_pitch, png, png_plane_stride, png_pitch, 0.0, 0.0, 0.0, 0.0};
    if (const int e = finish_args("shg_line_bisector_finish", 2 * n_levels, circle3, crop4, half_width, display_range, a)) return e;
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_bisector_finish", st);
    return launch_bisector_finish<kMaxLevels>(n_levels, a, st);
}
