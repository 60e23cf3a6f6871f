// Line-profile maps: the line core's position, its intensity, the line's width (FWHM), its centre of gravity and its equivalent
// width within the window, for every (slit row, frame) of a scan, and those five raw planes taken to the products' geometry.
// Not a reference stage: the arithmetic is the one include/shg_hip.h states and tests/lineprofile_ref.py restates in NumPy, bit for bit.
//
// k_line_profile_rot (rotated files): the walk of k_line_core_rot in doppler.hip (a lane owns eight slit rows, one 16-byte load per
// raw row, wave-uniform j over the band of the wave's 512 rows, eight rows in flight).  Walk 1 carries the vertex state, Σp, Σ(j - lo)p
// and p(lo) + p(hi); after it the half level is known, and walk 2 reads the same band again for the half-level crossings.  The wave
// has just read those rows (about 1 KiB per band row), so walk 2 is served on-die (L2, else the Infinity Cache): the profile samples
// do not fit in LDS at 8 waves (512 rows x up to 65 samples x 2 B per wave) nor in registers.  A workgroup is eight waves x two
// phases of eight frames (16 frames of the same 512 rows); each phase leaves through an LDS tile [5][8][512] as 32-byte runs of
// map rows, the two phases completing 64-byte runs in the same L2.  No atomics.
// k_line_profile_plain (un-rotated files): a wave is one slit row of 64 frames, each lane walks its window twice, stores coalesced.
// k_line_profile_finish: k_doppler_finish's arithmetic for all five planes of one output pixel in one thread, and the display planes.
// The helpers below restate doppler.hip's (anonymous namespace there): window_of with the shift S added, load_row8 unchanged.
#include "shg_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kPlanes = 5;                     // shift, core, width, cog, ew
constexpr int kMaxHalfWidth = 32;
constexpr int kRowsPerLane = 8;
constexpr int kTileRows = 64 * kRowsPerLane;   // slit rows of a workgroup
constexpr int kWaves = 8;
constexpr int kPhases = 2;                     // frames of a workgroup: kPhases x kWaves
constexpr int kTileFrames = kPhases * kWaves;
constexpr int kInFlight = 8;                   // raw rows a lane has loads in flight for

struct ProfileArgs {
    const void* stack;
    int n;
    int64_t height, width, fstride;            // file layout
    const double* fit;                         // [ih][4]
    int hw, shift;
    float* planes;
    int64_t plane_stride, pitch, n_cols, k_offset;
    int flip_x;
};

// Window of a slit row around fit[y][0] + S: lo > hi when the row has none (then every plane is NaN).
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

// Walk 1 of one slit row: the first minimum of p over [lo, hi] and the samples either side, Σp, Σ(j - lo) p and p(lo) + p(hi).
// Σ(j - lo) p <= 64 * 65 / 2 * 65535 < 2^31.
struct Walk1 {
    int best, jb, a, e, prev, sp, st, c2;
};

__device__ __forceinline__ void walk1_init(Walk1& s) {
    s.best = INT_MAX;
    s.jb = -2;
    s.a = s.e = s.prev = s.sp = s.st = s.c2 = 0;
}

__device__ __forceinline__ void walk1_step(Walk1& s, int j, int p, int lo, int hi) {
    if (j == s.jb + 1) s.e = p;
    if (j >= lo && j <= hi) {
        if (p < s.best) {
            s.best = p;
            s.jb = j;
            s.a = s.prev;
        }
        s.sp += p;
        s.st += (j - lo) * p;
        if (j == lo || j == hi) s.c2 += p;
    }
    s.prev = p;
}

// Walk 2 of one slit row: jl = the largest j in [lo, j*) with p(j) >= half, jr = the smallest j in (j*, hi] with p(j) >= half
// (p(j) >= half <=> p(j) >= thr = ceil(half) for integer p; thr = INT_MAX when the row has no width).  The sample pairs either
// side of a crossing are kept as p | p' << 16 (samples < 2^16).
struct Walk2 {
    int jl, jr, prev;
    uint32_t l, r;
};

__device__ __forceinline__ void walk2_init(Walk2& s) {
    s.jl = s.jr = -1;
    s.l = s.r = s.prev = 0;
}

__device__ __forceinline__ void walk2_step(Walk2& s, int j, int p, int lo, int hi, int jb, int thr) {
    if (j > lo && j <= jb && s.prev >= thr) {
        s.jl = j - 1;
        s.l = (uint32_t)s.prev | ((uint32_t)p << 16);    // p(jl), p(jl + 1)
    }
    if (j > jb && j <= hi && s.jr < 0 && p >= thr) {
        s.jr = j;
        s.r = (uint32_t)p | ((uint32_t)s.prev << 16);    // p(jr), p(jr - 1)
    }
    s.prev = p;
}

// The planes walk 1 decides (shift, core, cog, ew), and the half level of the width: see include/shg_hip.h.
struct Vertex {
    float shift, core, cog, ew;
    double half;
    int thr;                                   // INT_MAX: no width
};

__device__ __forceinline__ Vertex vertex_of(const Walk1& s, int lo, int hi, double ref) {
    const float nan = __builtin_nanf("");
    Vertex v{nan, nan, nan, nan, 0.0, INT_MAX};
    if (lo > hi) return v;
    const int64_t n = hi - lo + 1, c2 = s.c2;
    const int64_t s0 = n * c2 - 2 * (int64_t)s.sp;
    const int64_t sj = n * (int64_t)(lo + hi) / 2;                       // Σj over [lo, hi] (n (lo + hi) is even)
    const int64_t s1 = c2 * sj - 2 * ((int64_t)lo * s.sp + (int64_t)s.st);
    if (s0 > 0) v.cog = (float)((double)s1 / (double)s0 - ref);
    if (c2 != 0) v.ew = (float)((double)s0 / (double)c2);
    if (!(s.jb > lo && s.jb < hi)) return v;
    const int den = s.a + s.e - 2 * s.best;                              // > 0: a > b (first minimum), e >= b
    v.shift = (float)(((double)s.jb + (double)(s.a - s.e) / (double)(2 * den)) - ref);
    const int64_t d = s.a - s.e;
    const double core = (double)s.best - (double)(d * d) / (8.0 * (double)den);
    v.core = (float)core;
    v.half = 0.5 * (0.5 * (double)c2 + core);
    if ((double)s.best < v.half) v.thr = (int)ceil(v.half);             // |half| < 2^17
    return v;
}

__device__ __forceinline__ float width_of(const Walk2& s, double half, int thr) {
    if (thr == INT_MAX || s.jl < 0 || s.jr < 0) return __builtin_nanf("");
    const int pl = (int)(s.l & 0xffffu), pl1 = (int)(s.l >> 16), pr = (int)(s.r & 0xffffu), pr1 = (int)(s.r >> 16);
    const double xl = (double)s.jl + ((double)pl - half) / (double)(pl - pl1);
    const double xr = (double)s.jr - ((double)pr - half) / (double)(pr - pr1);
    return (float)(xr - xl);
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

// One walk of the band [wlo, whi] (wave-uniform) by a lane owning eight slit rows: rows outside the lane's [llo, lhi] read as 0.
template <typename T, bool VEC, typename Step>
__device__ __forceinline__ void walk_band(const char* frame, uint32_t rowb, uint32_t colb, int64_t x0, int64_t width, int wlo, int whi,
                                          int llo, int lhi, Step&& step) {
    constexpr int scale = sizeof(T) == 1 ? 256 : 1;                  // video_reader.py:121-122
    for (int j0 = wlo; j0 <= whi; j0 += kInFlight) {
        Row8 v[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int j = j0 + u;
            if (j <= whi && j >= llo && j <= lhi) {
                v[u] = load_row8<T, VEC>(frame, (uint32_t)j * rowb + colb, x0, width);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[u].w[q] = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int j = j0 + u;
            if (j > lhi) break;
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) step(j, r, (int)((v[u].w[r >> 1] >> (16 * (r & 1))) & 0xffffu) * scale);
        }
    }
}

// LDS tile [plane][frame of the phase][slit row]: row index XOR 4 x frame, so that the read-out (8 frames x 4 rows per 32 lanes)
// hits 32 banks and a lane's four consecutive rows stay one aligned float4.
__device__ __forceinline__ int tile_at(int q, int f, int row) { return (q * kWaves + f) * kTileRows + (row ^ (f << 2)); }

template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void k_line_profile_rot(const ProfileArgs a) {
    __shared__ float tile[kPlanes * kWaves * kTileRows];            // 80 KiB: two workgroups per CU
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t width = a.width;                                   // = ih
    const int iw = (int)a.height, hw = a.hw;
    const int64_t x0 = (int64_t)blockIdx.x * kTileRows + lane * kRowsPerLane;     // the lane's first raw column
    int lo[kRowsPerLane], hi[kRowsPerLane];
    int llo = INT_MAX, lhi = INT_MIN;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
        const int64_t x = x0 + r;
        const int64_t y = width - 1 - x;                            // a1: out[i, j] = raw[j, W - 1 - i]
        window_of(x < width ? a.fit[y * 4] : (double)NAN, a.shift, hw, iw, lo[r], hi[r]);
        if (lo[r] <= hi[r]) {
            llo = min(llo, lo[r]);
            lhi = max(lhi, hi[r]);
        }
    }
    int wlo = llo, whi = lhi;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        wlo = min(wlo, __shfl_xor(wlo, d));
        whi = max(whi, __shfl_xor(whi, d));
    }
    wlo = __builtin_amdgcn_readfirstlane(wlo);
    whi = __builtin_amdgcn_readfirstlane(whi);
    const uint32_t rowb = (uint32_t)(width * (int64_t)sizeof(T));   // (the entry point checks a frame's bytes < 4 GiB)
    const uint32_t colb = (uint32_t)(x0 * (int64_t)sizeof(T));
    for (int ph = 0; ph < kPhases; ++ph) {
        const int64_t kb = (int64_t)blockIdx.y * kTileFrames + ph * kWaves;
        const int64_t k = kb + wave;
        if (k < a.n) {
            const char* frame = static_cast<const char*>(a.stack) + k * a.fstride * (int64_t)sizeof(T);
            Walk1 s[kRowsPerLane];
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) walk1_init(s[r]);
            walk_band<T, VEC>(frame, rowb, colb, x0, width, wlo, whi, llo, lhi,
                              [&](int j, int r, int p) { walk1_step(s[r], j, p, lo[r], hi[r]); });
            double half[kRowsPerLane];
            int thr[kRowsPerLane], jb[kRowsPerLane];
#pragma unroll
            for (int h = 0; h < kRowsPerLane; h += 4) {
                Vertex v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t x = x0 + h + r;
                    const double ref = x < width ? a.fit[(width - 1 - x) * 4 + 3] + (double)a.shift : 0.0;
                    v[r] = vertex_of(s[h + r], lo[h + r], hi[h + r], ref);
                    half[h + r] = v[r].half;
                    thr[h + r] = v[r].thr;
                    jb[h + r] = s[h + r].jb;
                }
                const int row = lane * kRowsPerLane + h;
                *reinterpret_cast<float4*>(&tile[tile_at(0, wave, row)]) = make_float4(v[0].shift, v[1].shift, v[2].shift, v[3].shift);
                *reinterpret_cast<float4*>(&tile[tile_at(1, wave, row)]) = make_float4(v[0].core, v[1].core, v[2].core, v[3].core);
                *reinterpret_cast<float4*>(&tile[tile_at(3, wave, row)]) = make_float4(v[0].cog, v[1].cog, v[2].cog, v[3].cog);
                *reinterpret_cast<float4*>(&tile[tile_at(4, wave, row)]) = make_float4(v[0].ew, v[1].ew, v[2].ew, v[3].ew);
            }
            Walk2 t[kRowsPerLane];
#pragma unroll
            for (int r = 0; r < kRowsPerLane; ++r) walk2_init(t[r]);
            walk_band<T, VEC>(frame, rowb, colb, x0, width, wlo, whi, llo, lhi,
                              [&](int j, int r, int p) { walk2_step(t[r], j, p, lo[r], hi[r], jb[r], thr[r]); });
#pragma unroll
            for (int h = 0; h < kRowsPerLane; h += 4)
                *reinterpret_cast<float4*>(&tile[tile_at(2, wave, lane * kRowsPerLane + h)]) =
                    make_float4(width_of(t[h], half[h], thr[h]), width_of(t[h + 1], half[h + 1], thr[h + 1]),
                                width_of(t[h + 2], half[h + 2], thr[h + 2]), width_of(t[h + 3], half[h + 3], thr[h + 3]));
        }
        __syncthreads();
        // 8 threads write 8 consecutive columns of one map row of one plane
        for (int idx = threadIdx.x; idx < kPlanes * kTileRows * kWaves; idx += 64 * kWaves) {
            const int q = idx / (kTileRows * kWaves), rl = (idx / kWaves) % kTileRows, f = idx % kWaves;
            const int64_t x = (int64_t)blockIdx.x * kTileRows + rl, kf = kb + f;
            if (x < width && kf < a.n) {
                const int64_t c = a.k_offset + kf;
                a.planes[q * a.plane_stride + (width - 1 - x) * a.pitch + (a.flip_x ? a.n_cols - 1 - c : c)] = tile[tile_at(q, f, rl)];
            }
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kWaves) void k_line_profile_plain(const ProfileArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t y = (int64_t)blockIdx.y * kWaves + (threadIdx.x >> 6);
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    const int64_t ih = a.height;
    if (y >= ih || k >= a.n) return;
    constexpr int scale = sizeof(T) == 1 ? 256 : 1;
    int lo, hi;
    window_of(a.fit[y * 4], a.shift, a.hw, (int)a.width, lo, hi);
    const T* row = static_cast<const T*>(a.stack) + k * a.fstride + y * a.width;
    Walk1 s;
    walk1_init(s);
    for (int j = lo; j <= hi; ++j) walk1_step(s, j, (int)row[j] * scale, lo, hi);
    const Vertex v = vertex_of(s, lo, hi, a.fit[y * 4 + 3] + (double)a.shift);
    Walk2 t;
    walk2_init(t);
    for (int j = lo; j <= hi; ++j) walk2_step(t, j, (int)row[j] * scale, lo, hi, s.jb, v.thr);
    const int64_t c = a.k_offset + k;
    float* out = a.planes + y * a.pitch + (a.flip_x ? a.n_cols - 1 - c : c);
    out[0] = v.shift;
    out[a.plane_stride] = v.core;
    out[2 * a.plane_stride] = width_of(t, v.half, v.thr);
    out[3 * a.plane_stride] = v.cog;
    out[4 * a.plane_stride] = v.ew;
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
};

__global__ __launch_bounds__(256) void k_line_profile_finish(const FinishArgs a) {
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
            off = dx * dx + dy * dy > a.rad * a.rad;
        }
    }
#pragma unroll
    for (int q = 0; q < kPlanes; ++q) {
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
                const double e = q == 0 || q == 3 ? 32768.0 + (double)v * a.shift_scale
                                 : q == 1         ? (double)v
                                                  : 1.0 + (double)v * a.width_scale;
                d = (uint16_t)fmin(fmax(rint(e), 1.0), 65535.0);
            }
            a.png[q * a.png_plane + r * a.png_pitch + oc] = d;
        }
    }
}

}  // namespace

extern "C" int shg_line_profile(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                                int64_t frame_stride_px, const double* fit, int half_width, int shift, int flip_x, float* planes,
                                int64_t plane_stride, int64_t row_pitch, int64_t n_cols, int64_t k_offset, shg_stream_t stream) {
    SHG_REQUIRE(stack && fit && planes, SHG_E_ARG, "shg_line_profile: null pointer");
    SHG_REQUIRE(n_frames > 0 && height > 0 && width > 0, SHG_E_ARG, "shg_line_profile: empty input");
    SHG_REQUIRE(bytes_per_px == 1 || bytes_per_px == 2, SHG_E_ARG, "shg_line_profile: bytes_per_px must be 1 or 2");
    SHG_REQUIRE(half_width >= 1 && half_width <= kMaxHalfWidth, SHG_E_UNSUPPORTED, "shg_line_profile: half-width %d outside [1, %d]",
                half_width, kMaxHalfWidth);
    SHG_REQUIRE(n_frames < (1ll << 31) && n_cols < (1ll << 31), SHG_E_UNSUPPORTED, "shg_line_profile: %lld frames / %lld columns",
                (long long)n_frames, (long long)n_cols);
    SHG_REQUIRE(n_cols >= n_frames && k_offset >= 0 && k_offset + n_frames <= n_cols, SHG_E_ARG,
                "shg_line_profile: frames [%lld, %lld) do not fit %lld columns", (long long)k_offset, (long long)(k_offset + n_frames),
                (long long)n_cols);
    SHG_REQUIRE(row_pitch >= n_cols, SHG_E_ARG, "shg_line_profile: row_pitch < n_cols");
    SHG_REQUIRE(frame_stride_px == 0 || frame_stride_px >= height * width, SHG_E_ARG, "shg_line_profile: frame stride smaller than a frame");
    SHG_REQUIRE(height * width * bytes_per_px < (1ll << 32) && height < (1ll << 31) && width < (1ll << 31), SHG_E_UNSUPPORTED,
                "shg_line_profile: a frame of %lld x %lld samples is larger than 4 GiB", (long long)height, (long long)width);
    const bool rot = width > height;
    const int64_t ih = rot ? width : height, iw = rot ? height : width;
    SHG_REQUIRE(plane_stride >= ih * row_pitch, SHG_E_ARG, "shg_line_profile: plane stride < %lld x %lld", (long long)ih,
                (long long)row_pitch);
    // a line at a column in [0, iw) shifted by S has a window of three samples within [1, iw - 2] only when 3 - iw - H < S < iw - 3 + H
    SHG_REQUIRE(shift > 3 - iw - half_width && shift < iw - 3 + half_width, SHG_E_ARG,
                "shg_line_profile: shift %d puts every window outside columns [1, %lld]", shift, (long long)(iw - 2));
    const int64_t fstride = frame_stride_px > 0 ? frame_stride_px : height * width;
    ProfileArgs a{stack, (int)n_frames, height, width, fstride, fit, half_width, shift, planes, plane_stride, row_pitch, n_cols,
                  k_offset, flip_x ? 1 : 0};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_profile", st);
    if (rot) {
        // 16-byte pieces (8 for 8-bit samples) when every row of every frame starts on that boundary
        const int64_t piece = kRowsPerLane * bytes_per_px;
        const bool vec = (reinterpret_cast<uintptr_t>(stack) % piece) == 0 && (width * bytes_per_px) % piece == 0 &&
                         (fstride * bytes_per_px) % piece == 0;
        const dim3 grid((unsigned)((ih + kTileRows - 1) / kTileRows), (unsigned)((n_frames + kTileFrames - 1) / kTileFrames));
        if (bytes_per_px == 2)
            return vec ? shg::launch(k_line_profile_rot<uint16_t, true>, grid, dim3(64 * kWaves), 0, st, a, "k_line_profile_rot")
                       : shg::launch(k_line_profile_rot<uint16_t, false>, grid, dim3(64 * kWaves), 0, st, a, "k_line_profile_rot");
        return vec ? shg::launch(k_line_profile_rot<uint8_t, true>, grid, dim3(64 * kWaves), 0, st, a, "k_line_profile_rot")
                   : shg::launch(k_line_profile_rot<uint8_t, false>, grid, dim3(64 * kWaves), 0, st, a, "k_line_profile_rot");
    }
    const dim3 grid((unsigned)((n_frames + 63) / 64), (unsigned)((ih + kWaves - 1) / kWaves));
    if (bytes_per_px == 2) return shg::launch(k_line_profile_plain<uint16_t>, grid, dim3(64 * kWaves), 0, st, a, "k_line_profile_plain");
    return shg::launch(k_line_profile_plain<uint8_t>, grid, dim3(64 * kWaves), 0, st, a, "k_line_profile_plain");
}

extern "C" int shg_line_profile_finish(const float* raw, int64_t raw_plane_stride, int64_t h, int64_t w, int64_t raw_pitch, double h00,
                                       double h01, double h02, int64_t out_h, int64_t out_w, const double* circle3, const int64_t* crop4,
                                       float* maps, int64_t map_plane_stride, int64_t map_pitch, uint16_t* png, int64_t png_plane_stride,
                                       int64_t png_pitch, int half_width, double display_range, shg_stream_t stream) {
    SHG_REQUIRE(raw && maps, SHG_E_ARG, "shg_line_profile_finish: null pointer");
    SHG_REQUIRE(h > 0 && w > 0 && raw_pitch >= w && raw_plane_stride >= h * raw_pitch && out_h > 0 && out_w > 0, SHG_E_ARG,
                "shg_line_profile_finish: empty or mis-pitched input");
    SHG_REQUIRE(out_h < (1ll << 31), SHG_E_UNSUPPORTED, "shg_line_profile_finish: %lld output rows", (long long)out_h);
    int64_t nw = out_w, lo = 0, dx0 = 0, n = out_w;
    if (crop4) {
        nw = crop4[0];
        lo = crop4[1];
        dx0 = crop4[2];
        n = crop4[3];
        SHG_REQUIRE(nw > 0 && lo >= 0 && dx0 >= 0 && n >= 0 && dx0 + n <= nw && lo + n <= out_w, SHG_E_ARG,
                    "shg_line_profile_finish: crop (%lld, %lld, %lld, %lld) does not fit %lld columns", (long long)nw, (long long)lo,
                    (long long)dx0, (long long)n, (long long)out_w);
    }
    SHG_REQUIRE(map_pitch >= nw && map_plane_stride >= out_h * map_pitch, SHG_E_ARG, "shg_line_profile_finish: map pitch < %lld",
                (long long)nw);
    SHG_REQUIRE(!png || (png_pitch >= nw && png_plane_stride >= out_h * png_pitch), SHG_E_ARG,
                "shg_line_profile_finish: display pitch < %lld", (long long)nw);
    SHG_REQUIRE(!png || (isfinite(display_range) && display_range > 0.0), SHG_E_ARG,
                "shg_line_profile_finish: display range must be positive");
    SHG_REQUIRE(!png || (half_width >= 1 && half_width <= kMaxHalfWidth), SHG_E_UNSUPPORTED,
                "shg_line_profile_finish: half-width %d outside [1, %d]", half_width, kMaxHalfWidth);
    const bool masked = circle3 && !(circle3[0] == -1.0 && circle3[1] == -1.0 && circle3[2] == -1.0);
    FinishArgs a{raw, raw_plane_stride, h, w, raw_pitch, h00, h01, h02, out_h, out_w, masked ? 1 : 0, masked ? circle3[0] : 0.0,
                 masked ? circle3[1] : 0.0, masked ? circle3[2] : 0.0, nw, lo, dx0, n, maps, map_plane_stride, map_pitch, png,
                 png_plane_stride, png_pitch, png ? 32767.0 / display_range : 0.0, png ? 65534.0 / (double)(2 * half_width + 1) : 0.0};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_profile_finish", st);
    return shg::launch(k_line_profile_finish, dim3((unsigned)((nw + 255) / 256), (unsigned)out_h), dim3(256), 0, st, a,
                       "k_line_profile_finish");
}
