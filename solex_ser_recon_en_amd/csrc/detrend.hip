// Removing a fitted plane from a finished line map (shg_map_plane_moments, shg_map_detrend).  Not a reference stage: the arithmetic is
// the one include/shg_hip.h states, restated in NumPy by tests/detrend_ref.py.  The fit itself is the host's (linemaps.py): the GPU
// gathers the ten integer moments of the used pixels in one streaming read, and subtracts the plane in one read and two writes.
#include "image_args.h"

#include <math.h>
#include <stdlib.h>

namespace {

constexpr int kThreads = 256;
constexpr int kQuad = 4;                        // columns a thread owns
constexpr int kChunk = kThreads * kQuad;        // columns a workgroup spans
constexpr int kInFlight = 8;                    // rows a thread loads before it folds them
constexpr int kMaxDim = 8192;
constexpr int kMaxBandRows = 4096;              // rows of one workgroup: a column's sum of q stays below 2^12 * 2^18 = 2^30
constexpr int kTargetGroups = 512;              // workgroups a launch aims at (SHG_MOMENTS_GROUPS in the environment: another count)

struct MomentArgs {
    const float* map;
    int h, w;
    int64_t pitch;
    int masked;
    double cx, cy, rad2;
    int clipped;
    double a, b, g, limit;
    int band;                                   // rows a workgroup folds
    unsigned long long* out;                    // moments10, zeroed before the launch
};

// The column of a thread's j-th element: with 16-byte loads four neighbours, else four columns a workgroup's width apart (each load
// of a wave then reads 256 consecutive bytes).
template <bool VEC>
__device__ __forceinline__ int column_of(int j) {
    const int base = blockIdx.x * kChunk;
    return VEC ? base + (int)threadIdx.x * kQuad + j : base + j * kThreads + (int)threadIdx.x;
}

// Row `row` of the thread's four columns; NaN (never used, never stored) for a column at or beyond w.  The 16-byte load only where
// all four columns exist: the last row of a buffer may end at column w.
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* row, int w, float (&v)[kQuad]) {
    const int c0 = column_of<VEC>(0);
    if (VEC && c0 + kQuad <= w) {
        const float4 q = *reinterpret_cast<const float4*>(row + c0);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
        const int c = column_of<VEC>(j);
        v[j] = c < w ? row[c] : __builtin_nanf("");
    }
}

// One workgroup: columns [blockIdx.x * 1024, + 1024) of the rows [blockIdx.y * band, + band).  A thread's columns are fixed, so what
// depends on the column alone -- (c - cx)^2 and a + b c -- is computed once, and the sums over c come from per-column sums at the
// end: per pixel the thread adds to n, sum r and sum q of the column (32 bits each: a band has at most 4096 rows, |q| <= 2^18) and
// to sum q^2 (one 64-bit multiply-add); sum r^2 and sum q r take one multiply-add a row.  Every sum is an integer: the order of the
// additions, here and across the workgroups, cannot change a bit.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_plane_moments(const MomentArgs a) {
    int c[kQuad];
    double dx2[kQuad], abc[kQuad];
    uint32_t n[kQuad], sr[kQuad];
    int32_t sq[kQuad];
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
        c[j] = column_of<VEC>(j);
        const double dx = (double)c[j] - a.cx;
        dx2[j] = dx * dx;
        abc[j] = a.a + a.b * (double)c[j];
        n[j] = sr[j] = 0;
        sq[j] = 0;
    }
    uint64_t srr = 0;
    int64_t sqr = 0, sqq = 0;
    const int r0 = blockIdx.y * a.band, r1 = min(r0 + a.band, a.h);
    if (c[0] < a.w) {                            // (VEC: the quad's first column; else the thread's leftmost)
        for (int rb = r0; rb < r1; rb += kInFlight) {
            float v[kInFlight][kQuad];
#pragma unroll
            for (int i = 0; i < kInFlight; ++i) {
                if (rb + i < r1) {
                    load_quad<VEC>(a.map + (int64_t)(rb + i) * a.pitch, a.w, v[i]);
                } else {
#pragma unroll
                    for (int j = 0; j < kQuad; ++j) v[i][j] = __builtin_nanf("");
                }
            }
#pragma unroll
            for (int i = 0; i < kInFlight; ++i) {
                const int r = rb + i;            // (a row at or beyond r1 holds NaN only: nothing is added for it)
                const double dy = (double)r - a.cy, dy2 = dy * dy, gr = a.g * (double)r;
                uint32_t in_row = 0;
                int32_t q_row = 0;
#pragma unroll
                for (int j = 0; j < kQuad; ++j) {
                    const float x = v[i][j];
                    bool used = fabsf(x) < 64.0f;                              // false for NaN and the infinities
                    if (a.masked) used = used && !(dx2[j] + dy2 > a.rad2);
                    if (a.clipped) used = used && fabs((double)x - (abc[j] + gr)) <= a.limit;
                    // x * 4096 is exact in float32 as it is in float64 (a power of two, |x| < 64), so rintf gives the header's q
                    const int32_t q = used ? (int32_t)rintf(x * 4096.0f) : 0;
                    n[j] += used;
                    sr[j] += used ? (uint32_t)r : 0u;
                    sq[j] += q;
                    in_row += used;
                    q_row += q;
                    sqq += (int64_t)q * q;
                }
                srr += (uint64_t)((uint32_t)r * (uint32_t)r) * in_row;
                sqr += (int64_t)q_row * r;
            }
        }
    }
    uint64_t m[10] = {0, 0, 0, 0, 0, srr, 0, 0, (uint64_t)sqr, (uint64_t)sqq};
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
        const uint64_t cj = (uint64_t)c[j];
        m[0] += n[j];
        m[1] += cj * n[j];
        m[2] += sr[j];
        m[3] += cj * cj * n[j];
        m[4] += cj * sr[j];
        m[6] += (uint64_t)(int64_t)sq[j];
        m[7] += (uint64_t)((int64_t)c[j] * (int64_t)sq[j]);
    }
    __shared__ uint64_t part[kThreads / shg::kWave][10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const uint64_t t = shg::wave_sum(m[k]);
        if (shg::lane_id() == 0) part[threadIdx.x / shg::kWave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 10) {                      // one atomic instruction a workgroup: ten lanes, ten neighbouring slots
        uint64_t t = 0;
#pragma unroll
        for (int wv = 0; wv < kThreads / shg::kWave; ++wv) t += part[wv][threadIdx.x];
        if (t) atomicAdd(a.out + threadIdx.x, (unsigned long long)t);
    }
}

struct DetrendArgs {
    const float* map;
    int h, w;
    int64_t pitch;
    double a, b, g;
    float* out;
    int64_t out_pitch;
    uint16_t* png;
    int64_t png_pitch;
    double scale;                               // 32767 / display_range
    int rows;                                   // rows a workgroup handles
};

// The same column ownership; an element is read and written by one thread, so out may be map.  VEC: 16-byte loads and stores of the
// map and the output and 8-byte stores of the display plane, for the quads that lie inside the row; else element by element.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_map_detrend(const DetrendArgs a) {
    double abc[kQuad];
#pragma unroll
    for (int j = 0; j < kQuad; ++j) abc[j] = a.a + a.b * (double)column_of<VEC>(j);
    const int c0 = column_of<VEC>(0);
    if (c0 >= a.w) return;
    const bool whole = VEC && c0 + kQuad <= a.w;
    const int r0 = blockIdx.y * a.rows, r1 = min(r0 + a.rows, a.h);
    for (int r = r0; r < r1; ++r) {
        float v[kQuad];
        load_quad<VEC>(a.map + (int64_t)r * a.pitch, a.w, v);
        const double gr = a.g * (double)r;
        uint16_t d[kQuad];
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
            v[j] = (float)((double)v[j] - (abc[j] + gr));
            d[j] = isnan(v[j]) ? (uint16_t)0 : (uint16_t)fmin(fmax(rint(32768.0 + (double)v[j] * a.scale), 1.0), 65535.0);
        }
        float* orow = a.out + (int64_t)r * a.out_pitch;
        uint16_t* prow = a.png ? a.png + (int64_t)r * a.png_pitch : nullptr;
        if (whole) {
            *reinterpret_cast<float4*>(orow + c0) = make_float4(v[0], v[1], v[2], v[3]);
            if (prow) *reinterpret_cast<ushort4*>(prow + c0) = make_ushort4(d[0], d[1], d[2], d[3]);
        } else {
#pragma unroll
            for (int j = 0; j < kQuad; ++j) {
                const int c = column_of<VEC>(j);
                if (c < a.w) {
                    orow[c] = v[j];
                    if (prow) prow[c] = d[j];
                }
            }
        }
    }
}

int check_map(const char* fn, const void* map, int64_t h, int64_t w, int64_t pitch) {
    SHG_REQUIRE(map, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(h >= 1 && h <= kMaxDim && w >= 1 && w <= kMaxDim, SHG_E_UNSUPPORTED, "%s: a map of %lld x %lld (1 to %d either way)", fn,
                (long long)h, (long long)w, kMaxDim);
    SHG_REQUIRE(pitch >= w, SHG_E_ARG, "%s: pitch < w", fn);
    return 0;
}

int round_up(int64_t v, int to) { return (int)((v + to - 1) / to * to); }

}  // namespace

extern "C" int shg_map_plane_moments(const float* map, int64_t h, int64_t w, int64_t pitch, const double* circle3, const double* prev4,
                                     int64_t* moments10, shg_stream_t stream) {
    if (const int e = check_map("shg_map_plane_moments", map, h, w, pitch)) return e;
    SHG_REQUIRE(moments10, SHG_E_ARG, "shg_map_plane_moments: null pointer");
    MomentArgs a{map, (int)h, (int)w, pitch, 0, 0.0, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0, reinterpret_cast<unsigned long long*>(moments10)};
    if (prev4) {
        SHG_REQUIRE(isfinite(prev4[0]) && isfinite(prev4[1]) && isfinite(prev4[2]), SHG_E_ARG,
                    "shg_map_plane_moments: the previous plane (%g, %g, %g) is not finite", prev4[0], prev4[1], prev4[2]);
        SHG_REQUIRE(prev4[3] >= 0.0, SHG_E_ARG, "shg_map_plane_moments: limit %g is negative or NaN", prev4[3]);
        a.clipped = 1;
        a.a = prev4[0], a.b = prev4[1], a.g = prev4[2], a.limit = prev4[3];
    }
    a.masked = circle3 && !(circle3[0] == -1.0 && circle3[1] == -1.0 && circle3[2] == -1.0);
    if (a.masked) a.cx = circle3[0], a.cy = circle3[1], a.rad2 = circle3[2] * circle3[2];
    const int gx = (int)((w + kChunk - 1) / kChunk);
    int target = kTargetGroups;
    if (const char* s = getenv("SHG_MOMENTS_GROUPS")) target = atoi(s) > 0 ? atoi(s) : target;
    const int64_t band = round_up((h * gx + target - 1) / target, kInFlight);
    a.band = (int)(band > kMaxBandRows ? kMaxBandRows : band);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("map_plane_moments", st);
    if (const int e = shg::zero_async("shg_map_plane_moments", moments10, 10 * sizeof(int64_t), st)) return e;
    const dim3 grid((unsigned)gx, (unsigned)((h + a.band - 1) / a.band));
    return shg::launch(shg::rows_aligned(map, pitch, sizeof(float), 16) ? k_plane_moments<true> : k_plane_moments<false>, grid, dim3(kThreads), 0,
                       st, a, "k_plane_moments");
}

extern "C" int shg_map_detrend(const float* map, int64_t h, int64_t w, int64_t pitch, const double* plane3, float* out, int64_t out_pitch,
                               uint16_t* png, int64_t png_pitch, double display_range, shg_stream_t stream) {
    if (const int e = check_map("shg_map_detrend", map, h, w, pitch)) return e;
    SHG_REQUIRE(plane3 && out, SHG_E_ARG, "shg_map_detrend: null pointer");
    SHG_REQUIRE(out_pitch >= w && (!png || png_pitch >= w), SHG_E_ARG, "shg_map_detrend: output pitch < w");
    SHG_REQUIRE(isfinite(plane3[0]) && isfinite(plane3[1]) && isfinite(plane3[2]), SHG_E_ARG,
                "shg_map_detrend: the plane (%g, %g, %g) is not finite", plane3[0], plane3[1], plane3[2]);
    SHG_REQUIRE(!png || (isfinite(display_range) && display_range > 0.0), SHG_E_ARG, "shg_map_detrend: display range must be positive");
    SHG_REQUIRE(out != map || out_pitch == pitch, SHG_E_ARG, "shg_map_detrend: in place needs equal pitches");
    constexpr int kRows = 4;
    DetrendArgs a{map, (int)h, (int)w, pitch, plane3[0], plane3[1], plane3[2], out, out_pitch, png, png_pitch,
                  png ? 32767.0 / display_range : 0.0, kRows};
    const bool vec = shg::rows_aligned(map, pitch, sizeof(float), 16) && shg::rows_aligned(out, out_pitch, sizeof(float), 16) &&
                     (!png || (reinterpret_cast<uintptr_t>(png) % 8 == 0 && png_pitch % 4 == 0));
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("map_detrend", st);
    const dim3 grid((unsigned)((w + kChunk - 1) / kChunk), (unsigned)((h + kRows - 1) / kRows));
    return shg::launch(vec ? k_map_detrend<true> : k_map_detrend<false>, grid, dim3(kThreads), 0, st, a, "k_map_detrend");
}
