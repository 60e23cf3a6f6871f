// Sharpening a disk: the undecimated B3-spline wavelet layers of a 16-bit image recombined with one gain and one soft noise gate a
// layer (shg_wavelet_sharpen_u16), and the lower median of |w_1| over the disk that the gates are sized by (shg_wavelet_noise_u16).
// Not a reference stage: the arithmetic is the one include/shg_hip.h states, all of it integers, restated in NumPy by
// tests/sharpen_ref.py.
//
// Sharpen.
//   k_wavelet_fused<NL>   levels 1 .. NL = min(L, 3) in one launch.  A workgroup owns 64 x 32 outputs; the tile with its halo of
//                         2 (2^NL - 1) pixels (14 for three levels: 92 x 60 words, 22 KB) sits in LDS as c_0, and every level
//                         replaces it in place by c_j on a region 2 holes narrower on every side: a row pass into a second array of
//                         the same geometry, a barrier, a column pass back, a barrier.  The halo is loaded through the reflection,
//                         and that is enough for every level: the symmetric extension of c_(j-1) filtered by a symmetric kernel
//                         is the symmetric extension of c_j, so a c_j computed at a position beyond the border equals c_j at the
//                         reflected position.  A thread keeps the eight pixels it owns (one column, every fourth row) in registers
//                         from level to level: w_j = the value before - the value after, gated, times the gain, into a 64-bit sum.
//                         L <= 3: the launch writes the output.  Otherwise it leaves c_3 and the sum in the workspace.
//   k_wavelet_level       one launch a deeper level (holes 8, 16, 32): a thread a pixel, the 25 taps as five coalesced reads in each
//                         of five rows of the c plane before it, which the caches serve; it carries the sum forward, or -- the last
//                         one -- writes the output.  Two c planes take turns.
// Without `planes` no w_j reaches memory.  Nothing accumulates across threads: every pixel is written once, by one thread.
//
// Noise: a two-level radix select of the 22-bit |w_1| over the on-disk pixels, 11 bits a level, over two tables of 2048 32-bit counts.
//   hipMemsetAsync          both tables
//   k_noise_hist<false>     T0[|w_1| >> 11] += 1.  A workgroup walks 64 x 16 tiles: w_1 from the image (halo 2, uint16 in LDS),
//                           counted in LDS; at its end it adds the non-zero counters to the table with integer atomics
//   k_noise_pick<false>     one workgroup: n, the bin that holds rank (n - 1) / 2, the rank left inside it
//   k_noise_hist<true>      T1[|w_1| & 2047] += 1 where |w_1| >> 11 is that bin
//   k_noise_pick<true>      the median and n
// Everything accumulated is an integer count: neither the grid nor the order of the atomics can change a bit.
#include "image_args.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = 6;
constexpr int kFusedLevels = 3;
constexpr int kMaxGain = 4096;
constexpr int kMaxThreshold = 1 << 22;
constexpr int kTW = 64, kTH = 32;                 // the fused kernel's tile; a thread owns column threadIdx.x % 64 of rows threadIdx.x / 64 + 4 i
constexpr int kOwned = kTW * kTH / kThreads;
constexpr int kRowStep = kThreads / kTW;
constexpr int kBins = 2048;                       // 11 bits a level of the select
constexpr size_t kNoiseBytes = 2 * kBins * sizeof(uint32_t) + 256;       // T0 | T1 | the state {bin, rank left, n}
constexpr uint32_t kNoBin = 0xFFFFFFFFu;          // the "bin" of an empty set: no value has it

// R(i, n) of the header.  The extension is symmetric about 0, so |i| stands for i; only an index beyond the far border divides.
__device__ __forceinline__ int reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) {
        const int p = 2 * (n - 1);
        if (p == 0) return 0;
        i %= p;
        if (i >= n) i = p - i;
    }
    return i;
}

__device__ __forceinline__ int soft(int w, int t) {
    const int m = max(abs(w) - t, 0);
    return w < 0 ? -m : m;
}

__device__ __forceinline__ uint16_t finish(long long acc) {
    const long long q = (acc + 8192) >> 14;
    return (uint16_t)(q < 0 ? 0 : q > 65535 ? 65535 : q);
}

struct FusedArgs {
    const uint16_t* img;
    int h, w;
    int64_t pitch;
    int levels;                       // L; the launch runs min(L, 3) of them
    int gain[kFusedLevels], thr[kFusedLevels];
    uint16_t* out;                    // L <= 3
    int64_t out_pitch;
    int32_t* planes;                  // NULL, or [L + 1][h][w]
    int32_t* c_next;                  // L > 3: c_3, [h][w]
    long long* acc;                   // L > 3: the sum so far, [h][w]
};

// One level inside the tile: A holds c_(j-1) on the region E_IN pixels wider than the tile on every side, and afterwards c_j on the
// region E_IN - 2 HOLE wider.  Both arrays have the geometry of the widest region (E0).
template <int E0, int E_IN, int HOLE>
__device__ __forceinline__ void fused_level(int32_t* A, int32_t* T) {
    constexpr int AW = kTW + 2 * E0, E_OUT = E_IN - 2 * HOLE;
    constexpr int rows_in = kTH + 2 * E_IN, rows_out = kTH + 2 * E_OUT, cols_out = kTW + 2 * E_OUT;
    constexpr int first_in = E0 - E_IN, first_out = E0 - E_OUT;
    static_assert(E_OUT >= 0, "halo");
    for (int i = threadIdx.x; i < rows_in * cols_out; i += kThreads) {
        const int at = (first_in + i / cols_out) * AW + first_out + i % cols_out;
        const int32_t* p = A + at;
        T[at] = (p[-2 * HOLE] + p[2 * HOLE]) + 4 * (p[-HOLE] + p[HOLE]) + 6 * p[0];                          // < 2^26
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows_out * cols_out; i += kThreads) {
        const int at = (first_out + i / cols_out) * AW + first_out + i % cols_out;
        const int32_t* p = T + at;
        const int32_t s = (p[-2 * HOLE * AW] + p[2 * HOLE * AW]) + 4 * (p[-HOLE * AW] + p[HOLE * AW]) + 6 * p[0];    // < 2^30
        A[at] = (s + 128) >> 8;
    }
    __syncthreads();
}

template <int NL>
__global__ __launch_bounds__(kThreads) void k_wavelet_fused(const FusedArgs a) {
    constexpr int E0 = 2 * ((1 << NL) - 1), AW = kTW + 2 * E0, AH = kTH + 2 * E0;
    __shared__ int32_t A[AH * AW];
    __shared__ int32_t T[AH * AW];
    const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
    for (int i = threadIdx.x; i < AH * AW; i += kThreads) {
        const int gr = reflect(ty0 - E0 + i / AW, a.h), gc = reflect(tx0 - E0 + i % AW, a.w);
        A[i] = 64 * (int32_t)a.img[(int64_t)gr * a.pitch + gc];
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % kTW, ly = (int)threadIdx.x / kTW, c = tx0 + lx;
    const int64_t plane = (int64_t)a.h * a.w;
    int32_t prev[kOwned];
    long long acc[kOwned];
#pragma unroll
    for (int i = 0; i < kOwned; ++i) {
        prev[i] = A[(E0 + ly + i * kRowStep) * AW + E0 + lx];
        acc[i] = 0;
    }
    // what level j (0-based) left in A, taken into the threads' own pixels
    auto absorb = [&](int j) {
#pragma unroll
        for (int i = 0; i < kOwned; ++i) {
            const int r = ty0 + ly + i * kRowStep;
            const int32_t cj = A[(E0 + ly + i * kRowStep) * AW + E0 + lx], wj = prev[i] - cj;
            if (a.planes && c < a.w && r < a.h) a.planes[j * plane + (int64_t)r * a.w + c] = wj;
            acc[i] += (long long)a.gain[j] * soft(wj, a.thr[j]);
            prev[i] = cj;
        }
    };
    fused_level<E0, E0, 1>(A, T);
    absorb(0);
    if constexpr (NL >= 2) {
        fused_level<E0, E0 - 2, 2>(A, T);
        absorb(1);
    }
    if constexpr (NL >= 3) {
        fused_level<E0, E0 - 6, 4>(A, T);
        absorb(2);
    }
    if (c >= a.w) return;
#pragma unroll
    for (int i = 0; i < kOwned; ++i) {
        const int r = ty0 + ly + i * kRowStep;
        if (r >= a.h) continue;
        const int64_t at = (int64_t)r * a.w + c;
        if (a.levels == NL) {
            a.out[(int64_t)r * a.out_pitch + c] = finish(acc[i] + 256ll * prev[i]);
            if (a.planes) a.planes[NL * plane + at] = prev[i];
        } else {
            a.c_next[at] = prev[i];
            a.acc[at] = acc[i];
        }
    }
}

struct LevelArgs {
    const int32_t* c_in;              // c_(j-1), [h][w]
    int32_t* c_out;                   // c_j for the next launch (NULL: this is the last level)
    long long* acc;
    int h, w, hole, gain, thr, j;     // j: 0-based
    uint16_t* out;                    // the last level
    int64_t out_pitch;
    int32_t* planes;
    int levels;
};

__global__ __launch_bounds__(kThreads) void k_wavelet_level(const LevelArgs a) {
    const int c = blockIdx.x * kTW + (int)threadIdx.x % kTW, r = blockIdx.y * kRowStep + (int)threadIdx.x / kTW;
    if (c >= a.w || r >= a.h) return;
    int col[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) col[l] = reflect(c + (l - 2) * a.hole, a.w);
    int32_t s = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int32_t* row = a.c_in + (int64_t)reflect(r + (k - 2) * a.hole, a.h) * a.w;
        const int32_t t = (row[col[0]] + row[col[4]]) + 4 * (row[col[1]] + row[col[3]]) + 6 * row[col[2]];
        s += (k == 0 || k == 4 ? 1 : k == 2 ? 6 : 4) * t;
    }
    const int64_t at = (int64_t)r * a.w + c, plane = (int64_t)a.h * a.w;
    const int32_t cj = (s + 128) >> 8, wj = a.c_in[at] - cj;
    const long long acc = a.acc[at] + (long long)a.gain * soft(wj, a.thr);
    if (a.planes) a.planes[a.j * plane + at] = wj;
    if (a.c_out) {
        a.c_out[at] = cj;
        a.acc[at] = acc;
    } else {
        a.out[(int64_t)r * a.out_pitch + c] = finish(acc + 256ll * cj);
        if (a.planes) a.planes[a.levels * plane + at] = cj;
    }
}

// ---- noise ----
constexpr int kNW = 64, kNH = 16;
constexpr int kNoiseOwned = kNW * kNH / kThreads;
constexpr int kNoiseBlocks = 1024;               // workgroups of a histogram launch: each walks its tiles and adds its counters once

struct NoiseArgs {
    const uint16_t* img;
    int h, w;
    int64_t pitch;
    int masked;
    double cx, cy, rad2;
    uint32_t* table;                  // first pass: T0; second pass: T1
    const uint32_t* state;            // second pass: what k_noise_pick<false> left
    int tiles_x, tiles;
};

template <bool SECOND>
__global__ __launch_bounds__(kThreads) void k_noise_hist(const NoiseArgs a) {
    constexpr int LW = kNW + 4, LH = kNH + 4;
    __shared__ uint16_t tile[LH * LW];
    __shared__ uint32_t cnt[kBins];
    uint32_t wanted = 0;
    if (SECOND) {
        wanted = a.state[0];
        if (wanted == kNoBin) return;             // an empty set
    }
    for (int i = threadIdx.x; i < kBins; i += kThreads) cnt[i] = 0;
    const int lx = (int)threadIdx.x % kNW, ly = (int)threadIdx.x / kNW;
    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int tx0 = (t % a.tiles_x) * kNW, ty0 = (t / a.tiles_x) * kNH, c = tx0 + lx;
        const double dx = (double)c - a.cx, dx2 = dx * dx;
        bool on[kNoiseOwned];
        int any = 0;
#pragma unroll
        for (int i = 0; i < kNoiseOwned; ++i) {
            const int r = ty0 + ly + i * kRowStep;
            bool ok = c < a.w && r < a.h;
            if (ok && a.masked) {
                const double dy = (double)r - a.cy, d2 = dx2 + dy * dy;
                ok = !(d2 > a.rad2);
            }
            on[i] = ok;
            any |= ok ? 1 : 0;
        }
        // (a barrier too: the tile of the round before has been read by everyone, and the counters are clear before their first use)
        if (!__syncthreads_or(any)) continue;     // no pixel of the tile is in the set
        for (int i = threadIdx.x; i < LH * LW; i += kThreads)
            tile[i] = a.img[(int64_t)reflect(ty0 - 2 + i / LW, a.h) * a.pitch + reflect(tx0 - 2 + i % LW, a.w)];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kNoiseOwned; ++i) {
            if (!on[i]) continue;
            const uint16_t* p = tile + (ly + i * kRowStep) * LW + lx;      // the tap (0, 0); the pixel itself is p[2 * LW + 2]
            int32_t s = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint16_t* q = p + k * LW;
                const int32_t row = ((int32_t)q[0] + q[4]) + 4 * ((int32_t)q[1] + q[3]) + 6 * (int32_t)q[2];
                s += (k == 0 || k == 4 ? 1 : k == 2 ? 6 : 4) * row;
            }
            // c_0 = 64 img and the sum is linear: S = 64 s, below 2^30
            const int32_t c1 = (64 * s + 128) >> 8;
            const uint32_t m = (uint32_t)abs(64 * (int32_t)p[2 * LW + 2] - c1);
            if (!SECOND) atomicAdd(&cnt[m >> 11], 1u);
            else if ((m >> 11) == wanted) atomicAdd(&cnt[m & (kBins - 1)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kThreads)
        if (cnt[i]) atomicAdd(a.table + i, cnt[i]);
}

struct PickArgs {
    const uint32_t* tables;           // T0 | T1
    uint32_t* state;                  // {the high bin, the rank left in it, n}
    unsigned long long* out2;
};

// One workgroup: eight bins a thread, a prefix sum over the wave and the four waves' totals through LDS.
template <bool LOW>
__global__ __launch_bounds__(kThreads) void k_noise_pick(const PickArgs a) {
    static_assert(kBins == 8 * kThreads, "eight bins a thread");
    __shared__ uint32_t wave_total[kThreads / shg::kWave];
    const uint32_t* t = a.tables + (LOW ? kBins : 0);
    const int tid = threadIdx.x, wave = tid / shg::kWave;
    const uint4 lo4 = reinterpret_cast<const uint4*>(t)[2 * tid], hi4 = reinterpret_cast<const uint4*>(t)[2 * tid + 1];
    const uint32_t b[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += b[k];
    const uint32_t incl = (uint32_t)shg::wave_scan((int)s);              // (an image holds at most 2^28 pixels)
    if (shg::lane_id() == shg::kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = incl - s, total = 0;
#pragma unroll
    for (int v = 0; v < kThreads / shg::kWave; ++v) {
        if (v < wave) before += wave_total[v];
        total += wave_total[v];
    }
    uint32_t n, rank;
    if (!LOW) {
        n = total;
        if (n == 0) {
            if (tid == 0) a.state[0] = kNoBin, a.state[1] = 0, a.state[2] = 0;
            return;
        }
        rank = (n - 1) / 2;
    } else {
        n = a.state[2];
        if (n == 0) {
            if (tid == 0) a.out2[0] = 0, a.out2[1] = 0;
            return;
        }
        rank = a.state[1];
    }
    if (!(before <= rank && rank < before + s)) return;
    uint32_t bin = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        if (bin == (uint32_t)k && rank >= before + b[k]) before += b[k], bin = k + 1;
    }
    bin += 8 * (uint32_t)tid;
    if (!LOW) {
        a.state[0] = bin, a.state[1] = rank - before, a.state[2] = n;
    } else {
        a.out2[0] = (unsigned long long)(a.state[0] << 11 | bin);
        a.out2[1] = n;
    }
}

// ---- host ----
using shg::overlap;
using shg::Span;
using shg::span_of;

// the planes the launches of an L-level call hand each other: the 64-bit sum and one or two c planes, beyond three levels
size_t carried_bytes(int64_t h, int64_t w, int levels) {
    if (levels <= kFusedLevels) return 0;
    const size_t px = (size_t)h * (size_t)w;
    return px * sizeof(long long) + px * sizeof(int32_t) * (levels == kFusedLevels + 1 ? 1 : 2);
}

size_t workspace_bytes(int64_t h, int64_t w, int levels) { return shg::kWorkspaceAlign + kNoiseBytes + carried_bytes(h, w, levels); }

}  // namespace

extern "C" size_t shg_wavelet_workspace_bytes(int64_t h, int64_t w, int levels) {
    return shg::image_dims_ok(h, w) && levels >= 1 && levels <= kMaxLevels ? workspace_bytes(h, w, levels) : 0;
}

extern "C" int shg_wavelet_sharpen_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, int levels, const int32_t* host_gain_q8,
                                       const int32_t* host_threshold_q6, uint16_t* out, int64_t out_pitch, int32_t* planes, void* workspace,
                                       size_t workspace_bytes_given, shg_stream_t stream) {
    const char* fn = "shg_wavelet_sharpen_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(host_gain_q8 && host_threshold_q6 && out && workspace, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(out_pitch >= w, SHG_E_ARG, "%s: output pitch < w", fn);
    SHG_REQUIRE(levels >= 1 && levels <= kMaxLevels, SHG_E_ARG, "%s: %d levels (1 to %d)", fn, levels, kMaxLevels);
    for (int j = 0; j < levels; ++j) {
        SHG_REQUIRE(host_gain_q8[j] >= 0 && host_gain_q8[j] <= kMaxGain, SHG_E_ARG, "%s: gain_q8[%d] = %d outside [0, %d]", fn, j,
                    host_gain_q8[j], kMaxGain);
        SHG_REQUIRE(host_threshold_q6[j] >= 0 && host_threshold_q6[j] <= kMaxThreshold, SHG_E_ARG, "%s: threshold_q6[%d] = %d outside [0, %d]",
                    fn, j, host_threshold_q6[j], kMaxThreshold);
    }
    SHG_REQUIRE(workspace_bytes_given >= workspace_bytes(h, w, levels), SHG_E_ARG, "%s: workspace of %zu bytes, %zu needed", fn,
                workspace_bytes_given, workspace_bytes(h, w, levels));
    const Span img_span = span_of(img, h, w, pitch, sizeof(uint16_t)), out_span = span_of(out, h, w, out_pitch, sizeof(uint16_t));
    SHG_REQUIRE(!overlap(out_span, img_span), SHG_E_ARG, "%s: the output overlaps the image (a stencil cannot run in place)", fn);
    if (planes) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(planes);
        const Span planes_span{lo, lo + (uintptr_t)(levels + 1) * (uintptr_t)h * (uintptr_t)w * sizeof(int32_t)};
        SHG_REQUIRE(!overlap(planes_span, img_span), SHG_E_ARG, "%s: the planes overlap the image", fn);
        SHG_REQUIRE(!overlap(planes_span, out_span), SHG_E_ARG, "%s: the planes overlap the output", fn);
    }
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("wavelet_sharpen", st);
    const size_t px = (size_t)h * (size_t)w;
    long long* acc = reinterpret_cast<long long*>(shg::align_up(workspace, shg::kWorkspaceAlign) + kNoiseBytes);
    int32_t* c_plane[2] = {reinterpret_cast<int32_t*>(acc + px), reinterpret_cast<int32_t*>(acc + px) + px};
    FusedArgs fa{};
    fa.img = img, fa.h = (int)h, fa.w = (int)w, fa.pitch = pitch, fa.levels = levels;
    const int fused = levels < kFusedLevels ? levels : kFusedLevels;
    for (int j = 0; j < fused; ++j) fa.gain[j] = host_gain_q8[j], fa.thr[j] = host_threshold_q6[j];
    fa.out = out, fa.out_pitch = out_pitch, fa.planes = planes;
    fa.c_next = levels > kFusedLevels ? c_plane[0] : nullptr;
    fa.acc = levels > kFusedLevels ? acc : nullptr;
    const dim3 tiles((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kTH - 1) / kTH));
    const char* what = "k_wavelet_fused";
    if (const int e = fused == 1   ? shg::launch(k_wavelet_fused<1>, tiles, dim3(kThreads), 0, st, fa, what)
                      : fused == 2 ? shg::launch(k_wavelet_fused<2>, tiles, dim3(kThreads), 0, st, fa, what)
                                   : shg::launch(k_wavelet_fused<3>, tiles, dim3(kThreads), 0, st, fa, what))
        return e;
    const dim3 rows((unsigned)((w + kTW - 1) / kTW), (unsigned)((h + kRowStep - 1) / kRowStep));
    for (int j = kFusedLevels; j < levels; ++j) {
        const bool last = j == levels - 1;
        LevelArgs la{};
        la.c_in = c_plane[(j - kFusedLevels) % 2], la.c_out = last ? nullptr : c_plane[(j - kFusedLevels + 1) % 2], la.acc = acc;
        la.h = (int)h, la.w = (int)w, la.hole = 1 << j, la.gain = host_gain_q8[j], la.thr = host_threshold_q6[j], la.j = j;
        la.out = out, la.out_pitch = out_pitch, la.planes = planes, la.levels = levels;
        if (const int e = shg::launch(k_wavelet_level, rows, dim3(kThreads), 0, st, la, "k_wavelet_level")) return e;
    }
    return 0;
}

extern "C" int shg_wavelet_noise_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, uint64_t* out2,
                                     void* workspace, size_t workspace_bytes_given, shg_stream_t stream) {
    const char* fn = "shg_wavelet_noise_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(out2 && workspace, SHG_E_ARG, "%s: null pointer", fn);
    NoiseArgs na{};
    if (const int e = shg::parse_disk_mask(fn, circle3, &na.masked, &na.cx, &na.cy, &na.rad2)) return e;
    SHG_REQUIRE(workspace_bytes_given >= workspace_bytes(h, w, 1), SHG_E_ARG, "%s: workspace of %zu bytes, %zu needed", fn,
                workspace_bytes_given, workspace_bytes(h, w, 1));
    uint32_t* tables = reinterpret_cast<uint32_t*>(shg::align_up(workspace, shg::kWorkspaceAlign));
    uint32_t* state = tables + 2 * kBins;
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("wavelet_noise", st);
    if (const int e = shg::zero_async(fn, tables, 2 * kBins * sizeof(uint32_t), st)) return e;
    na.img = img, na.h = (int)h, na.w = (int)w, na.pitch = pitch, na.table = tables, na.state = nullptr;
    const PickArgs pa{tables, state, reinterpret_cast<unsigned long long*>(out2)};
    na.tiles_x = (int)((w + kNW - 1) / kNW);
    na.tiles = na.tiles_x * (int)((h + kNH - 1) / kNH);
    const dim3 tiles((unsigned)(na.tiles < kNoiseBlocks ? na.tiles : kNoiseBlocks));
    if (const int e = shg::launch(k_noise_hist<false>, tiles, dim3(kThreads), 0, st, na, "k_noise_hist (high bits)")) return e;
    if (const int e = shg::launch(k_noise_pick<false>, dim3(1), dim3(kThreads), 0, st, pa, "k_noise_pick (high bits)")) return e;
    na.table = tables + kBins, na.state = state;
    if (const int e = shg::launch(k_noise_hist<true>, tiles, dim3(kThreads), 0, st, na, "k_noise_hist (low bits)")) return e;
    return shg::launch(k_noise_pick<true>, dim3(1), dim3(kThreads), 0, st, pa, "k_noise_pick (low bits)");
}
