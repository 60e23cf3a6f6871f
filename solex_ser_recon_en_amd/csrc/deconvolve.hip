// Deconvolving a disk: Richardson-Lucy iterations of a 16-bit image with a separable point-spread function (shg_rl_deconvolve_u16).
// Not a reference stage: the arithmetic is the one include/shg_hip.h states, all of it float32 with every product and sum rounded on
// its own, restated in NumPy by tests/deconvolve_ref.py.
//
// Two launches an iteration, both of one kernel, k_rl_blur<RP, MODE>: a workgroup of 256 threads owns 64 x 32 pixels and blurs them
// inside LDS.
//   the tile    the source plane with a halo of RP on every side, loaded through the reflection into A (a row of A holds the image row
//               R(ty0 - RP + j, h), so what the row pass makes of it IS t at that reflected row: no symmetry argument is needed);
//   row pass    t for every row of A and the tile's 64 columns into T.  A thread owns a run of 8 outputs along the row: it reads the
//               8 + 2 RP values under them once, as 16-byte LDS reads, and slides the window in registers -- (8 + 2 RP) / 8 LDS
//               values an output, not 2 RP + 1.  Lanes run down the rows; A's pitch is an odd number of 16-byte units, so the 16
//               lanes of a read group fall into 16 different bank quads, and T's pitch (68) does the same for the 16-byte writes;
//   column pass a thread owns 8 outputs down one column (lanes run along the row: consecutive banks), reads 8 + 2 RP values of T
//               and slides the same way;
//   MODE        kForwardImg / kForward: the source is img itself (e_0) / the plane e; the thread divides its pixels of img by
//               max(b, 2^-10) and writes q.  kAdjoint: the source is q and the taps arrive reversed; the thread multiplies its own
//               pixels of e (of img in the first iteration), applies the flush and the clamp and writes e in place -- or, in the
//               last iteration, out and the estimate: no conversion pass and no final pass remain.
// RP is the radius rounded up to one of 2, 6, 10, 16 with the taps padded by zeros, which changes no bit (property (c) of the
// header); the taps travel by value in the kernel's argument.  Every pixel is written once, by one thread, as a fixed expression of
// its inputs: the grid cannot change a bit (property (d)).
#include "image_args.h"

#include <math.h>

#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 64, kTH = 32;                 // the tile
constexpr int kRun = 8;                           // outputs a thread owns along the filter axis
constexpr int kMaxRadius = 16, kMaxIterations = 200;
constexpr float kMinBlur = 0x1p-10f, kFlush = 0x1p-20f, kClamp = 0x1p20f, kMinTap = 0x1p-30f;
constexpr double kSumSlack = 0x1p-10;
constexpr int kColStep = kThreads / kTW;          // a thread owns column threadIdx.x % 64, rows 8 (threadIdx.x / 64) .. + 7
static_assert(kColStep * kRun == kTH, "the column pass covers the tile");

enum { kForwardImg, kForward, kAdjoint };

template <int RP>
struct Tile {
    static constexpr int AW = kTW + 2 * RP, AH = kTH + 2 * RP;
    static constexpr int AP = (AW / 4) % 2 ? AW : AW + 4;          // A's pitch: an odd number of 16-byte units
    static constexpr int TP = kTW + 4;                             // T's: 17 of them
    static constexpr int kWin = kRun + 2 * RP;                     // values under a run
    static_assert(RP % 2 == 0 && AW % 4 == 0 && kWin % 4 == 0, "16-byte reads");
};

template <int RP>
struct RlArgs {
    const uint16_t* img;
    int64_t pitch;
    int h, w;
    float* e;                         // [h][w]
    float* q;                         // [h][w]
    uint16_t* out;                    // the last adjoint launch
    int64_t out_pitch;
    float* estimate;                  // NULL, or [h][w]
    int first, last;                  // the adjoint launch: e is still img; e goes to out and estimate
    float taps[2 * RP + 1];
};

// shg_rl_deconvolve_xy_u16: taps is the row pass's set, taps_y the column pass's.
template <int RP>
struct RlArgsXY : RlArgs<RP> {
    float taps_y[2 * RP + 1];
};

template <int RP>
__device__ __forceinline__ const float (&column_taps(const RlArgs<RP>& a))[2 * RP + 1] { return a.taps; }
template <int RP>
__device__ __forceinline__ const float (&column_taps(const RlArgsXY<RP>& a))[2 * RP + 1] { return a.taps_y; }

// R(i, n) of the header.
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

// the kRun sums under a window, each from 0 in the order of the taps, one rounded multiply and one rounded add a tap
template <int RP>
__device__ __forceinline__ void slide(const float (&win)[kRun + 2 * RP], const float (&taps)[2 * RP + 1], float (&acc)[kRun]) {
#pragma unroll
    for (int o = 0; o < kRun; ++o) {
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t <= 2 * RP; ++t) s = s + taps[t] * win[o + t];
        acc[o] = s;
    }
}

template <int RP, int MODE, class ARGS = RlArgs<RP>>
__global__ __launch_bounds__(kThreads) void k_rl_blur(const ARGS a) {
    using G = Tile<RP>;
    __shared__ __attribute__((aligned(16))) float A[G::AH * G::AP];
    __shared__ __attribute__((aligned(16))) float T[G::AH * G::TP];
    const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
    const float* src = MODE == kAdjoint ? a.q : a.e;
    // (every load of a thread is issued before the first is stored: one round trip to memory a tile, not one a round)
    constexpr int kLoads = (G::AH * G::AW + kThreads - 1) / kThreads;
    float held[kLoads];
#pragma unroll
    for (int n = 0; n < kLoads; ++n) {
        const int i = (int)threadIdx.x + n * kThreads;
        if (i < G::AH * G::AW) {
            const int gr = reflect(ty0 - RP + i / G::AW, a.h), gc = reflect(tx0 - RP + i % G::AW, a.w);
            held[n] = MODE == kForwardImg ? (float)a.img[(int64_t)gr * a.pitch + gc] : src[(int64_t)gr * a.w + gc];
        }
    }
#pragma unroll
    for (int n = 0; n < kLoads; ++n) {
        const int i = (int)threadIdx.x + n * kThreads;
        if (i < G::AH * G::AW) A[i / G::AW * G::AP + i % G::AW] = held[n];
    }
    __syncthreads();
    float win[G::kWin], acc[kRun];
    for (int i = threadIdx.x; i < G::AH * (kTW / kRun); i += kThreads) {
        const int run = i / G::AH, j = i % G::AH;
        const float4* p = reinterpret_cast<const float4*>(A + j * G::AP + kRun * run);
#pragma unroll
        for (int v = 0; v < G::kWin / 4; ++v) {
            const float4 x = p[v];
            win[4 * v] = x.x, win[4 * v + 1] = x.y, win[4 * v + 2] = x.z, win[4 * v + 3] = x.w;
        }
        slide<RP>(win, a.taps, acc);
        float4* t = reinterpret_cast<float4*>(T + j * G::TP + kRun * run);
        t[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        t[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % kTW, ly = (int)threadIdx.x / kTW, c = tx0 + lx;
#pragma unroll
    for (int v = 0; v < G::kWin; ++v) win[v] = T[(kRun * ly + v) * G::TP + lx];
    slide<RP>(win, column_taps<RP>(a), acc);
    if (c >= a.w) return;
#pragma unroll
    for (int o = 0; o < kRun; ++o) {
        const int r = ty0 + kRun * ly + o;
        if (r >= a.h) continue;
        const int64_t at = (int64_t)r * a.w + c;
        if (MODE != kAdjoint) {
            const float d = (float)a.img[(int64_t)r * a.pitch + c];
            a.q[at] = d / fmaxf(acc[o], kMinBlur);
        } else {
            const float before = a.first ? (float)a.img[(int64_t)r * a.pitch + c] : a.e[at];
            const float p = before * acc[o];
            const float e = p < kFlush ? 0.0f : fminf(p, kClamp);
            if (!a.last) {
                a.e[at] = e;
            } else {
                a.out[(int64_t)r * a.out_pitch + c] = (uint16_t)fminf(rintf(e), 65535.0f);          // (e >= 0)
                if (a.estimate) a.estimate[at] = e;
            }
        }
    }
}

// ---- host ----
using shg::overlap;
using shg::Span;
using shg::span_of;

size_t workspace_bytes(int64_t h, int64_t w) { return shg::kWorkspaceAlign + 2 * (size_t)h * (size_t)w * sizeof(float); }

struct Call {
    const uint16_t* img;
    int64_t h, w, pitch;
    const float* taps;                // the row pass's; the column pass's too unless taps_y is given
    int radius, iterations;
    uint16_t* out;
    int64_t out_pitch;
    float* estimate;
    float* planes;                    // e | q
    hipStream_t st;
    const float* taps_y = nullptr;    // shg_rl_deconvolve_xy_u16
    int radius_y = 0;
};

// taps[-radius .. radius] in the middle of dst[-RP .. RP] (the rest stays zero), or reversed about the centre
template <int RP>
void place_taps(float (&dst)[2 * RP + 1], const float* taps, int radius, bool reversed) {
    for (int i = 0; i <= 2 * radius; ++i) dst[reversed ? RP + radius - i : RP - radius + i] = taps[i];
}

template <int RP, class ARGS>
int iterate(const Call& c, ARGS& fwd, ARGS& adj) {
    const dim3 tiles((unsigned)((c.w + kTW - 1) / kTW), (unsigned)((c.h + kTH - 1) / kTH));
    for (int n = 0; n < c.iterations; ++n) {
        adj.first = n == 0, adj.last = n == c.iterations - 1;
        if (const int e = n == 0 ? shg::launch(k_rl_blur<RP, kForwardImg, ARGS>, tiles, dim3(kThreads), 0, c.st, fwd, "k_rl_blur (forward, from the image)")
                                 : shg::launch(k_rl_blur<RP, kForward, ARGS>, tiles, dim3(kThreads), 0, c.st, fwd, "k_rl_blur (forward)"))
            return e;
        if (const int e = shg::launch(k_rl_blur<RP, kAdjoint, ARGS>, tiles, dim3(kThreads), 0, c.st, adj, "k_rl_blur (adjoint)")) return e;
    }
    return 0;
}

template <int RP, class ARGS>
int run(const Call& c) {
    ARGS fwd{}, adj{};
    fwd.img = c.img, fwd.pitch = c.pitch, fwd.h = (int)c.h, fwd.w = (int)c.w;
    fwd.e = c.planes, fwd.q = c.planes + (size_t)c.h * (size_t)c.w;
    fwd.out = c.out, fwd.out_pitch = c.out_pitch, fwd.estimate = c.estimate;
    adj = fwd;
    place_taps<RP>(fwd.taps, c.taps, c.radius, false);
    place_taps<RP>(adj.taps, c.taps, c.radius, true);
    if constexpr (std::is_same<ARGS, RlArgsXY<RP>>::value) {
        place_taps<RP>(fwd.taps_y, c.taps_y, c.radius_y, false);
        place_taps<RP>(adj.taps_y, c.taps_y, c.radius_y, true);
    }
    return iterate<RP>(c, fwd, adj);
}

int check_taps(const char* fn, const char* axis, const float* taps, int radius) {
    SHG_REQUIRE(radius >= 0 && radius <= kMaxRadius, SHG_E_ARG, "%s: a radius of %d%s (0 to %d)", fn, radius, axis, kMaxRadius);
    double sum = 0.0;
    for (int i = 0; i <= 2 * radius; ++i) {
        const float k = taps[i];
        SHG_REQUIRE(isfinite(k) && (k == 0.0f || (k >= kMinTap && k <= 1.0f)), SHG_E_ARG, "%s: tap %d%s = %g is neither 0 nor in [2^-30, 1]", fn,
                    i - radius, axis, (double)k);
        sum += (double)k;
    }
    SHG_REQUIRE(fabs(sum - 1.0) <= kSumSlack, SHG_E_ARG, "%s: the taps%s sum to %.9g, more than 2^-10 off 1", fn, axis, sum);
    return 0;
}

// What the two entry points share: every check but the taps', then the launches.  taps_y NULL: one tap set for both passes.
int deconvolve(const char* fn, const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const float* taps_x, int radius_x,
               const float* taps_y, int radius_y, int iterations, uint16_t* out, int64_t out_pitch, float* estimate, void* workspace,
               size_t workspace_bytes_given, shg_stream_t stream) {
    SHG_REQUIRE(iterations >= 1 && iterations <= kMaxIterations, SHG_E_ARG, "%s: %d iterations (1 to %d)", fn, iterations, kMaxIterations);
    if (const int e = check_taps(fn, taps_y ? " along x" : "", taps_x, radius_x)) return e;
    if (taps_y)
        if (const int e = check_taps(fn, " along y", taps_y, radius_y)) return e;
    const size_t need = workspace_bytes(h, w);
    SHG_REQUIRE(workspace_bytes_given >= need, SHG_E_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes_given, need);
    const Span img_span = span_of(img, h, w, pitch, sizeof(uint16_t)), out_span = span_of(out, h, w, out_pitch, sizeof(uint16_t));
    const uintptr_t ws_lo = reinterpret_cast<uintptr_t>(workspace);
    const Span ws_span{ws_lo, ws_lo + need};
    SHG_REQUIRE(!overlap(out_span, img_span), SHG_E_ARG, "%s: the output overlaps the image (a stencil cannot run in place)", fn);
    SHG_REQUIRE(!overlap(ws_span, img_span), SHG_E_ARG, "%s: the workspace overlaps the image", fn);
    SHG_REQUIRE(!overlap(ws_span, out_span), SHG_E_ARG, "%s: the workspace overlaps the output", fn);
    if (estimate) {
        const Span est_span = span_of(estimate, h, w, w, sizeof(float));
        SHG_REQUIRE(!overlap(est_span, img_span), SHG_E_ARG, "%s: the estimate overlaps the image", fn);
        SHG_REQUIRE(!overlap(est_span, out_span), SHG_E_ARG, "%s: the estimate overlaps the output", fn);
        SHG_REQUIRE(!overlap(est_span, ws_span), SHG_E_ARG, "%s: the estimate overlaps the workspace", fn);
    }
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF(taps_y ? "rl_deconvolve_xy" : "rl_deconvolve", st);
    Call c{img, h, w, pitch, taps_x, radius_x, iterations, out, out_pitch, estimate,
           reinterpret_cast<float*>(shg::align_up(workspace, shg::kWorkspaceAlign)), st};
    if (!taps_y) return radius_x <= 2 ? run<2, RlArgs<2>>(c) : radius_x <= 6 ? run<6, RlArgs<6>>(c) : radius_x <= 10 ? run<10, RlArgs<10>>(c) : run<16, RlArgs<16>>(c);
    c.taps_y = taps_y, c.radius_y = radius_y;
    const int radius = radius_x > radius_y ? radius_x : radius_y;          // RP from the larger; the shorter set is padded with zeros
    return radius <= 2 ? run<2, RlArgsXY<2>>(c) : radius <= 6 ? run<6, RlArgsXY<6>>(c) : radius <= 10 ? run<10, RlArgsXY<10>>(c) : run<16, RlArgsXY<16>>(c);
}

}  // namespace

extern "C" size_t shg_rl_workspace_bytes(int64_t h, int64_t w) { return shg::image_dims_ok(h, w) ? workspace_bytes(h, w) : 0; }

extern "C" int shg_rl_deconvolve_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const float* host_taps, int radius,
                                     int iterations, uint16_t* out, int64_t out_pitch, float* estimate, void* workspace,
                                     size_t workspace_bytes_given, shg_stream_t stream) {
    const char* fn = "shg_rl_deconvolve_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(host_taps && out && workspace, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(out_pitch >= w, SHG_E_ARG, "%s: output pitch < w", fn);
    return deconvolve(fn, img, h, w, pitch, host_taps, radius, nullptr, 0, iterations, out, out_pitch, estimate, workspace, workspace_bytes_given,
                      stream);
}

extern "C" int shg_rl_deconvolve_xy_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const float* host_taps_x, int radius_x,
                                        const float* host_taps_y, int radius_y, int iterations, uint16_t* out, int64_t out_pitch,
                                        float* estimate, void* workspace, size_t workspace_bytes_given, shg_stream_t stream) {
    const char* fn = "shg_rl_deconvolve_xy_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(host_taps_x && host_taps_y && out && workspace, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(out_pitch >= w, SHG_E_ARG, "%s: output pitch < w", fn);
    return deconvolve(fn, img, h, w, pitch, host_taps_x, radius_x, host_taps_y, radius_y, iterations, out, out_pitch, estimate, workspace,
                      workspace_bytes_given, stream);
}
