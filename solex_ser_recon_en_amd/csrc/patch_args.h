// What the patch kernels share (align.hip: k_patch_ssd, quality.hip: k_patch_sharpness).  One workgroup a point; the patch with a
// border of M pixels in an LDS tile; a thread owns the pixels threadIdx.x + 256 k of the patch in row-major order; per-wave partial
// sums in LDS are added into the point's output row by plain stores.  A kernel keeps its own argument struct and its own body between
// the tile load and the fold: the helpers are templates over the struct and use its h, w, B, masked, cx, cy, rad2, points and out.
#pragma once

#include "image_args.h"

namespace shg::patch {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxB = 32, kMaxMargin = 8;                       // the patch's half-size; the search of an SSD, the arm of a Laplacian
constexpr int kMaxSide = 2 * kMaxB + 1;                         // 65
constexpr int kTile = kMaxSide + 2 * kMaxMargin;                // 81: the LDS tile's side and its pitch (odd: rows fall on different banks)
constexpr int kPerThread = (kMaxSide * kMaxSide + kThreads - 1) / kThreads;      // 17
constexpr int64_t kMaxPoints = (int64_t)1 << 23;

// An entry point's first checks: check_images, then the number of points and the patch's half-size.
inline int check_patches(const char* fn, bool pointers, const char* images, int64_t h, int64_t w, int64_t pitch, int64_t n, int B) {
    if (const int e = check_images(fn, pointers, images, h, w, pitch)) return e;
    SHG_REQUIRE(n >= 1 && n <= kMaxPoints, SHG_E_ARG, "%s: %lld points (1 to %lld)", fn, (long long)n, (long long)kMaxPoints);
    SHG_REQUIRE(B >= 1 && B <= kMaxB, SHG_E_ARG, "%s: a half-size of %d pixels (1 to %d)", fn, B, kMaxB);
    return 0;
}

// The n rows of `words` words of the output overlap neither the points nor an image (img2: null for one image).
inline int check_output(const char* fn, const uint64_t* out, int64_t words, const int32_t* points, int64_t n, int64_t h, int64_t w,
                        const uint16_t* img, int64_t pitch, const uint16_t* img2 = nullptr, int64_t pitch2 = 0) {
    const Span out_span = span_of(out, 1, n * words, n * words, sizeof(uint64_t));
    SHG_REQUIRE(!overlap(out_span, span_of(img, h, w, pitch, sizeof(uint16_t))) &&
                    !(img2 && overlap(out_span, span_of(img2, h, w, pitch2, sizeof(uint16_t)))) &&
                    !overlap(out_span, span_of(points, 1, 2 * n, 2 * n, sizeof(int32_t))),
                SHG_E_ARG, "%s: the output overlaps an input", fn);
    return 0;
}

// The first row and column of the workgroup's patch; 64-bit: a centre may lie anywhere.
template <class A>
__device__ __forceinline__ void patch_origin(const A& a, int64_t* r0, int64_t* c0) {
    *r0 = (int64_t)a.points[2 * blockIdx.x] - a.B, *c0 = (int64_t)a.points[2 * blockIdx.x + 1] - a.B;
}

// The pixel (r, c) of the image is in the set: at least M from every edge and, with a disk, on it.
template <class A>
__device__ __forceinline__ bool in_set(const A& a, int64_t r, int64_t c, int M) {
    bool ok = c >= M && c < a.w - M && r >= M && r < a.h - M;
    if (ok && a.masked) {
        const double dx = (double)c - a.cx, dy = (double)r - a.cy, d2 = dx * dx + dy * dy;
        ok = !(d2 > a.rad2);
    }
    return ok;
}

// Bit k: the thread's pixel threadIdx.x + 256 k of the patch of side ps is in the set.  (k_patch_ssd walks its pixels itself: it
// loads ref where it finds one in the set, and with that in a callback here its train ran 1.3 % slower.)
template <class A>
__device__ __forceinline__ uint32_t pixels_of_set(const A& a, int64_t r0, int64_t c0, int ps, int M) {
    const int pixels = ps * ps, per = (pixels + kThreads - 1) / kThreads;
    uint32_t valid = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (int)threadIdx.x + k * kThreads;
        if (k < per && i < pixels) {
            const int y = i / ps, x = i - y * ps;
            if (in_set(a, r0 + y, c0 + x, M)) valid |= 1u << k;
        }
    }
    return valid;
}

// The patch with its border of M pixels into the tile, by the whole workgroup; zero outside the image (no pixel of the set reads it).
__device__ __forceinline__ void load_tile(uint16_t* tile, const uint16_t* img, int64_t pitch, int h, int w, int64_t r0, int64_t c0, int ps, int M) {
    const int ts = ps + 2 * M;
    for (int i = threadIdx.x; i < ts * ts; i += kThreads) {
        const int y = i / ts, x = i - y * ts;
        const int64_t gr = r0 - M + y, gc = c0 - M + x;
        tile[y * kTile + x] = gr >= 0 && gr < h && gc >= 0 && gc < w ? img[gr * pitch + gc] : (uint16_t)0;
    }
}

// The waves' partial sums added into the point's output row, by the whole workgroup after a barrier.
template <int W>
__device__ __forceinline__ void fold_partials(const unsigned long long (&part)[kWaves][W], int words, unsigned long long* row) {
    for (int i = threadIdx.x; i < words; i += kThreads) {
        unsigned long long t = part[0][i];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) t += part[wv][i];
        row[i] = t;
    }
}

}  // namespace shg::patch
