// Local alignment points: the exact sums of squared differences of many small patches over a window of integer offsets, in one
// launch (shg_patch_ssd_u16).  Not a reference stage: the arithmetic is the one include/shg_hip.h states, restated in NumPy by
// tests/align_ref.py.  The host places the points and reads the tables (stack.py); the combine that bends each source by the field
// the tables give is in stack.hip.
//
// One workgroup a point.  The patch of img with its border of S pixels sits in LDS (at most 81 x 81 x 2 B), the patch of ref in
// registers: a thread owns the pixels threadIdx.x + 256 k of the patch in row-major order, at most 17 of the 65 x 65, in an array
// that only compile-time indices touch, with a bit mask for "in the set".  Per offset a thread sums the squared differences of its
// pixels (a term is below 2^32, the sum 64-bit), the wave folds with DPP, and the first lane puts the wave's total into its wave's
// row of a table in LDS; at the end the table's four rows are added and every word of the point's output row is written by a plain
// store.  No global atomic, no memset, and everything accumulated is an integer: no grid shape or order can change a bit.
#include "image_args.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxB = 32, kMaxS = 8;
constexpr int kMaxSide = 2 * kMaxB + 1;                         // 65
constexpr int kTile = kMaxSide + 2 * kMaxS;                     // 81: the LDS tile's side and its pitch (odd: rows fall on different banks)
constexpr int kPerThread = (kMaxSide * kMaxSide + kThreads - 1) / kThreads;      // 17
constexpr int kMaxOffsets = (2 * kMaxS + 1) * (2 * kMaxS + 1);
constexpr int kExtra = 3;                                       // after the sums: the size of the set, the sum of ref, of ref^2
constexpr int64_t kMaxPoints = (int64_t)1 << 23;

struct PatchArgs {
    const uint16_t* ref;
    const uint16_t* img;
    int64_t ref_pitch, img_pitch;
    int h, w, B, S, masked;
    double cx, cy, rad2;
    const int* points;
    unsigned long long* out;
};

__global__ __launch_bounds__(kThreads) void k_patch_ssd(const PatchArgs a) {
    __shared__ uint16_t tile[kTile * kTile];
    __shared__ unsigned long long part[kWaves][kMaxOffsets + kExtra];
    const int S = a.S, side = 2 * S + 1, n_off = side * side, words = n_off + kExtra;
    const int ps = 2 * a.B + 1, pixels = ps * ps, per = (pixels + kThreads - 1) / kThreads;
    unsigned long long* row = a.out + (int64_t)blockIdx.x * words;
    // the patch's first row and column; 64-bit: a centre may lie anywhere
    const int64_t r0 = (int64_t)a.points[2 * blockIdx.x] - a.B, c0 = (int64_t)a.points[2 * blockIdx.x + 1] - a.B;
    uint32_t mine[kPerThread];
    int base[kPerThread];
    uint32_t valid = 0;
    uint64_t n_valid = 0, sum1 = 0, sum2 = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        mine[k] = 0, base[k] = 0;
        const int i = (int)threadIdx.x + k * kThreads;
        if (k < per && i < pixels) {
            const int y = i / ps, x = i - y * ps;
            const int64_t r = r0 + y, c = c0 + x;
            bool ok = c >= S && c < a.w - S && r >= S && r < a.h - S;
            if (ok && a.masked) {
                const double dx = (double)c - a.cx, dy = (double)r - a.cy, d2 = dx * dx + dy * dy;
                ok = !(d2 > a.rad2);
            }
            if (ok) {
                const uint32_t v = a.ref[r * a.ref_pitch + c];
                mine[k] = v, valid |= 1u << k, base[k] = y * kTile + x;
                n_valid += 1, sum1 += v, sum2 += (uint64_t)(v * v);              // v <= 65535: v * v < 2^32
            }
        }
    }
    if (!__syncthreads_or(valid != 0)) {                                         // an empty set: a row of zeros
        for (int i = threadIdx.x; i < words; i += kThreads) row[i] = 0;
        return;
    }
    const int ts = ps + 2 * S;
    for (int i = threadIdx.x; i < ts * ts; i += kThreads) {
        const int y = i / ts, x = i - y * ts;
        const int64_t gr = r0 - S + y, gc = c0 - S + x;
        // (outside the image: a pixel of the set never reads it)
        tile[y * kTile + x] = gr >= 0 && gr < a.h && gc >= 0 && gc < a.w ? a.img[gr * a.img_pitch + gc] : (uint16_t)0;
    }
    __syncthreads();
    const bool first_lane = shg::lane_id() == 0;
    unsigned long long* mine_part = part[threadIdx.x / 64];
    for (int v = 0; v < side; ++v) {
        for (int u = 0; u < side; ++u) {
            const int shift = v * kTile + u;
            uint64_t s = 0;
#pragma unroll
            for (int k = 0; k < kPerThread; ++k) {
                if (k < per) {                                                   // (uniform: the patch's size decides)
                    const uint32_t other = tile[base[k] + shift];
                    const uint32_t d = mine[k] > other ? mine[k] - other : other - mine[k];
                    s += valid >> k & 1u ? (uint64_t)(d * d) : 0;                // d <= 65535: d * d < 2^32
                }
            }
            s = shg::wave_sum(s);
            if (first_lane) mine_part[v * side + u] = s;
        }
    }
    n_valid = shg::wave_sum(n_valid), sum1 = shg::wave_sum(sum1), sum2 = shg::wave_sum(sum2);
    if (first_lane) mine_part[n_off] = n_valid, mine_part[n_off + 1] = sum1, mine_part[n_off + 2] = sum2;
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += kThreads) {
        unsigned long long t = part[0][i];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) t += part[wv][i];
        row[i] = t;
    }
}

}  // namespace

extern "C" int shg_patch_ssd_u16(const uint16_t* ref, int64_t ref_pitch, const uint16_t* img, int64_t img_pitch, int64_t h, int64_t w,
                                 const int32_t* points, int64_t n, int B, int S, const double* circle3, uint64_t* out, shg_stream_t stream) {
    const char* fn = "shg_patch_ssd_u16";
    SHG_REQUIRE(ref && img && points && out, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(shg::image_dims_ok(h, w), SHG_E_UNSUPPORTED, "%s: images of %lld x %lld (1 to %d either way)", fn, (long long)h,
                (long long)w, shg::kMaxImageDim);
    SHG_REQUIRE(ref_pitch >= w && img_pitch >= w, SHG_E_ARG, "%s: pitch < w", fn);
    SHG_REQUIRE(n >= 1 && n <= kMaxPoints, SHG_E_ARG, "%s: %lld points (1 to %lld)", fn, (long long)n, (long long)kMaxPoints);
    SHG_REQUIRE(B >= 1 && B <= kMaxB, SHG_E_ARG, "%s: a half-size of %d pixels (1 to %d)", fn, B, kMaxB);
    SHG_REQUIRE(S >= 0 && S <= kMaxS, SHG_E_ARG, "%s: a search of %d pixels (0 to %d)", fn, S, kMaxS);
    PatchArgs a{};
    if (const int e = shg::parse_disk_mask(fn, circle3, &a.masked, &a.cx, &a.cy, &a.rad2)) return e;
    const int64_t words = (int64_t)(2 * S + 1) * (2 * S + 1) + kExtra;
    const shg::Span out_span = shg::span_of(out, 1, n * words, n * words, sizeof(uint64_t));
    SHG_REQUIRE(!shg::overlap(out_span, shg::span_of(ref, h, w, ref_pitch, sizeof(uint16_t))) &&
                    !shg::overlap(out_span, shg::span_of(img, h, w, img_pitch, sizeof(uint16_t))) &&
                    !shg::overlap(out_span, shg::span_of(points, 1, 2 * n, 2 * n, sizeof(int32_t))),
                SHG_E_ARG, "%s: the output overlaps an input", fn);
    a.ref = ref, a.img = img, a.ref_pitch = ref_pitch, a.img_pitch = img_pitch, a.h = (int)h, a.w = (int)w, a.B = B, a.S = S;
    a.points = points, a.out = reinterpret_cast<unsigned long long*>(out);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("patch_ssd", st);
    return shg::launch(k_patch_ssd, dim3((unsigned)n), dim3(kThreads), 0, st, a, "k_patch_ssd");
}
