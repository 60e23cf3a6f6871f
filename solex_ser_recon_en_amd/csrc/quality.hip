// Sharpness of many small patches of one image in one launch (shg_patch_sharpness_u16): per patch the size of its pixel set, the
// sums of I and I^2 and the sum of the squared five-point Laplacian with an arm of D pixels.  Not a reference stage: the arithmetic
// is the one include/shg_hip.h states, restated in NumPy by tests/quality_ref.py.  The host places the points and turns the sums
// into a quality figure (stack.py); the combine that weights each source by a lattice of such figures is in stack.hip.
//
// One workgroup a point, the layout of align.hip.  The patch with its halo of D pixels sits in LDS (at most 81 x 81 x 2 B, the
// pitch 81: odd, rows fall on different banks); a thread owns the pixels threadIdx.x + 256 k of the patch in row-major order, at
// most 17 of the 65 x 65, reads a pixel and its four arms from the tile and keeps four 64-bit sums.  The wave folds them with
// DPP, the first lane puts the wave's totals into its wave's row of a table in LDS, and four threads add the rows and write the
// point's four words by plain stores.  No global atomic, no memset, and everything accumulated is an integer: no grid shape or
// order can change a bit.  Whether a pixel is in the set is decided before anything is loaded: an empty set writes its row of
// zeros and returns without a read of the image.
#include "image_args.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxB = 32, kMaxD = 8;
constexpr int kMaxSide = 2 * kMaxB + 1;                         // 65
constexpr int kTile = kMaxSide + 2 * kMaxD;                     // 81: the LDS tile's side and its pitch
constexpr int kPerThread = (kMaxSide * kMaxSide + kThreads - 1) / kThreads;      // 17
constexpr int kWords = 4;                                       // the size of the set, the sums of I, I^2 and L^2
constexpr int64_t kMaxPoints = (int64_t)1 << 23;

struct SharpArgs {
    const uint16_t* img;
    int64_t pitch;
    int h, w, B, D, masked;
    double cx, cy, rad2;
    const int* points;
    unsigned long long* out;
};

__global__ __launch_bounds__(kThreads) void k_patch_sharpness(const SharpArgs a) {
    __shared__ uint16_t tile[kTile * kTile];
    __shared__ unsigned long long part[kWaves][kWords];
    const int D = a.D, ps = 2 * a.B + 1, pixels = ps * ps, per = (pixels + kThreads - 1) / kThreads;
    unsigned long long* row = a.out + (int64_t)blockIdx.x * kWords;
    // the patch's first row and column; 64-bit: a centre may lie anywhere
    const int64_t r0 = (int64_t)a.points[2 * blockIdx.x] - a.B, c0 = (int64_t)a.points[2 * blockIdx.x + 1] - a.B;
    uint32_t valid = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = (int)threadIdx.x + k * kThreads;
        if (k < per && i < pixels) {
            const int y = i / ps, x = i - y * ps;
            const int64_t r = r0 + y, c = c0 + x;
            bool ok = c >= D && c < a.w - D && r >= D && r < a.h - D;
            if (ok && a.masked) {
                const double dx = (double)c - a.cx, dy = (double)r - a.cy, d2 = dx * dx + dy * dy;
                ok = !(d2 > a.rad2);
            }
            if (ok) valid |= 1u << k;
        }
    }
    if (!__syncthreads_or(valid != 0)) {                                         // an empty set: a row of zeros
        if (threadIdx.x < kWords) row[threadIdx.x] = 0;
        return;
    }
    const int ts = ps + 2 * D;
    for (int i = threadIdx.x; i < ts * ts; i += kThreads) {
        const int y = i / ts, x = i - y * ts;
        const int64_t gr = r0 - D + y, gc = c0 - D + x;
        // (outside the image: a pixel of the set never reads it)
        tile[y * kTile + x] = gr >= 0 && gr < a.h && gc >= 0 && gc < a.w ? a.img[gr * a.pitch + gc] : (uint16_t)0;
    }
    __syncthreads();
    uint64_t n_valid = 0, sum1 = 0, sum2 = 0, sum_l2 = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (valid >> k & 1u) {
            const int i = (int)threadIdx.x + k * kThreads;
            const int y = i / ps, x = i - y * ps;
            const uint16_t* p = tile + (y + D) * kTile + (x + D);
            const uint32_t v = p[0];
            const int lap = 4 * (int)v - (int)p[-D * kTile] - (int)p[D * kTile] - (int)p[-D] - (int)p[D];        // |lap| < 2^18
            n_valid += 1, sum1 += v, sum2 += (uint64_t)(v * v);                  // v <= 65535: v * v < 2^32
            sum_l2 += (uint64_t)((int64_t)lap * (int64_t)lap);                   // < 2^36
        }
    }
    n_valid = shg::wave_sum(n_valid), sum1 = shg::wave_sum(sum1), sum2 = shg::wave_sum(sum2), sum_l2 = shg::wave_sum(sum_l2);
    if (shg::lane_id() == 0) {
        unsigned long long* mine = part[threadIdx.x / 64];
        mine[0] = n_valid, mine[1] = sum1, mine[2] = sum2, mine[3] = sum_l2;
    }
    __syncthreads();
    if (threadIdx.x < kWords) {
        unsigned long long t = part[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < kWaves; ++wv) t += part[wv][threadIdx.x];
        row[threadIdx.x] = t;
    }
}

}  // namespace

extern "C" int shg_patch_sharpness_u16(const uint16_t* img, int64_t pitch, int64_t h, int64_t w, const int32_t* points, int64_t n, int B,
                                       int D, const double* circle3, uint64_t* out, shg_stream_t stream) {
    const char* fn = "shg_patch_sharpness_u16";
    SHG_REQUIRE(img && points && out, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(shg::image_dims_ok(h, w), SHG_E_UNSUPPORTED, "%s: an image of %lld x %lld (1 to %d either way)", fn, (long long)h,
                (long long)w, shg::kMaxImageDim);
    SHG_REQUIRE(pitch >= w, SHG_E_ARG, "%s: pitch < w", fn);
    SHG_REQUIRE(n >= 1 && n <= kMaxPoints, SHG_E_ARG, "%s: %lld points (1 to %lld)", fn, (long long)n, (long long)kMaxPoints);
    SHG_REQUIRE(B >= 1 && B <= kMaxB, SHG_E_ARG, "%s: a half-size of %d pixels (1 to %d)", fn, B, kMaxB);
    SHG_REQUIRE(D >= 1 && D <= kMaxD, SHG_E_ARG, "%s: an arm of %d pixels (1 to %d)", fn, D, kMaxD);
    SharpArgs a{};
    if (const int e = shg::parse_disk_mask(fn, circle3, &a.masked, &a.cx, &a.cy, &a.rad2)) return e;
    const shg::Span out_span = shg::span_of(out, 1, n * kWords, n * kWords, sizeof(uint64_t));
    SHG_REQUIRE(!shg::overlap(out_span, shg::span_of(img, h, w, pitch, sizeof(uint16_t))) &&
                    !shg::overlap(out_span, shg::span_of(points, 1, 2 * n, 2 * n, sizeof(int32_t))),
                SHG_E_ARG, "%s: the output overlaps an input", fn);
    a.img = img, a.pitch = pitch, a.h = (int)h, a.w = (int)w, a.B = B, a.D = D;
    a.points = points, a.out = reinterpret_cast<unsigned long long*>(out);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("patch_sharpness", st);
    return shg::launch(k_patch_sharpness, dim3((unsigned)n), dim3(kThreads), 0, st, a, "k_patch_sharpness");
}
