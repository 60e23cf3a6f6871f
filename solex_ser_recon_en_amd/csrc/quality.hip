// Sharpness of many small patches of one image in one launch (shg_patch_sharpness_u16): per patch the size of its pixel set, the
// sums of I and I^2 and the sum of the squared five-point Laplacian with an arm of D pixels.  Not a reference stage: the arithmetic
// is the one include/shg_hip.h states, restated in NumPy by tests/quality_ref.py.  The host places the points and turns the sums
// into a quality figure (stack.py); the combine that weights each source by a lattice of such figures is in stack.hip.
//
// The frame is patch_args.h's.  A thread reads each of its at most 17 pixels and its four arms from the tile and keeps four 64-bit
// sums; the wave folds them with DPP and the first lane puts the wave's totals into its wave's row of the table in LDS.  No global
// atomic, no memset, and everything accumulated is an integer: no grid shape or order can change a bit.  Whether a pixel is in the
// set is decided before anything is loaded: an empty set writes its row of zeros and returns without a read of the image.
#include "patch_args.h"

namespace {

using namespace shg::patch;

constexpr int kMaxD = kMaxMargin;
constexpr int kWords = 4;                                       // the size of the set, the sums of I, I^2 and L^2

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
    const int D = a.D, ps = 2 * a.B + 1;
    unsigned long long* row = a.out + (int64_t)blockIdx.x * kWords;
    int64_t r0, c0;
    patch_origin(a, &r0, &c0);
    const uint32_t valid = pixels_of_set(a, r0, c0, ps, D);
    if (!__syncthreads_or(valid != 0)) {                                         // an empty set: a row of zeros
        if (threadIdx.x < kWords) row[threadIdx.x] = 0;
        return;
    }
    load_tile(tile, a.img, a.pitch, a.h, a.w, r0, c0, ps, D);
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
    fold_partials(part, kWords, row);
}

}  // namespace

extern "C" int shg_patch_sharpness_u16(const uint16_t* img, int64_t pitch, int64_t h, int64_t w, const int32_t* points, int64_t n, int B,
                                       int D, const double* circle3, uint64_t* out, shg_stream_t stream) {
    const char* fn = "shg_patch_sharpness_u16";
    if (const int e = check_patches(fn, img && points && out, "an image", h, w, pitch, n, B)) return e;
    SHG_REQUIRE(D >= 1 && D <= kMaxD, SHG_E_ARG, "%s: an arm of %d pixels (1 to %d)", fn, D, kMaxD);
    SharpArgs a{};
    if (const int e = shg::parse_disk_mask(fn, circle3, &a.masked, &a.cx, &a.cy, &a.rad2)) return e;
    if (const int e = check_output(fn, out, kWords, points, n, h, w, img, pitch)) return e;
    a.img = img, a.pitch = pitch, a.h = (int)h, a.w = (int)w, a.B = B, a.D = D;
    a.points = points, a.out = reinterpret_cast<unsigned long long*>(out);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("patch_sharpness", st);
    return shg::launch(k_patch_sharpness, dim3((unsigned)n), dim3(kThreads), 0, st, a, "k_patch_sharpness");
}
