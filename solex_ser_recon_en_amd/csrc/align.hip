// Local alignment points: the exact sums of squared differences of many small patches over a window of integer offsets, in one
// launch (shg_patch_ssd_u16).  Not a reference stage: the arithmetic is the one include/shg_hip.h states, restated in NumPy by
// tests/align_ref.py.  The host places the points and reads the tables (stack.py); the combine that bends each source by the field
// the tables give is in stack.hip.
//
// The frame is patch_args.h's.  The patch of ref sits in registers beside the tile of img: a thread's at most 17 pixels, in arrays
// that only compile-time indices touch.  Per offset a thread sums the squared differences of its pixels (a term is below 2^32, the
// sum 64-bit), the wave folds with DPP, and the first lane puts the wave's total into its wave's row of the table in LDS.  No
// global atomic, no memset, and everything accumulated is an integer: no grid shape or order can change a bit.
#include "patch_args.h"

namespace {

using namespace shg::patch;

constexpr int kMaxS = kMaxMargin;
constexpr int kMaxOffsets = (2 * kMaxS + 1) * (2 * kMaxS + 1);
constexpr int kExtra = 3;                                       // after the sums: the size of the set, the sum of ref, of ref^2

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
    int64_t r0, c0;
    patch_origin(a, &r0, &c0);
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
            if (in_set(a, r, c, S)) {
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
    load_tile(tile, a.img, a.img_pitch, a.h, a.w, r0, c0, ps, S);
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
    fold_partials(part, words, row);
}

}  // namespace

extern "C" int shg_patch_ssd_u16(const uint16_t* ref, int64_t ref_pitch, const uint16_t* img, int64_t img_pitch, int64_t h, int64_t w,
                                 const int32_t* points, int64_t n, int B, int S, const double* circle3, uint64_t* out, shg_stream_t stream) {
    const char* fn = "shg_patch_ssd_u16";
    if (const int e = check_patches(fn, ref && img && points && out, "images", h, w, ref_pitch < img_pitch ? ref_pitch : img_pitch, n, B)) return e;
    SHG_REQUIRE(S >= 0 && S <= kMaxS, SHG_E_ARG, "%s: a search of %d pixels (0 to %d)", fn, S, kMaxS);
    PatchArgs a{};
    if (const int e = shg::parse_disk_mask(fn, circle3, &a.masked, &a.cx, &a.cy, &a.rad2)) return e;
    if (const int e = check_output(fn, out, (int64_t)(2 * S + 1) * (2 * S + 1) + kExtra, points, n, h, w, ref, ref_pitch, img, img_pitch)) return e;
    a.ref = ref, a.img = img, a.ref_pitch = ref_pitch, a.img_pitch = img_pitch, a.h = (int)h, a.w = (int)w, a.B = B, a.S = S;
    a.points = points, a.out = reinterpret_cast<unsigned long long*>(out);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("patch_ssd", st);
    return shg::launch(k_patch_ssd, dim3((unsigned)n), dim3(kThreads), 0, st, a, "k_patch_ssd");
}
