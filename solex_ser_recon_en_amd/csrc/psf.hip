// Measuring the blur from the limb: the edge-spread tables of the annulus |rho - rad| < reach, one row a sector (shg_limb_profile_u16).
// Not a reference stage: the arithmetic is the one include/shg_hip.h states, all of it float64 with one IEEE operation a step, restated
// in NumPy by tests/psf_ref.py.  The host fits the edge a sector and regresses the widths on the angle (psf.py); the GPU bins and sums.
//
// One launch over the annulus's bounding rows and columns, a workgroup of 256 threads a 32 x 32 tile, four pixels a thread.
//   early-outs   a tile whose farthest pixel lies a pixel inside rad - reach, or whose nearest lies a pixel beyond rad + reach, returns
//                before it touches LDS; a pixel the same way before its square root and its division.  Both compare d2 with squared
//                bounds a whole pixel clear of the annulus, where the roundings (2^-52 relative) cannot matter: whether a pixel counts
//                is decided by the stated v alone, so no bit depends on the path.
//   LDS table    kSlots sectors x kWindow radial bins.  A tile's pixel centres lie within 43.9 pixels of each other, so it touches at
//                most 45 * sub + 1 <= 361 consecutive bins (kWindow = 384, from the tile's lowest bin) and, away from the centre, a
//                few neighbouring sectors.  The sector slot is sector % kSlots with the sector as its tag, claimed by the first pixel
//                that needs it: sectors that follow each other never collide.  An entry is {count << 48 | sum of v^2} (64-bit LDS
//                atomic: a tile holds 1024 pixels, so the sum of squares stays below 2^42 and the count below 2^11) and the sum of v
//                (32-bit: below 2^26).  A pixel whose sector lost its slot or whose bin lies beyond the window -- tiles near the
//                centre of a small disk -- goes straight to the tables: slower, never wrong, never out of bounds.
//   flush        the non-zero entries, with device-scope integer atomics: 32-bit for count, 64-bit for sum and sumsq.
// Everything accumulated is an integer: neither the grid nor the order of the atomics can change a bit.
#include "image_args.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                         // a workgroup's tile is kTile x kTile
constexpr int kPerThread = kTile * kTile / kThreads, kRowStep = kThreads / kTile;
constexpr int kSlots = 4, kWindow = 384, kEntries = kSlots * kWindow;
constexpr int kMaxReach = 64, kMaxSub = 8, kMinSectors = 8, kMaxSectors = 64;
constexpr int kMaxThresholds = kMaxSectors / 8 - 1;
constexpr double kMaxRadius = 16384.0, kMaxCentre = 65536.0;
static_assert(45 * kMaxSub + 1 <= kWindow, "a tile's bins fit the window");
static_assert(kSlots > 0 && kMinSectors % kSlots == 0, "consecutive sectors fall into different slots");

typedef unsigned long long u64;

struct ProfileArgs {
    const uint16_t* img;
    int64_t pitch;
    double cx, cy;
    double inner;                    // rad - reach
    double sub;
    double lo2, hi2;                  // d2 < lo2: at least a pixel inside the annulus; d2 > hi2: at least a pixel beyond it
    int bins, per_octant;             // 2 reach sub; sectors / 8
    int r0, c0, r1, c1;               // the rows and columns walked
    uint32_t* count;
    u64* sum;
    u64* sumsq;
    double threshold[kMaxThresholds];
};

// The sector of a pixel that is not the centre: the fold into the first octant, one division, the thresholds at or below it.
__device__ __forceinline__ int sector_of(const ProfileArgs& a, double dx, double dy) {
    const double ax = fabs(dx), ay = fabs(dy);
    const bool swap = ay > ax;
    const double hi = swap ? ay : ax, lo = swap ? ax : ay;
    const double q = lo / hi;
    int idx = 0;
    for (int k = 0; k < kMaxThresholds; ++k)
        if (k < a.per_octant - 1 && a.threshold[k] <= q) ++idx;
    int octant = swap ? 1 : 0;
    bool rev = swap;
    if (dx < 0.0) octant = 3 - octant, rev = !rev;
    if (dy < 0.0) octant = 7 - octant, rev = !rev;
    return octant * a.per_octant + (rev ? a.per_octant - 1 - idx : idx);
}

__global__ __launch_bounds__(kThreads) void k_limb_profile(const ProfileArgs a) {
    __shared__ u64 cs[kEntries];                  // count << 48 | sum of squares
    __shared__ uint32_t sm[kEntries];             // sum
    __shared__ int tag[kSlots];
    __shared__ int s_base;
    const int tc0 = a.c0 + (int)blockIdx.x * kTile, tr0 = a.r0 + (int)blockIdx.y * kTile;
    {   // the tile as a whole (uniform over the workgroup)
        const double x0 = (double)tc0 - a.cx, x1 = (double)(min(tc0 + kTile, a.c1) - 1) - a.cx;
        const double y0 = (double)tr0 - a.cy, y1 = (double)(min(tr0 + kTile, a.r1) - 1) - a.cy;
        const double nx = x0 > 0.0 ? x0 : x1 < 0.0 ? x1 : 0.0, ny = y0 > 0.0 ? y0 : y1 < 0.0 ? y1 : 0.0;
        const double fx = fmax(fabs(x0), fabs(x1)), fy = fmax(fabs(y0), fabs(y1));
        if (fx * fx + fy * fy < a.lo2 || nx * nx + ny * ny > a.hi2) return;
    }
    for (int i = threadIdx.x; i < kEntries; i += kThreads) cs[i] = 0, sm[i] = 0;
    if (threadIdx.x < kSlots) tag[threadIdx.x] = -1;
    if (threadIdx.x == 0) s_base = INT_MAX;
    __syncthreads();
    const int c = tc0 + (int)threadIdx.x % kTile, r_first = tr0 + (int)threadIdx.x / kTile;
    const double dx = (double)c - a.cx, dx2 = dx * dx;
    int sector[kPerThread], bin[kPerThread];
    uint32_t v[kPerThread];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const int r = r_first + i * kRowStep;
        bin[i] = -1, sector[i] = 0, v[i] = 0;
        if (c >= a.c1 || r >= a.r1) continue;
        const double dy = (double)r - a.cy, d2 = dx2 + dy * dy;
        if (d2 < a.lo2 || d2 > a.hi2) continue;
        const double rho = sqrt(d2), pos = (rho - a.inner) * a.sub;
        if (!(pos >= 0.0 && pos < (double)a.bins)) continue;
        bin[i] = (int)floor(pos);
        sector[i] = sector_of(a, dx, dy);
        v[i] = a.img[(int64_t)r * a.pitch + c];
        atomicMin(&s_base, bin[i]);
        atomicCAS(&tag[sector[i] % kSlots], -1, sector[i]);
    }
    __syncthreads();
    const int base = s_base;
    if (base == INT_MAX) return;                  // no pixel of the tile counts (uniform)
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        if (bin[i] < 0) continue;
        const int slot = sector[i] % kSlots, local = bin[i] - base;
        const u64 sq = (u64)v[i] * (u64)v[i];
        if (local < kWindow && tag[slot] == sector[i]) {
            atomicAdd(&cs[slot * kWindow + local], (u64)1 << 48 | sq);
            atomicAdd(&sm[slot * kWindow + local], v[i]);
        } else {
            const int64_t at = (int64_t)sector[i] * a.bins + bin[i];
            atomicAdd(a.count + at, 1u);
            atomicAdd(a.sum + at, (u64)v[i]);
            atomicAdd(a.sumsq + at, sq);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kEntries; i += kThreads) {
        const u64 word = cs[i];
        if (word == 0) continue;
        const int b = base + i % kWindow;         // (< bins: an entry is non-zero only where a pixel of that bin added to it)
        const int64_t at = (int64_t)tag[i / kWindow] * a.bins + b;
        atomicAdd(a.count + at, (uint32_t)(word >> 48));
        atomicAdd(a.sum + at, (u64)sm[i]);
        atomicAdd(a.sumsq + at, word & (((u64)1 << 48) - 1));
    }
}

using shg::overlap;
using shg::Span;

Span table_span(const void* p, size_t bytes) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + bytes};
}

}  // namespace

extern "C" int shg_limb_profile_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, int reach, int sub,
                                    int sectors, const double* thresholds, uint32_t* count, uint64_t* sum, uint64_t* sumsq,
                                    shg_stream_t stream) {
    const char* fn = "shg_limb_profile_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(circle3 && count && sum && sumsq, SHG_E_ARG, "%s: null pointer", fn);
    const double cx = circle3[0], cy = circle3[1], rad = circle3[2];
    SHG_REQUIRE(isfinite(cx) && isfinite(cy) && isfinite(rad), SHG_E_ARG, "%s: the circle (%g, %g, %g) is not finite", fn, cx, cy, rad);
    SHG_REQUIRE(rad >= 0.0 && rad < kMaxRadius, SHG_E_ARG, "%s: radius %g outside [0, %g)", fn, rad, kMaxRadius);
    SHG_REQUIRE(fabs(cx) < kMaxCentre && fabs(cy) < kMaxCentre, SHG_E_ARG, "%s: centre (%g, %g) beyond %g", fn, cx, cy, kMaxCentre);
    SHG_REQUIRE(reach >= 1 && reach <= kMaxReach && (double)reach <= rad - 1.0, SHG_E_ARG, "%s: a reach of %d (1 to %d, and at most rad - 1 = %g)",
                fn, reach, kMaxReach, rad - 1.0);
    SHG_REQUIRE(sub >= 1 && sub <= kMaxSub, SHG_E_ARG, "%s: %d bins a pixel (1 to %d)", fn, sub, kMaxSub);
    SHG_REQUIRE(sectors >= kMinSectors && sectors <= kMaxSectors && sectors % 8 == 0, SHG_E_ARG, "%s: %d sectors (a multiple of 8 from %d to %d)",
                fn, sectors, kMinSectors, kMaxSectors);
    const int per_octant = sectors / 8;
    SHG_REQUIRE(thresholds || per_octant == 1, SHG_E_ARG, "%s: null pointer", fn);
    for (int k = 0; k < per_octant - 1; ++k) {
        const double t = thresholds[k];
        SHG_REQUIRE(isfinite(t) && t > 0.0 && t < 1.0 && (k == 0 || t > thresholds[k - 1]), SHG_E_ARG,
                    "%s: threshold %d = %g is not finite, not in (0, 1) or not above the one before it", fn, k, t);
    }
    const int bins = 2 * reach * sub;
    const size_t entries = (size_t)sectors * (size_t)bins;
    const Span img_span = shg::span_of(img, h, w, pitch, sizeof(uint16_t)), count_span = table_span(count, entries * sizeof(uint32_t)),
               sum_span = table_span(sum, entries * sizeof(uint64_t)), sumsq_span = table_span(sumsq, entries * sizeof(uint64_t));
    SHG_REQUIRE(!overlap(count_span, img_span) && !overlap(sum_span, img_span) && !overlap(sumsq_span, img_span), SHG_E_ARG,
                "%s: a table overlaps the image", fn);
    SHG_REQUIRE(!overlap(count_span, sum_span) && !overlap(count_span, sumsq_span) && !overlap(sum_span, sumsq_span), SHG_E_ARG,
                "%s: the tables overlap one another", fn);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("limb_profile", st);
    if (const int e = shg::zero_async(fn, count, entries * sizeof(uint32_t), st)) return e;
    if (const int e = shg::zero_async(fn, sum, entries * sizeof(uint64_t), st)) return e;
    if (const int e = shg::zero_async(fn, sumsq, entries * sizeof(uint64_t), st)) return e;
    ProfileArgs a{};
    a.img = img, a.pitch = pitch, a.cx = cx, a.cy = cy;
    a.count = count, a.sum = reinterpret_cast<u64*>(sum), a.sumsq = reinterpret_cast<u64*>(sumsq);
    a.inner = rad - (double)reach, a.sub = (double)sub, a.bins = bins, a.per_octant = per_octant;
    const double clear_in = a.inner - 1.0, clear_out = rad + (double)reach + 1.0;
    a.lo2 = clear_in > 0.0 ? clear_in * clear_in : 0.0, a.hi2 = clear_out * clear_out;
    // the annulus's bounding rows and columns, a pixel to spare either way (|cx|, |cy| < 65536 and clear_out < 16450: exact in int64)
    const int64_t c0 = (int64_t)floor(cx - clear_out), c1 = (int64_t)floor(cx + clear_out) + 2;
    const int64_t r0 = (int64_t)floor(cy - clear_out), r1 = (int64_t)floor(cy + clear_out) + 2;
    a.c0 = (int)(c0 < 0 ? 0 : c0), a.c1 = (int)(c1 > w ? w : c1), a.r0 = (int)(r0 < 0 ? 0 : r0), a.r1 = (int)(r1 > h ? h : r1);
    if (c0 >= w || r0 >= h || a.c0 >= a.c1 || a.r0 >= a.r1) return 0;          // the annulus misses the image: the tables stay zero
    for (int k = 0; k < per_octant - 1; ++k) a.threshold[k] = thresholds[k];
    const dim3 grid((unsigned)((a.c1 - a.c0 + kTile - 1) / kTile), (unsigned)((a.r1 - a.r0 + kTile - 1) / kTile));
    return shg::launch(k_limb_profile, grid, dim3(kThreads), 0, st, a, "k_limb_profile");
}
