// Limb protection for the filters that follow a stack (deconvolve, sharpen): the image split into a disk plane and a sky plane that
// have no step at the limb (shg_limb_split_u16), and the filtered planes put back around the untouched band of the limb
// (shg_limb_merge_u16).  Not reference stages: the arithmetic is the one include/shg_hip.h states, restated in NumPy by
// tests/limbguard_ref.py.  Both are streaming kernels with the column ownership of k_ring_flatten (rings.hip): eight columns a
// thread, 16-byte loads and stores where every pitch and pointer allows.
//
// Split: one read of the image, two planes.  A pixel of the inner plane is a copy out to E = rad - margin and a point reflection
// beyond (two bilinear samples on the pixel's ray); the outer plane the mirror image from F = rad + margin inwards.  Every pixel
// outside the band [E, F] is a copy in one plane and a reflection in the other, so with both planes asked for every pixel pays for
// one square root, two divisions and eight gathered samples; a run of eight that copies in every plane asked for (the outer plane
// alone beyond F, the inner one alone inside E) pays for none of them.  The samples of a wave's pixels lie on neighbouring rays:
// the gathers hit the lines their neighbours fetched.
//
// Merge: three reads, one write.  A run of eight that lies in the band is the image, one that lies where the weight is 1 is the
// disk (or sky) plane: neither needs a square root.
//
// Both early-outs decide on d2 against a bound 2^-40 inside the exact one: sqrt is monotone and correctly rounded, so a d2 below
// E^2 (1 - 2^-40) has rho < E however E * E and the square root round, and the full path a run takes otherwise computes the very
// same values: no bit depends on which path a run took.
#include "image_args.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kOct = 8;                           // columns a thread owns
constexpr int kChunk = kThreads * kOct;           // columns a workgroup spans
constexpr int kRows = 2;                          // rows a workgroup handles
constexpr double kSlack = 0x1p-40;                // the early-outs' distance from the exact bounds, relative

template <bool VEC>
__device__ __forceinline__ int column_of(int j) {
    const int base = blockIdx.x * kChunk;
    return VEC ? base + (int)threadIdx.x * kOct + j : base + j * kThreads + (int)threadIdx.x;
}

__device__ __forceinline__ void load8(const uint16_t* row, int c0, uint16_t* v) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + c0);
    v[0] = (uint16_t)q.x, v[1] = (uint16_t)(q.x >> 16), v[2] = (uint16_t)q.y, v[3] = (uint16_t)(q.y >> 16);
    v[4] = (uint16_t)q.z, v[5] = (uint16_t)(q.z >> 16), v[6] = (uint16_t)q.w, v[7] = (uint16_t)(q.w >> 16);
}

__device__ __forceinline__ void store8(uint16_t* row, int c0, const uint16_t* v) {
    uint4 q;
    q.x = (uint32_t)v[0] | (uint32_t)v[1] << 16, q.y = (uint32_t)v[2] | (uint32_t)v[3] << 16;
    q.z = (uint32_t)v[4] | (uint32_t)v[5] << 16, q.w = (uint32_t)v[6] | (uint32_t)v[7] << 16;
    *reinterpret_cast<uint4*>(row + c0) = q;
}

template <bool VEC>
__device__ __forceinline__ void load_run(const uint16_t* row, int w, bool whole, uint16_t* v) {
    if (whole) {
        load8(row, column_of<VEC>(0), v);
    } else {
#pragma unroll
        for (int j = 0; j < kOct; ++j) {
            const int c = column_of<VEC>(j);
            v[j] = c < w ? row[c] : (uint16_t)0;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_run(uint16_t* row, int w, bool whole, const uint16_t* v) {
    if (whole) {
        store8(row, column_of<VEC>(0), v);
    } else {
#pragma unroll
        for (int j = 0; j < kOct; ++j) {
            const int c = column_of<VEC>(j);
            if (c < w) row[c] = v[j];
        }
    }
}

__device__ __forceinline__ uint16_t quantise(double v) { return (uint16_t)fmin(fmax(rint(v), 0.0), 65535.0); }

struct SplitArgs {
    const uint16_t* img;
    uint16_t* inner;                  // may be null
    uint16_t* outer;                  // may be null
    int h, w;
    int64_t pitch, inner_pitch, outer_pitch;
    double cx, cy;
    double e, f;                      // E = rad - margin, F = rad + margin
    double e_floor, f_ceil;           // E - reach, F + reach: where the continuations hold their plateau
    double e_sure2, f_sure2;          // d2 <= e_sure2: rho < E for sure; d2 >= f_sure2: rho > F for sure
};

// bilin(x, y) of the header.  The comparisons are written so that a NaN -- which the entry point's limits rule out -- would clamp
// to 0 and never index.
__device__ __forceinline__ double bilin(const SplitArgs& a, double x, double y) {
    const double xm = (double)(a.w - 1), ym = (double)(a.h - 1);
    x = !(x > 0.0) ? 0.0 : x > xm ? xm : x;
    y = !(y > 0.0) ? 0.0 : y > ym ? ym : y;
    const int x0 = (int)x, y0 = (int)y, x1 = min(x0 + 1, a.w - 1), y1 = min(y0 + 1, a.h - 1);
    const double fx = x - (double)x0, fy = y - (double)y0;
    const uint16_t* r0 = a.img + (int64_t)y0 * a.pitch;
    const uint16_t* r1 = a.img + (int64_t)y1 * a.pitch;
    const double p = (double)r0[x0], q = (double)r0[x1], s = (double)r1[x0], t = (double)r1[x1];
    const double top = p + (q - p) * fx, bot = s + (t - s) * fx;
    return top + (bot - top) * fy;
}

__device__ __forceinline__ double sample(const SplitArgs& a, double ux, double uy, double t) {
    return bilin(a, a.cx + ux * t, a.cy + uy * t);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_limb_split(const SplitArgs a) {
    const int c0 = column_of<VEC>(0);
    if (c0 >= a.w) return;
    double dx[kOct], near2 = INFINITY, far2 = 0.0;
#pragma unroll
    for (int j = 0; j < kOct; ++j) {
        const int c = column_of<VEC>(j);
        dx[j] = (double)c - a.cx;
        const double dx2 = dx[j] * dx[j];
        if (c < a.w) near2 = fmin(near2, dx2), far2 = fmax(far2, dx2);
    }
    const bool whole = VEC && c0 + kOct <= a.w;
    const int r0 = blockIdx.y * kRows, r1 = min(r0 + kRows, a.h);
    for (int r = r0; r < r1; ++r) {
        const double dy = (double)r - a.cy, dy2 = dy * dy;
        uint16_t v[kOct];
        load_run<VEC>(a.img + (int64_t)r * a.pitch, a.w, whole, v);
        // rounding is monotone: every pixel's d2 lies between near2 + dy2 and far2 + dy2 as computed here
        const bool inner_copies = !a.inner || far2 + dy2 <= a.e_sure2, outer_copies = !a.outer || near2 + dy2 >= a.f_sure2;
        uint16_t vi[kOct], vo[kOct];
#pragma unroll
        for (int j = 0; j < kOct; ++j) vi[j] = vo[j] = v[j];
        if (!(inner_copies && outer_copies)) {
#pragma unroll
            for (int j = 0; j < kOct; ++j) {
                if (column_of<VEC>(j) >= a.w) continue;
                const double d2 = dx[j] * dx[j] + dy2, rho = sqrt(d2);
                double ux = 1.0, uy = 0.0;
                if (rho > 0.0) ux = dx[j] / rho, uy = dy / rho;
                if (a.inner && rho > a.e) {
                    const double s = sample(a, ux, uy, a.e), m = sample(a, ux, uy, fmax((a.e + a.e) - rho, a.e_floor));
                    vi[j] = quantise((s + s) - m);
                }
                if (a.outer && rho < a.f) {
                    const double s = sample(a, ux, uy, a.f), m = sample(a, ux, uy, fmin((a.f + a.f) - rho, a.f_ceil));
                    vo[j] = quantise((s + s) - m);
                }
            }
        }
        if (a.inner) store_run<VEC>(a.inner + (int64_t)r * a.inner_pitch, a.w, whole, vi);
        if (a.outer) store_run<VEC>(a.outer + (int64_t)r * a.outer_pitch, a.w, whole, vo);
    }
}

struct MergeArgs {
    const uint16_t* img;
    const uint16_t* disk;
    const uint16_t* sky;              // may be null
    uint16_t* out;
    int h, w;
    int64_t pitch, disk_pitch, sky_pitch, out_pitch;
    double cx, cy;
    double e, f, blend;
    double e_sure2, f_sure2;          // e_sure2 <= d2 <= f_sure2: E < rho < F for sure (the band; e_sure2 > f_sure2 when it is too thin)
    double disk_sure2, sky_sure2;     // d2 <= disk_sure2: wt = 1 on the disk side for sure (-1: nowhere); d2 >= sky_sure2: on the sky side
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_limb_merge(const MergeArgs a) {
    const int c0 = column_of<VEC>(0);
    if (c0 >= a.w) return;
    double dx2[kOct], near2 = INFINITY, far2 = 0.0;
#pragma unroll
    for (int j = 0; j < kOct; ++j) {
        const int c = column_of<VEC>(j);
        const double dx = (double)c - a.cx;
        dx2[j] = dx * dx;
        if (c < a.w) near2 = fmin(near2, dx2[j]), far2 = fmax(far2, dx2[j]);
    }
    const bool whole = VEC && c0 + kOct <= a.w;
    const int r0 = blockIdx.y * kRows, r1 = min(r0 + kRows, a.h);
    for (int r = r0; r < r1; ++r) {
        const double dy = (double)r - a.cy, dy2 = dy * dy, lo2 = near2 + dy2, hi2 = far2 + dy2;
        uint16_t* orow = a.out + (int64_t)r * a.out_pitch;
        uint16_t v[kOct];
        if (hi2 <= a.disk_sure2) {                                   // wt = 1: the disk plane as it is
            load_run<VEC>(a.disk + (int64_t)r * a.disk_pitch, a.w, whole, v);
            store_run<VEC>(orow, a.w, whole, v);
            continue;
        }
        if (a.sky && lo2 >= a.sky_sure2) {                           // wt = 1: the sky plane as it is
            load_run<VEC>(a.sky + (int64_t)r * a.sky_pitch, a.w, whole, v);
            store_run<VEC>(orow, a.w, whole, v);
            continue;
        }
        load_run<VEC>(a.img + (int64_t)r * a.pitch, a.w, whole, v);
        const bool band = lo2 >= a.e_sure2 && (!a.sky || hi2 <= a.f_sure2);      // (without a sky plane everything beyond E is the image)
        if (!band) {
            uint16_t d[kOct], s[kOct];
            load_run<VEC>(a.disk + (int64_t)r * a.disk_pitch, a.w, whole, d);
            if (a.sky) load_run<VEC>(a.sky + (int64_t)r * a.sky_pitch, a.w, whole, s);
#pragma unroll
            for (int j = 0; j < kOct; ++j) {
                const double rho = sqrt(dx2[j] + dy2), o = (double)v[j];
                if (rho < a.e) {
                    const double wt = fmin((a.e - rho) / a.blend, 1.0);
                    v[j] = quantise(o + wt * ((double)d[j] - o));
                } else if (a.sky && rho > a.f) {
                    const double wt = fmin((rho - a.f) / a.blend, 1.0);
                    v[j] = quantise(o + wt * ((double)s[j] - o));
                }
            }
        }
        store_run<VEC>(orow, a.w, whole, v);
    }
}

struct Ring {
    double cx, cy, e, f;
};

// circle3 and margin -> the ring; the limits both calls share
int check_ring(const char* fn, const double* circle3, double margin, Ring* ring) {
    SHG_REQUIRE(circle3, SHG_E_ARG, "%s: null pointer", fn);
    const double cx = circle3[0], cy = circle3[1], rad = circle3[2];
    SHG_REQUIRE(isfinite(cx) && isfinite(cy) && isfinite(rad), SHG_E_ARG, "%s: the circle (%g, %g, %g) is not finite", fn, cx, cy, rad);
    SHG_REQUIRE(rad > 0.0 && rad < (double)shg::kMaxImageDim, SHG_E_ARG, "%s: radius %g outside (0, %d)", fn, rad, shg::kMaxImageDim);
    SHG_REQUIRE(fabs(cx) < 65536.0 && fabs(cy) < 65536.0, SHG_E_ARG, "%s: centre (%g, %g) beyond 65536", fn, cx, cy);
    SHG_REQUIRE(isfinite(margin) && margin >= 0.0, SHG_E_ARG, "%s: a margin of %g (finite and >= 0)", fn, margin);
    SHG_REQUIRE(rad - margin >= 1.0, SHG_E_ARG, "%s: rad - margin = %g is below 1", fn, rad - margin);
    *ring = Ring{cx, cy, rad - margin, rad + margin};
    return 0;
}

dim3 grid_of(int64_t h, int64_t w) { return dim3((unsigned)((w + kChunk - 1) / kChunk), (unsigned)((h + kRows - 1) / kRows)); }

}  // namespace

extern "C" int shg_limb_split_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, double margin,
                                  double reach, uint16_t* inner, int64_t inner_pitch, uint16_t* outer, int64_t outer_pitch,
                                  shg_stream_t stream) {
    using shg::overlap;
    using shg::span_of;
    const char* fn = "shg_limb_split_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(inner || outer, SHG_E_ARG, "%s: null pointer (neither plane is asked for)", fn);
    SHG_REQUIRE(!inner || inner_pitch >= w, SHG_E_ARG, "%s: inner pitch < w", fn);
    SHG_REQUIRE(!outer || outer_pitch >= w, SHG_E_ARG, "%s: outer pitch < w", fn);
    Ring ring;
    if (const int e = check_ring(fn, circle3, margin, &ring)) return e;
    SHG_REQUIRE(isfinite(reach) && reach >= 1.0 && reach <= ring.e, SHG_E_ARG, "%s: a reach of %g (1 to rad - margin = %g)", fn, reach, ring.e);
    const shg::Span img_span = span_of(img, h, w, pitch, sizeof(uint16_t));
    if (inner) SHG_REQUIRE(!overlap(span_of(inner, h, w, inner_pitch, sizeof(uint16_t)), img_span), SHG_E_ARG, "%s: the inner plane overlaps the image", fn);
    if (outer) SHG_REQUIRE(!overlap(span_of(outer, h, w, outer_pitch, sizeof(uint16_t)), img_span), SHG_E_ARG, "%s: the outer plane overlaps the image", fn);
    if (inner && outer)
        SHG_REQUIRE(!overlap(span_of(inner, h, w, inner_pitch, sizeof(uint16_t)), span_of(outer, h, w, outer_pitch, sizeof(uint16_t))), SHG_E_ARG,
                    "%s: the inner plane overlaps the outer plane", fn);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("limb_split", st);
    SplitArgs a{};
    a.img = img, a.inner = inner, a.outer = outer, a.h = (int)h, a.w = (int)w;
    a.pitch = pitch, a.inner_pitch = inner_pitch, a.outer_pitch = outer_pitch;
    a.cx = ring.cx, a.cy = ring.cy, a.e = ring.e, a.f = ring.f, a.e_floor = ring.e - reach, a.f_ceil = ring.f + reach;
    a.e_sure2 = ring.e * ring.e * (1.0 - kSlack), a.f_sure2 = ring.f * ring.f * (1.0 + kSlack);
    const bool vec = shg::rows_aligned(img, pitch, sizeof(uint16_t), 16) && (!inner || shg::rows_aligned(inner, inner_pitch, sizeof(uint16_t), 16)) &&
                     (!outer || shg::rows_aligned(outer, outer_pitch, sizeof(uint16_t), 16));
    return shg::launch(vec ? k_limb_split<true> : k_limb_split<false>, grid_of(h, w), dim3(kThreads), 0, st, a, "k_limb_split");
}

extern "C" int shg_limb_merge_u16(const uint16_t* img, int64_t pitch, const uint16_t* disk, int64_t disk_pitch, const uint16_t* sky,
                                  int64_t sky_pitch, int64_t h, int64_t w, const double* circle3, double margin, double blend, uint16_t* out,
                                  int64_t out_pitch, shg_stream_t stream) {
    using shg::overlap;
    using shg::span_of;
    const char* fn = "shg_limb_merge_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(disk && out, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(disk_pitch >= w && out_pitch >= w && (!sky || sky_pitch >= w), SHG_E_ARG, "%s: a pitch < w", fn);
    Ring ring;
    if (const int e = check_ring(fn, circle3, margin, &ring)) return e;
    SHG_REQUIRE(isfinite(blend) && blend > 0.0, SHG_E_ARG, "%s: a blend of %g (finite and > 0)", fn, blend);
    const shg::Span out_span = span_of(out, h, w, out_pitch, sizeof(uint16_t));
    SHG_REQUIRE(!overlap(out_span, span_of(img, h, w, pitch, sizeof(uint16_t))), SHG_E_ARG, "%s: the output overlaps the image", fn);
    SHG_REQUIRE(!overlap(out_span, span_of(disk, h, w, disk_pitch, sizeof(uint16_t))), SHG_E_ARG, "%s: the output overlaps the disk plane", fn);
    if (sky) SHG_REQUIRE(!overlap(out_span, span_of(sky, h, w, sky_pitch, sizeof(uint16_t))), SHG_E_ARG, "%s: the output overlaps the sky plane", fn);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("limb_merge", st);
    MergeArgs a{};
    a.img = img, a.disk = disk, a.sky = sky, a.out = out, a.h = (int)h, a.w = (int)w;
    a.pitch = pitch, a.disk_pitch = disk_pitch, a.sky_pitch = sky_pitch, a.out_pitch = out_pitch;
    a.cx = ring.cx, a.cy = ring.cy, a.e = ring.e, a.f = ring.f, a.blend = blend;
    a.e_sure2 = ring.e * ring.e * (1.0 + kSlack), a.f_sure2 = ring.f * ring.f * (1.0 - kSlack);
    // (E - rho) / blend >= 1 needs rho <= E - blend; a blend that leaves no such radius has no sure region
    const double full = ring.e - blend * (1.0 + kSlack), far = ring.f + blend * (1.0 + kSlack);
    a.disk_sure2 = full > 0.0 ? full * full * (1.0 - kSlack) : -1.0;
    a.sky_sure2 = far * far * (1.0 + kSlack);
    const bool vec = shg::rows_aligned(img, pitch, sizeof(uint16_t), 16) && shg::rows_aligned(disk, disk_pitch, sizeof(uint16_t), 16) &&
                     (!sky || shg::rows_aligned(sky, sky_pitch, sizeof(uint16_t), 16)) && shg::rows_aligned(out, out_pitch, sizeof(uint16_t), 16);
    return shg::launch(vec ? k_limb_merge<true> : k_limb_merge<false>, grid_of(h, w), dim3(kThreads), 0, st, a, "k_limb_merge");
}
