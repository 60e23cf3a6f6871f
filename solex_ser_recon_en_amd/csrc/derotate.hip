// Differential rotation taken out of a finished disk (shg_derotate_u16): every on-disk pixel is carried to the sphere, turned back
// about the solar pole by the angle its latitude rotates in the time difference, carried back to the image, sampled there with a Keys
// cubic in integers and rescaled by the limb darkening of the two radii.  Not a reference stage: the arithmetic is the one
// include/shg_hip.h states -- float64, one IEEE operation a step, no trigonometric call on the device --, restated in NumPy by
// tests/derotate_ref.py.  Every pixel is a fixed expression of its inputs: neither the grid nor any early-out can change a bit.
//
// The launch: 256 threads are 32 along 256 columns x 8 rows; a thread owns eight pixels of one row, as k_ring_flatten (rings.hip)
// and k_column_shift (dejitter.hip) own eight columns: neighbours in one 16-byte store where the output's pointer and pitch allow,
// columns 32 apart and single stores otherwise.  The sixteen taps of a pixel lie within the largest displacement of the pixel itself
// (a few pixels in any real series), so a wave's gathers fall into the few row segments its neighbours fetch as well: they go
// through the cache.  The circle, the matrix and the three rates travel by value in the kernel's arguments; the limb-darkening
// table (up to 16384 doubles) is read from device memory, two neighbouring entries a radius.  No LDS, no workspace, no scratch.
#include "image_args.h"

#include <math.h>

namespace {

constexpr int kOct = 8;                           // pixels a thread owns
constexpr int kLanes = 32;                        // threads along the columns
constexpr int kCols = kLanes * kOct;              // columns a workgroup spans
constexpr int kRows = 8;                          // rows a workgroup spans
constexpr int kThreads = kLanes * kRows;
constexpr int kMaxRings = 16384;
constexpr double kMaxRate = 0.5;                  // |k0| + |k1| + |k2|: the polynomials' range
constexpr double kOrthoTol = 1e-12;

// sin a = a P(a2) through a^15 and cos a = Q(a2) through a^16, a2 = a * a: the float64 nearest to +-1 / k!, Horner from the highest
// term down.  For |a| <= 0.5 the first term left out is below 2^-53 of the result.
constexpr double kS3 = -0.16666666666666666, kS5 = 0.008333333333333333, kS7 = -0.0001984126984126984, kS9 = 2.7557319223985893e-06,
                 kS11 = -2.505210838544172e-08, kS13 = 1.6059043836821613e-10, kS15 = -7.647163731819816e-13;
constexpr double kC2 = -0.5, kC4 = 0.041666666666666664, kC6 = -0.001388888888888889, kC8 = 2.48015873015873e-05,
                 kC10 = -2.755731922398589e-07, kC12 = 2.08767569878681e-09, kC14 = -1.1470745597729725e-11, kC16 = 4.779477332387385e-14;

struct DerotateArgs {
    const uint16_t* img;
    uint16_t* out;
    const double* clv;                // device, n_rings doubles, or NULL
    int h, w, n_rings;
    int64_t pitch, out_pitch;
    double cx, cy, rad;
    double m[9];                      // row-major: image (right, up, observer) -> (west, pole, central meridian)
    double k0, k1, k2;
};

template <bool VEC>
__device__ __forceinline__ int column_of(int base, int lx, int j) {
    return VEC ? base + lx * kOct + j : base + j * kLanes + lx;
}

// the four Keys cubic weights (a = -0.5) of the fraction t in Q14, summing to 16384: dejitter.weights' expressions
__device__ __forceinline__ void keys_q14(double t, int64_t* q) {
    const double tt = t * t;
    q[0] = (int64_t)rint((((-0.5 * t + 1.0) * t - 0.5) * t) * 16384.0);
    q[1] = (int64_t)rint(((1.5 * t - 2.5) * tt + 1.0) * 16384.0);
    q[2] = (int64_t)rint((((-1.5 * t + 2.0) * t + 0.5) * t) * 16384.0);
    q[3] = (int64_t)rint(((0.5 * t - 0.5) * tt) * 16384.0);
    q[1] += 16384 - (((q[0] + q[1]) + q[2]) + q[3]);
}

// shg_ring_flatten_u16's rule on the table, at the radius rho
__device__ __forceinline__ double table_at(const double* t, int n, double rho) {
    const double u = rho - 0.5;
    if (u <= 0.0) return t[0];
    if (!(u < (double)(n - 1))) return t[n - 1];
    const int j = (int)u;
    const double f = u - (double)j, g = t[j];
    return g + (t[j + 1] - g) * f;
}

__device__ __forceinline__ uint32_t derotate_pixel(const DerotateArgs& a, int r, int c) {
    const uint32_t same = a.img[(int64_t)r * a.pitch + c];
    const double u = ((double)c - a.cx) / a.rad, v = (a.cy - (double)r) / a.rad;
    const double d2 = u * u + v * v;
    if (!(d2 < 1.0)) return same;                                     // the sky, a prominence (and a NaN from a radius of 0)
    const double z = sqrt(1.0 - d2);
    const double qx = (a.m[0] * u + a.m[1] * v) + a.m[2] * z;
    const double qy = (a.m[3] * u + a.m[4] * v) + a.m[5] * z;
    const double qz = (a.m[6] * u + a.m[7] * v) + a.m[8] * z;
    const double s2 = qy * qy;
    const double ang = (a.k2 * s2 + a.k1) * s2 + a.k0;
    if (ang == 0.0) return same;
    const double a2 = ang * ang;
    const double sa = ang * (((((((kS15 * a2 + kS13) * a2 + kS11) * a2 + kS9) * a2 + kS7) * a2 + kS5) * a2 + kS3) * a2 + 1.0);
    const double ca = (((((((kC16 * a2 + kC14) * a2 + kC12) * a2 + kC10) * a2 + kC8) * a2 + kC6) * a2 + kC4) * a2 + kC2) * a2 + 1.0;
    const double sx = qx * ca - qz * sa, sz = qx * sa + qz * ca, sy = qy;
    const double pu = (a.m[0] * sx + a.m[3] * sy) + a.m[6] * sz;
    const double pv = (a.m[1] * sx + a.m[4] * sy) + a.m[7] * sz;
    const double pz = (a.m[2] * sx + a.m[5] * sy) + a.m[8] * sz;
    if (!(pz > 0.0)) return same;                                     // the source lies behind the limb
    const double x = a.cx + pu * a.rad, y = a.cy - pv * a.rad;
    const double fx = floor(x), fy = floor(y);
    int64_t wx[4], wy[4];
    keys_q14(x - fx, wx);
    keys_q14(y - fy, wy);
    const int x0 = (int)fx, y0 = (int)fy;                             // (|x|, |y| < 65536 + 16384)
    int xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = min(max(x0 + k - 1, 0), a.w - 1);
    int64_t t = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint16_t* row = a.img + (int64_t)min(max(y0 + j - 1, 0), a.h - 1) * a.pitch;
        int64_t hsum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) hsum += wx[k] * (int64_t)row[xs[k]];
        t += wy[j] * hsum;
    }
    const int64_t val = (t + ((int64_t)1 << 27)) >> 28;
    if (a.clv == nullptr) return (uint32_t)(val < 0 ? 0 : val > 65535 ? 65535 : val);
    const double g_out = table_at(a.clv, a.n_rings, sqrt(d2) * a.rad);
    const double g_src = table_at(a.clv, a.n_rings, sqrt(pu * pu + pv * pv) * a.rad);
    return (uint32_t)fmin(fmax(rint((double)val * (g_out / g_src)), 0.0), 65535.0);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_derotate(const DerotateArgs a) {
    const int lx = (int)threadIdx.x % kLanes, r = (int)blockIdx.y * kRows + (int)threadIdx.x / kLanes;
    const int base = (int)blockIdx.x * kCols, c0 = column_of<VEC>(base, lx, 0);
    if (r >= a.h || c0 >= a.w) return;
    uint16_t* orow = a.out + (int64_t)r * a.out_pitch;
    if (VEC && c0 + kOct <= a.w) {
        uint32_t v[kOct];
#pragma unroll
        for (int j = 0; j < kOct; ++j) v[j] = derotate_pixel(a, r, c0 + j);
        uint4 q;
        q.x = v[0] | v[1] << 16, q.y = v[2] | v[3] << 16, q.z = v[4] | v[5] << 16, q.w = v[6] | v[7] << 16;
        *reinterpret_cast<uint4*>(orow + c0) = q;
        return;
    }
#pragma unroll 1
    for (int j = 0; j < kOct; ++j) {
        const int c = column_of<VEC>(base, lx, j);
        if (c < a.w) orow[c] = (uint16_t)derotate_pixel(a, r, c);
    }
}

}  // namespace

extern "C" int shg_derotate_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, const double* matrix9,
                                const double* rate3, const double* clv, int64_t n_rings, uint16_t* out, int64_t out_pitch,
                                shg_stream_t stream) {
    const char* fn = "shg_derotate_u16";
    if (const int e = shg::check_images(fn, img && out && circle3 && matrix9 && rate3, "images", h, w, pitch < out_pitch ? pitch : out_pitch))
        return e;
    const double cx = circle3[0], cy = circle3[1], rad = circle3[2];
    SHG_REQUIRE(isfinite(cx) && isfinite(cy) && isfinite(rad), SHG_E_ARG, "%s: the circle (%g, %g, %g) is not finite", fn, cx, cy, rad);
    SHG_REQUIRE(rad >= 0.0 && rad < (double)kMaxRings, SHG_E_ARG, "%s: radius %g outside [0, %d)", fn, rad, kMaxRings);
    SHG_REQUIRE(fabs(cx) < 65536.0 && fabs(cy) < 65536.0, SHG_E_ARG, "%s: centre (%g, %g) beyond 65536", fn, cx, cy);
    SHG_REQUIRE(n_rings == (int64_t)floor(rad) + 1, SHG_E_ARG, "%s: %lld rings for radius %g (floor(rad) + 1 = %lld)", fn, (long long)n_rings,
                rad, (long long)floor(rad) + 1);
    for (int i = 0; i < 9; ++i) SHG_REQUIRE(isfinite(matrix9[i]), SHG_E_ARG, "%s: the matrix is not finite", fn);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double dot = 0.0;
            for (int k = 0; k < 3; ++k) dot += matrix9[3 * i + k] * matrix9[3 * j + k];
            SHG_REQUIRE(fabs(dot - (i == j ? 1.0 : 0.0)) <= kOrthoTol, SHG_E_ARG, "%s: the matrix is not orthonormal (rows %d and %d)", fn, i, j);
        }
    SHG_REQUIRE(isfinite(rate3[0]) && isfinite(rate3[1]) && isfinite(rate3[2]), SHG_E_ARG, "%s: the rates are not finite", fn);
    SHG_REQUIRE(fabs(rate3[0]) + fabs(rate3[1]) + fabs(rate3[2]) <= kMaxRate, SHG_E_ARG,
                "%s: |k0| + |k1| + |k2| = %g radians is beyond %g", fn, fabs(rate3[0]) + fabs(rate3[1]) + fabs(rate3[2]), kMaxRate);
    SHG_REQUIRE(!shg::overlap(shg::span_of(out, h, w, out_pitch, sizeof(uint16_t)), shg::span_of(img, h, w, pitch, sizeof(uint16_t))), SHG_E_ARG,
                "%s: the output overlaps the image", fn);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("derotate", st);
    DerotateArgs a{};
    a.img = img, a.out = out, a.clv = clv, a.h = (int)h, a.w = (int)w, a.n_rings = (int)n_rings, a.pitch = pitch, a.out_pitch = out_pitch;
    a.cx = cx, a.cy = cy, a.rad = rad;
    for (int i = 0; i < 9; ++i) a.m[i] = matrix9[i];
    a.k0 = rate3[0], a.k1 = rate3[1], a.k2 = rate3[2];
    const bool vec = shg::rows_aligned(out, out_pitch, sizeof(uint16_t), 16);
    const dim3 grid((unsigned)((w + kCols - 1) / kCols), (unsigned)((h + kRows - 1) / kRows));
    return shg::launch(vec ? k_derotate<true> : k_derotate<false>, grid, dim3(kThreads), 0, st, a, "k_derotate");
}
