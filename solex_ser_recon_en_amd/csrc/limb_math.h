// The arithmetic both chains of the limb stage share (limb.hip: one kernel per NumPy / OpenCV / scikit-image call;
// limb_fused.hip: the same through LDS tiles), stated once.  The stage's contract is bit-for-bit equality with SciPy,
// scikit-image 0.18.3 and cv2 (ellipse_to_circle.py:148-291): every function here fixes an order of float64 operations,
// and the two files differ only in where their operands live (planes in memory / tiles in LDS) -- the accessors they pass.
// Plain C++ so that tests/ can compile the same text with the host compiler (tests/c_abi/limb_math_check.cpp); what needs
// device atomics (the union-find) is there under hipcc only.
#pragma once
#include <math.h>
#include <stdint.h>
#include "shg_common.h"

namespace shg {
namespace limb {

constexpr int MAXR = 16;                     // Gaussian radius: int(4 * sigma + 0.5), sigma <= 4
struct GaussW { double w[2 * MAXR + 1]; int radius; };

// ---- the block-mean image in integers ----------------------------------------------------------------------------------
// The 4x4 block mean of uint16 / 65536 is a whole number of 2^-20 below 1, so a k x k window sum of cv2.blur is an integer
// number of these units and the blurred value is that sum times 1/(k*k), with one rounding: ((double)W * kUnit) * (1 / (k*k)).
constexpr double kUnit = 9.5367431640625e-07;        // 2^-20
constexpr double kPerUnit = 1048576.0;               // 2^20

// ---- get_flood_image's accumulators (ellipse_to_circle.py:159-169), unsigned 64-bit words -------------------------------
// Workgroups add their partial results to one of FLOOD_SLOTS slots (workgroup index % FLOOD_SLOTS), the reader folds the slots:
// 128 workgroups on the same three addresses queue up in the memory-side atomic units for most of the kernel's 9 us.
constexpr int FLOOD_SLOTS = 9;
constexpr int ACC_VERY_BRIGHT = 3;                                     // the bits of a double ([0..2]: cleared, unused)
SHG_HD constexpr int acc_sum(int slot) { return 4 + 3 * slot; }        // sum(image) in units of 2^-20
SHG_HD constexpr int acc_min(int slot) { return 5 + 3 * slot; }        // f64_key of min(blurred[blurred < very_bright])
SHG_HD constexpr int acc_max(int slot) { return 6 + 3 * slot; }        // f64_key of its max
constexpr int ACC_ORDER_STATS = 4 + 3 * FLOOD_SLOTS;                   // (limb_fused.hip) four doubles: the order statistics
constexpr int ACC_SMALLEST = ACC_ORDER_STATS + 4;                      // (limb_fused.hip) per slot: ~f64_key of blur k's smallest value
constexpr int ACC_WORDS = ACC_SMALLEST + FLOOD_SLOTS;

struct FloodFold { unsigned long long total, klo, khi; };
SHG_HD FloodFold flood_fold(const unsigned long long* acc) {
    unsigned long long total = 0, klo = ~0ull, khi = 0ull;
    for (int s = 0; s < FLOOD_SLOTS; ++s) {
        total += acc[acc_sum(s)];
        klo = acc[acc_min(s)] < klo ? acc[acc_min(s)] : klo;
        khi = acc[acc_max(s)] > khi ? acc[acc_max(s)] : khi;
    }
    return FloodFold{total, klo, khi};
}

// ---- np.histogram(data, 20) over [mn, mx] (ellipse_to_circle.py:169) -----------------------------------------------------
constexpr int HIST_BINS = 20;
// edge i of the HIST_BINS + 1.  np.histogram: first == last -> (first - 0.5, last + 0.5); bin_edges = np.linspace(first, last, 21)
SHG_HD double hist_edge(double mn, double mx, int i) {
    double first = mn, last = mx;
    if (first == last) { first = first - 0.5; last = last + 0.5; }
    const double step = (last - first) / (double)HIST_BINS;
    return i == HIST_BINS ? last : (double)i * step + first;
}
// largest bin with edge(bin) <= b; the last bin is closed
template <typename Edge>
SHG_HD int hist_bin(Edge edge, double b) {
    int bin = 0;
    for (int j = 1; j < HIST_BINS; ++j) bin = (b >= edge(j)) ? j : bin;
    return bin;
}

// ---- the flood image: img_blurred[< thresh3] = 0; [>= thresh3] = 65000 (ellipse_to_circle.py:226-227) ------------------
SHG_HD bool flood_below(double blurred, double flood_thresh) { return blurred < flood_thresh; }
SHG_HD double flood_value(bool below) { return below ? 0.0 : 65000.0; }

// ---- skimage.feature.canny (scikit-image 0.18.3) up to its masks --------------------------------------------------------
// SciPy's NI_Correlate1D with a symmetric kernel: the centre tap first, then the pairs from the outside in,
//   t = x[0]*w[0]; for j = -R..-1: t += (x[j] + x[-j]) * w[j]
// line(j): the input at offset j from the output pixel (mode 'constant', cval 0: the accessor's to return).  Several lines
// with the same taps go through one loop (canny smooths the image and an all-ones mask): t[i] belongs to the i-th line.
template <typename... Line>
SHG_HD void correlate1d_sym(const GaussW& g, double (&t)[sizeof...(Line)], Line... line) {
    const int R = g.radius;
    int i = 0;
    ((t[i++] = line(0) * g.w[R]), ...);
    for (int j = -R; j < 0; ++j) {
        i = 0;
        ((t[i++] += (line(j) + line(-j)) * g.w[R + j]), ...);
    }
}
template <typename Line>
SHG_HD double correlate1d_sym(const GaussW& g, Line line) {
    double t[1];
    correlate1d_sym(g, t, line);
    return t[0];
}

// smoothed = image / (bleed_over + eps): canny's normalisation by the smoothed all-ones mask (np.finfo(float).eps)
SHG_HD double bleed_over_div(double image, double bleed_over) { return image / (bleed_over + 2.220446049250313e-16); }

SHG_HD int refl(int i, int n) {       // scipy mode 'reflect': d c b a | a b c d | d c b a
    return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
}

// ndi.sobel(axis=0) -> iv and (axis=1) -> jv at (y, x) of the [h][w] image S(yy, xx) reads: derivative [-1,0,1] along the
// axis, then [1,2,1] along the other, each in NI_Correlate1D's order (the products with 0, -1 and 1 included):
//   antisymmetric     : t = x[0]*w[0]; for j = -R..-1: t += (x[j] - x[-j]) * w[j]
template <typename Img>
SHG_HD void sobel_pair(Img S, int y, int x, int h, int w, double& iv, double& jv) {
    const int ym = refl(y - 1, h), yp = refl(y + 1, h), xm = refl(x - 1, w), xp = refl(x + 1, w);
    // correlate1d([-1,0,1]): t = x[0]*0 + (x[-1] - x[+1]) * (-1)
    auto dy = [&](int xx) -> double { double t = S(y, xx) * 0.0; t += (S(ym, xx) - S(yp, xx)) * -1.0; return t; };
    auto dx = [&](int yy) -> double { double t = S(yy, x) * 0.0; t += (S(yy, xm) - S(yy, xp)) * -1.0; return t; };
    // correlate1d([1,2,1]): t = x[0]*2 + (x[-1] + x[+1]) * 1
    iv = dy(x) * 2.0;
    iv += (dy(xm) + dy(xp)) * 1.0;
    jv = dx(y) * 2.0;
    jv += (dx(ym) + dx(yp)) * 1.0;
}

// glibc 2.35 hypot (sysdeps/ieee754/dbl-64/e_hypot.c, the non-FMA kernel), for finite normal-range inputs:
// this is what np.hypot evaluates on the reference's x86-64 hosts.
SHG_HD double hypot_glibc(double x, double y) {
    x = fabs(x);
    y = fabs(y);
    const double ax = x < y ? y : x;
    const double ay = x < y ? x : y;
    if (ax >= ay / 0x1p-54) return ax + ay;
    double h = sqrt(ax * ax + ay * ay);
    double t1, t2;
    if (h <= 2.0 * ay) {
        const double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        const double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}

// 4-sector non-maximum suppression with interpolation, then the two thresholds: bit 0 = in the low mask, bit 1 = in the high mask.
// (y, x) of [h][w]: the pixel; m: its magnitude; grad(is, js): its two Sobel values; M(dy, dx): the magnitude of a neighbour.
template <typename Grad, typename Mag>
SHG_HD unsigned nms_bits(int y, int x, int h, int w, double m, Grad grad, Mag M, double low, double high) {
    bool local = false;
    // eroded all-ones mask (border_value 0) & magnitude > 0
    if (y > 0 && y < h - 1 && x > 0 && x < w - 1 && m > 0.0) {
        double is, js;
        grad(is, js);
        const double ai = fabs(is), aj = fabs(js);
        const bool same = (is >= 0 && js >= 0) || (is <= 0 && js <= 0);
        const bool opp = (is <= 0 && js >= 0) || (is >= 0 && js <= 0);
        auto test = [&](double wgt, double p1, double p2, double m1, double m2) -> bool {
            const bool c_plus = p2 * wgt + p1 * (1 - wgt) <= m;
            const bool c_minus = m2 * wgt + m1 * (1 - wgt) <= m;
            return c_plus && c_minus;
        };
        // later sectors overwrite earlier ones, as the sequential assignments in skimage do
        if (same && ai >= aj) local = test(aj / ai, M(1, 0), M(1, 1), M(-1, 0), M(-1, -1));
        if (same && ai <= aj) local = test(ai / aj, M(0, 1), M(1, 1), M(0, -1), M(-1, -1));
        if (opp && ai <= aj) local = test(ai / aj, M(0, 1), M(-1, 1), M(0, -1), M(1, -1));
        if (opp && ai >= aj) local = test(aj / ai, M(-1, 0), M(-1, 1), M(1, 0), M(1, -1));
    }
    return ((local && m >= low) ? 1u : 0u) | ((local && m >= high) ? 2u : 0u);
}

#if defined(__HIPCC__)
// ---- canny's hysteresis + the labelling of its result (ellipse_to_circle.py:245-252) ------------------------------------
// 8-connected components of the low mask by union-find on the pixel grid (each pixel links to its W, NW, N, NE neighbours;
// roots are the smallest linear index of a component, so sorting roots = scipy.ndimage.label's raster numbering).
// Load: how a parent is read.
struct AgentLoad {
    // agent-scope relaxed loads: parents are rewritten by other workgroups (other XCDs) during the merge,
    // and a CU's L1 / an XCD's L2 is not refreshed by them.  A stale parent would still be a valid older
    // ancestor (parents only ever decrease, and every link is validated by the atomicMin), but fresh reads
    // keep the chains short.
    static __device__ __forceinline__ int at(const int* L, int x) { return __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
struct LdsLoad {                           // labels of one workgroup's tile in LDS
    static __device__ __forceinline__ int at(const int* lab, int x) { return static_cast<const volatile int*>(lab)[x]; }
};

template <typename Load>
__device__ __forceinline__ int uf_find(const int* L, int x) {
    int p = Load::at(L, x);
    while (p != x) { x = p; p = Load::at(L, x); }
    return x;
}

template <typename Load>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
    while (true) {
        a = uf_find<Load>(L, a);
        b = uf_find<Load>(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }      // link the larger root under the smaller
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}
#endif

}  // namespace limb
}  // namespace shg
