// The spectral analyser's auto-dispersion loop (reference spectralAnalyserUI.py:271-300): for each scale guess s, the solar
// atlas put on the pixel axis x = (lambda - lambda_a) / s + anchor_x, the run of atlas points with 0 <= x < W (select, :41-48)
// interpolated onto the W pixels as np.interp does, the window around the anchor line set to the row's mean, and the Pearson
// correlation with the log spectrum (np.corrcoef).  One workgroup per guess; the guesses are independent.
//
// The atlas axis is never materialised: NumPy's arange gives a[k] = first + k * d exactly (d = (first + step) - first), so
// x[k] is two roundings of a product / sum and one true float64 division away from the uint8 atlas.  A pixel's bracketing pair
// comes from the closed-form index of its wavelength, corrected by comparing exact x[k] values (a step or two at most).
//
// Bit-exactness: the interpolated values follow np.interp's rules and operation order (-ffp-contract=off, IEEE division), and
// the fill value np.mean(u) is NumPy's pairwise summation (blocks of <= 128 summed by eight strided accumulators, halves split
// at a multiple of 8) then one division, so the rows this writes are NumPy's to the bit.  The correlation's three centred sums
// are plain workgroup reductions: np.corrcoef's own come from a BLAS dot whose order is not NumPy's to define.
#include "shg_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxW = 8192;
constexpr int kBlock = 128;                            // NumPy's PW_BLOCKSIZE
constexpr int kMaxLeaves = kMaxW / (kBlock / 2);       // leaves above the top are longer than 64: at most 128 of them
constexpr int kStack = 16;                             // the split depth is log2(8192 / 64) + 1 = 8

struct AtlasArgs {
    const uint8_t* y;
    int64_t n;                    // atlas points
    double first, d;              // a[k] = first + k * d
    double lambda_a, anchor_x;
    const float* v;               // log spectrum [w], window already filled
    int64_t w;
    int64_t fill_lo, fill_hi;     // [lo, hi) set to the row's mean
    const double* scales;
    int64_t n_guesses;
    double* corr;
    int32_t* run;                 // [n_guesses][2] or NULL
    const int32_t* row_of_guess;  // [n_guesses] or NULL: slot in rows, -1 = none
    int64_t n_rows;
    double* rows;                 // [n_rows][w]
};

__device__ __forceinline__ double atlas_x(const AtlasArgs& a, int64_t k, double s) {
    const double lam = a.first + (double)k * a.d;
    return (lam - a.lambda_a) / s + a.anchor_x;
}

__device__ __forceinline__ int64_t index_estimate(const AtlasArgs& a, double pixel, double s) {
    double e = floor(((pixel - a.anchor_x) * s + a.lambda_a - a.first) / a.d);
    e = fmin(fmax(e, 0.0), (double)(a.n - 1));
    return (int64_t)e;
}

// NumPy's pairwise_sum of a leaf (n <= 128): a plain loop below 8, else eight accumulators over the multiple of 8, the rest after.
__device__ double leaf_sum(const double* a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

__device__ __forceinline__ int left_half(int n) {
    int n2 = n / 2;
    return n2 - n2 % 8;
}

// The leaves of NumPy's pairwise split of [0, n), left to right (one thread).
__device__ int pairwise_leaves(int n, int* start, int* len) {
    int lo_st[kStack], n_st[kStack], sp = 0, count = 0;
    lo_st[0] = 0;
    n_st[0] = n;
    while (sp >= 0) {
        const int lo = lo_st[sp], m = n_st[sp];
        --sp;
        if (m <= kBlock) {
            start[count] = lo;
            len[count] = m;
            ++count;
        } else {
            const int m2 = left_half(m);
            lo_st[++sp] = lo + m2;            // right half, popped second
            n_st[sp] = m - m2;
            lo_st[++sp] = lo;
            n_st[sp] = m2;
        }
    }
    return count;
}

// The leaves' sums combined as the recursion does: left + right at every split (one thread).
__device__ double pairwise_combine(int n, const double* leaf) {
    int n_st[kStack], state[kStack], sp = 0, next = 0;
    double left[kStack], ret = 0.0;
    n_st[0] = n;
    state[0] = 0;
    while (sp >= 0) {
        const int m = n_st[sp];
        if (m <= kBlock) {
            ret = leaf[next++];
            --sp;
        } else if (state[sp] == 0) {
            state[sp] = 1;
            ++sp;
            n_st[sp] = left_half(m);
            state[sp] = 0;
        } else if (state[sp] == 1) {
            state[sp] = 2;
            left[sp] = ret;
            ++sp;
            n_st[sp] = m - left_half(m);
            state[sp] = 0;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}

struct Shared {
    int n_leaves;
    int start[kMaxLeaves], len[kMaxLeaves];
    double leaf[kMaxLeaves];
    double part[3][kThreads / shg::kWave];
    double total;
};

// NumPy's np.add.reduce of u[0, w): every thread gets it.
__device__ double block_pairwise_sum(const double* u, int w, Shared& sh) {
    for (int i = threadIdx.x; i < sh.n_leaves; i += kThreads) sh.leaf[i] = leaf_sum(u + sh.start[i], sh.len[i]);
    __syncthreads();
    if (threadIdx.x == 0) sh.total = pairwise_combine(w, sh.leaf);
    __syncthreads();
    const double r = sh.total;
    __syncthreads();              // (sh.total and sh.leaf are reused by the next call)
    return r;
}

__device__ __forceinline__ double wave_sum_f64(double x) {
    const uint64_t r = shg::wave_fold_u64(__double_as_longlong(x), [](uint64_t a, uint64_t b) {
        return (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
    });
    return __longlong_as_double((long long)r);
}

__global__ __launch_bounds__(kThreads) void k_atlas_correlate(AtlasArgs a) {
    extern __shared__ double u[];                      // [w]
    __shared__ Shared sh;
    const int64_t g = blockIdx.x;
    const int w = (int)a.w;
    const double s = a.scales[g];
    if (threadIdx.x == 0) sh.n_leaves = pairwise_leaves(w, sh.start, sh.len);

    // the run select() keeps: [k0, k1], the first point with x >= 0 and the last with x < w (x rises with k)
    int64_t k0 = index_estimate(a, 0.0, s);
    while (k0 > 0 && atlas_x(a, k0 - 1, s) >= 0.0) --k0;
    while (k0 < a.n && atlas_x(a, k0, s) < 0.0) ++k0;
    int64_t k1 = index_estimate(a, (double)w, s);
    while (k1 + 1 < a.n && atlas_x(a, k1 + 1, s) < (double)w) ++k1;
    while (k1 >= 0 && atlas_x(a, k1, s) >= (double)w) --k1;
    if (threadIdx.x == 0 && a.run) {
        a.run[2 * g] = (int32_t)k0;
        a.run[2 * g + 1] = (int32_t)k1;
    }
    const int slot = a.row_of_guess ? a.row_of_guess[g] : -1;
    double* row = (slot >= 0 && slot < a.n_rows) ? a.rows + (int64_t)slot * w : nullptr;
    if (k0 > k1) {                                     // nothing to interpolate: the reference's min() of an empty array
        if (threadIdx.x == 0) a.corr[g] = __longlong_as_double(0x7ff8000000000000LL);
        if (row)
            for (int p = threadIdx.x; p < w; p += kThreads) row[p] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }

    // np.interp(arange(w), x[k0..k1], y[k0..k1] / 255)
    const double x0 = atlas_x(a, k0, s), x1 = atlas_x(a, k1, s);
    const double f0 = (double)a.y[k0] / 255.0, f1 = (double)a.y[k1] / 255.0;
    for (int p = threadIdx.x; p < w; p += kThreads) {
        const double px = (double)p;
        double r;
        if (px >= x1) {
            r = f1;
        } else if (px < x0) {
            r = f0;
        } else {                                       // x[k0] <= p < x[k1]: j in [k0, k1) with x[j] <= p < x[j + 1]
            int64_t j = index_estimate(a, px, s);
            j = j < k0 ? k0 : (j > k1 - 1 ? k1 - 1 : j);
            double xj = atlas_x(a, j, s);
            while (j > k0 && xj > px) xj = atlas_x(a, --j, s);
            double xn = atlas_x(a, j + 1, s);
            while (j + 1 < k1 && xn <= px) {
                xj = xn;
                xn = atlas_x(a, ++j + 1, s);
            }
            const double fj = (double)a.y[j] / 255.0;
            if (xj == px) {
                r = fj;
            } else {
                const double slope = ((double)a.y[j + 1] / 255.0 - fj) / (xn - xj);
                r = slope * (px - xj) + fj;
            }
        }
        u[p] = r;
    }
    __syncthreads();

    // u[lo:hi] = np.mean(u), the mean taken before the fill
    const double fill = block_pairwise_sum(u, w, sh) / (double)w;
    for (int64_t p = a.fill_lo + threadIdx.x; p < a.fill_hi; p += kThreads) u[p] = fill;
    __syncthreads();
    if (row)
        for (int p = threadIdx.x; p < w; p += kThreads) row[p] = u[p];

    // np.corrcoef(u, v)[0, 1]: centred by the rows' means, c = X X^T * (1 / (w - 1)), c01 / sqrt(c00) / sqrt(c11), clipped
    const double mu = block_pairwise_sum(u, w, sh) / (double)w;
    double sv = 0.0;
    for (int p = threadIdx.x; p < w; p += kThreads) sv += (double)a.v[p];
    const int wave = threadIdx.x / shg::kWave;
    sv = wave_sum_f64(sv);
    if (shg::lane_id() == 0) sh.part[0][wave] = sv;
    __syncthreads();
    const double mv = ((sh.part[0][0] + sh.part[0][1]) + (sh.part[0][2] + sh.part[0][3])) / (double)w;
    __syncthreads();
    double suv = 0.0, suu = 0.0, svv = 0.0;
    for (int p = threadIdx.x; p < w; p += kThreads) {
        const double du = u[p] - mu, dv = (double)a.v[p] - mv;
        suv += du * dv;
        suu += du * du;
        svv += dv * dv;
    }
    suv = wave_sum_f64(suv);
    suu = wave_sum_f64(suu);
    svv = wave_sum_f64(svv);
    if (shg::lane_id() == 0) {
        sh.part[0][wave] = suv;
        sh.part[1][wave] = suu;
        sh.part[2][wave] = svv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[3];
        for (int i = 0; i < 3; ++i) t[i] = (sh.part[i][0] + sh.part[i][1]) + (sh.part[i][2] + sh.part[i][3]);
        const double f = 1.0 / (double)(w - 1);
        const double c = (t[0] * f) / sqrt(t[1] * f) / sqrt(t[2] * f);
        a.corr[g] = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);       // np.clip keeps a NaN
    }
}

}  // namespace

extern "C" int shg_atlas_correlate(const uint8_t* atlas_y, int64_t n_atlas, double first, double step_d, double anchor_wavelength,
                                   double anchor_x, const float* log_spectrum, int64_t w, int64_t fill_lo, int64_t fill_hi,
                                   const double* scales, int64_t n_guesses, double* corr, int32_t* run, const int32_t* row_of_guess,
                                   int64_t n_rows, double* rows, shg_stream_t stream) {
    SHG_REQUIRE(atlas_y && log_spectrum && scales && corr, SHG_E_ARG, "shg_atlas_correlate: null pointer");
    SHG_REQUIRE(n_atlas > 0 && n_atlas <= INT32_MAX, SHG_E_ARG, "shg_atlas_correlate: atlas of %lld points", (long long)n_atlas);
    SHG_REQUIRE(w >= 2 && n_guesses > 0 && n_guesses <= INT32_MAX, SHG_E_ARG, "shg_atlas_correlate: w = %lld, %lld guesses",
                (long long)w, (long long)n_guesses);
    SHG_REQUIRE(w <= kMaxW, SHG_E_UNSUPPORTED, "shg_atlas_correlate: w = %lld above the supported %d pixels", (long long)w, kMaxW);
    SHG_REQUIRE(isfinite(first) && isfinite(step_d) && step_d > 0.0 && isfinite(anchor_wavelength) && isfinite(anchor_x), SHG_E_ARG,
                "shg_atlas_correlate: non-finite or non-positive atlas / anchor parameters");
    SHG_REQUIRE(0 <= fill_lo && fill_lo <= fill_hi && fill_hi <= w, SHG_E_ARG, "shg_atlas_correlate: window [%lld, %lld) outside [0, %lld)",
                (long long)fill_lo, (long long)fill_hi, (long long)w);
    SHG_REQUIRE(n_rows >= 0 && (n_rows == 0 || (row_of_guess && rows)), SHG_E_ARG, "shg_atlas_correlate: %lld rows without their buffers",
                (long long)n_rows);
    const size_t lds = (size_t)w * sizeof(double);
    static const bool lds_ok = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(k_atlas_correlate), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(kMaxW * sizeof(double))) == hipSuccess;
    }();
    SHG_REQUIRE(lds_ok, SHG_E_UNSUPPORTED, "shg_atlas_correlate: %zu bytes of LDS refused", (size_t)(kMaxW * sizeof(double)));
    AtlasArgs a = {atlas_y, n_atlas, first, step_d, anchor_wavelength, anchor_x, log_spectrum, w, fill_lo, fill_hi, scales, n_guesses,
                   corr, run, row_of_guess, n_rows, rows};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("atlas_correlate", st);
    return shg::launch(k_atlas_correlate, dim3((unsigned)n_guesses), dim3(kThreads), lds, st, a, "k_atlas_correlate");
}
