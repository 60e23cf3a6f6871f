// Stacking a series of scans: the resample-and-combine of N registered disks (shg_stack_combine_u16) and the exact sum of squared
// differences over a window of integer offsets (shg_shift_ssd_u16).  Not reference stages: the arithmetic is the one
// include/shg_hip.h states, restated in NumPy by tests/stack_ref.py.  The host finds the transforms (stack.py); the GPU resamples,
// combines and sums.
//
// Combine: one launch, the resampled planes never leave the registers.  A thread owns eight adjacent output columns of one row and
// works through them one after the other: the four 2-byte gathers a source costs a pixel then fall, for the thread's own columns
// and for those of the lanes beside it, into the same cache lines (s is within a few per cent of 1), and the eight results leave
// in one 16-byte store (the counts in one 8-byte store) where pointer and pitch allow, element by element otherwise.  The source
// count and the per-source records are wave-uniform: they are read from the kernel's arguments (32 records of 56 bytes), where
// they are used (see combine_octet on why not once a thread).  The samples of a pixel sit in a private array that is only ever
// indexed by compile-time constants -- the kernel is a template on a capacity of 4 / 8 / 16 / 32 sources and on the mode, every
// loop over the array is unrolled, a bit mask says which samples are present or kept -- so the array lives in registers: no
// scratch.  The median pads the absent samples with +inf, runs a fixed bitonic network of compare-exchanges whose indices are
// template arguments and picks its two ranks by masking the samples' bits.
//
// Combine with a displacement field a source (shg_stack_combine_field_u16): the same code, a template on whether there are
// fields, under a kernel of its own that takes them as a second argument.  The lattice is one for all sources: the thread finds
// its row's cell and weight once, its column's cell once a column (the remainder walks along with the column: step >= 8 = a
// thread's columns, so it wraps once at most), and a source with a field costs four 16-byte node loads and two bilinear
// interpolations before its sample; a null field costs a scalar test.  Without fields none of this is compiled:
// k_stack_combine<CAP, MODE> is the kernel it was.
//
// Combine with a weight lattice a source as well (shg_stack_combine_weighted_u16): the same code again, a second template switch
// beside the first, under a third kernel that takes the lattices as a third argument.  A source's weight is interpolated between
// the four nodes of the pixel's cell (8-byte loads: the nodes are cache-resident) before its sample, and a weight that is not > 0
// skips the sample; the CAP weights sit in a second private array beside the samples, indexed by compile-time constants only, so
// they too live in registers (past 256 the compiler takes accumulation registers: still no scratch).  The clipping passes do not
// see the weights; the last step is a weighted in-order mean of the kept samples.  Without the switch none of this is compiled.
// On the host the three entry points are one function, combine(): one set of checks, one ladder over capacity and mode.
//
// SSD: a workgroup walks 64 x 16 tiles; it holds the tile of img with a border of S pixels in LDS and its own four pixels of ref
// in registers, and for each of the (2 S + 1)^2 offsets sums the squared differences of its pixels (a term is below 2^32, the sum
// 64-bit), folds the wave with DPP and adds the wave's total to a table in LDS; at its end it adds the table's non-zero entries
// to the output with 64-bit integer atomics.  Everything accumulated is an integer: neither the grid nor the order of the atomics
// can change a bit.  A tile without a pixel of the set is skipped before its border is loaded.
#include "image_args.h"

#include <math.h>
#include <utility>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSources = 32;

// ---- combine ----
constexpr int kOct = 8;                           // columns a thread owns
constexpr int kLanesX = 32;                       // threads along a row: a workgroup spans 256 columns ...
constexpr int kRows = kThreads / kLanesX;         // ... of 8 rows

struct SourceRec {
    const uint16_t* p;
    int h, w;
    int64_t pitch;
    double s, tx, ty, gain;
};

struct CombineArgs {
    uint16_t* out;
    uint8_t* count;
    int oh, ow;
    int64_t out_pitch, count_pitch;
    int n, iterations;
    double kappa;
    int vec_out, vec_count;           // rows of the output / of the counts start on 16 / 8 bytes
    SourceRec src[kMaxSources];
};
static_assert(sizeof(CombineArgs) <= 4096, "kernel arguments");

// A displacement field a source on one lattice: nodes at (j step, i step), (dx, dy) a node, null for none.  A kernel argument of
// its own: the compiler reads a by-value struct from the argument segment only while it counts fewer than 300 accesses to it --
// beyond that it copies the struct to scratch first -- and the records' 32 x 8 are most of that.
struct FieldArgs {
    const double* field[kMaxSources];
    int gh, gw, step;
};
static_assert(sizeof(CombineArgs) + sizeof(FieldArgs) <= 4096, "kernel arguments");
// One weight a node a source on the same lattice, null for 1 everywhere: a third kernel argument, for the same reason.
struct WeightArgs {
    const double* weight[kMaxSources];
};
static_assert(sizeof(CombineArgs) + sizeof(FieldArgs) + sizeof(WeightArgs) <= 4096, "kernel arguments");
constexpr int kMinStep = 8, kMaxStep = 128;
static_assert(kMinStep >= 8, "a thread's eight columns cross one lattice line at most");

// A pixel's place on the lattice: the element offsets of its cell's four nodes and its two weights.
struct Cell {
    int n00, n01, n10, n11;
    double fx, fy;
};

// The displacement of field `f` at the cell: per component top = a + (b - a) fx, bot = c + (d - c) fx, top + (bot - top) fy.
__device__ __forceinline__ void displacement(const double* f, const Cell& cell, double* dx, double* dy) {
    const double2 a = *reinterpret_cast<const double2*>(f + cell.n00), b = *reinterpret_cast<const double2*>(f + cell.n01);
    const double2 c = *reinterpret_cast<const double2*>(f + cell.n10), d = *reinterpret_cast<const double2*>(f + cell.n11);
    const double top_x = a.x + (b.x - a.x) * cell.fx, bot_x = c.x + (d.x - c.x) * cell.fx;
    const double top_y = a.y + (b.y - a.y) * cell.fx, bot_y = c.y + (d.y - c.y) * cell.fx;
    *dx = top_x + (bot_x - top_x) * cell.fy;
    *dy = top_y + (bot_y - top_y) * cell.fy;
}

// The weight of lattice `w` at the cell (whose offsets count the fields' two doubles a node): top = a + (b - a) fx,
// bot = c + (d - c) fx, top + (bot - top) fy.
__device__ __forceinline__ double node_weight(const double* w, const Cell& cell) {
    const double a = w[cell.n00 >> 1], b = w[cell.n01 >> 1], c = w[cell.n10 >> 1], d = w[cell.n11 >> 1];
    const double top = a + (b - a) * cell.fx, bot = c + (d - c) * cell.fx;
    return top + (bot - top) * cell.fy;
}

// The sample of source `s` at the output pixel (rd, cd): false when it is absent (also when rd or cd is not a number: the
// comparison is the negated one).
__device__ __forceinline__ bool sample(const SourceRec& s, double cd, double rd, double* v) {
    const double sx = s.tx + s.s * cd, sy = s.ty + s.s * rd;
    if (!(sx >= 0.0 && sx <= (double)(s.w - 1) && sy >= 0.0 && sy <= (double)(s.h - 1))) return false;
    const int x0 = (int)sx, y0 = (int)sy;                            // (0 <= sx <= w - 1 < 16384)
    const int x1 = min(x0 + 1, s.w - 1), y1 = min(y0 + 1, s.h - 1);
    const double fx = sx - (double)x0, fy = sy - (double)y0;
    const uint16_t* row0 = s.p + (int64_t)y0 * s.pitch;
    const uint16_t* row1 = s.p + (int64_t)y1 * s.pitch;
    const double a = (double)row0[x0], b = (double)row0[x1], c = (double)row1[x0], d = (double)row1[x1];
    const double top = a + (b - a) * fx, bot = c + (d - c) * fx;
    const double val = top + (bot - top) * fy;
    *v = val * s.gain;
    return true;
}

// The sum, in index order, of the samples whose bit is set.  (The samples are >= +0: starting from 0.0 changes no bit.)
template <int CAP>
__device__ __forceinline__ double sum_of(const double (&v)[CAP], uint32_t mask) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (mask >> j & 1u) s = s + v[j];
    return s;
}

// A fixed bitonic network over the CAP samples, ascending: every index is a template argument, so that the array is split into
// registers before any loop would have to be unrolled.
template <int CAP, int K, int J, int I>
__device__ __forceinline__ void compare_exchange(double (&v)[CAP]) {
    constexpr int L = I ^ J;
    if constexpr (L > I) {
        const double lo = fmin(v[I], v[L]), hi = fmax(v[I], v[L]);
        constexpr bool up = (I & K) == 0;
        v[I] = up ? lo : hi;
        v[L] = up ? hi : lo;
    }
}
template <int CAP, int K, int J, int... I>
__device__ __forceinline__ void network_stage(double (&v)[CAP], std::integer_sequence<int, I...>) {
    (compare_exchange<CAP, K, J, I>(v), ...);
}
template <int CAP, int K, int J>
__device__ __forceinline__ void network_merge(double (&v)[CAP]) {
    network_stage<CAP, K, J>(v, std::make_integer_sequence<int, CAP>{});
    if constexpr (J > 1) network_merge<CAP, K, J / 2>(v);
}
template <int CAP, int K = 2>
__device__ __forceinline__ void sort_network(double (&v)[CAP]) {
    network_merge<CAP, K, K / 2>(v);
    if constexpr (K < CAP) sort_network<CAP, K * 2>(v);
}

// The sample of rank `rank`: the bits of every sample under a mask that is all ones for that rank only (a chain of selects on the
// values is turned back into a run-time index by the compiler, and the array with it into memory).
template <int CAP>
__device__ __forceinline__ double pick(const double (&v)[CAP], int rank) {
    unsigned long long bits = 0;
#pragma unroll
    for (int j = 0; j < CAP; ++j) bits |= (unsigned long long)__double_as_longlong(v[j]) & (j == rank ? ~0ull : 0ull);
    return __longlong_as_double((long long)bits);
}

// One output pixel -> its 16-bit value and its count.  FIELD: `f` holds the fields and `cell` is the pixel's; else neither is read.
// WEIGHT (with FIELD only: the cell is the lattice's): `w` holds the weight lattices.
template <int CAP, int MODE, bool FIELD, bool WEIGHT>
__device__ __forceinline__ void combine_pixel(const CombineArgs& a, const FieldArgs* f, const WeightArgs* w, int r, int c, int zero,
                                              const Cell& cell, uint32_t* value, uint32_t* count) {
    static_assert(!WEIGHT || (FIELD && MODE != SHG_STACK_MEDIAN), "weights come on the fields' lattice, and not to a median");
    double v[CAP];
    double wt[WEIGHT ? CAP : 1];
    uint32_t present = 0;
    const double cd = (double)c, rd = (double)r;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        v[j] = INFINITY;
        if constexpr (WEIGHT) wt[j] = 0.0;
        if (j < a.n) {
            double t, cj = cd, rj = rd;
            bool wanted = true;
            if constexpr (WEIGHT) {
                double wj = 1.0;
                if (const double* nodes = w->weight[j + zero]) wj = node_weight(nodes, cell);
                wanted = wj > 0.0;                                   // (false for a weight that is not a number)
                if (wanted) wt[j] = wj;
            }
            if constexpr (FIELD) {
                if (const double* nodes = f->field[j + zero]) {
                    double dx, dy;
                    displacement(nodes, cell, &dx, &dy);
                    cj = cd + dx, rj = rd + dy;
                }
            }
            if (wanted && sample(a.src[j + zero], cj, rj, &t)) v[j] = t, present |= 1u << j;
        }
        // four sources' gathers in flight at a time: without the fence the scheduler hoists the loads of all CAP sources and
        // the registers of their addresses and records with them
        if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
    const int n = __popc(present);
    *value = 0, *count = 0;
    if (n == 0) return;
    double m;
    uint32_t kept = present;
    if (MODE == SHG_STACK_MEDIAN) {
        sort_network<CAP>(v);
        m = (pick<CAP>(v, (n - 1) / 2) + pick<CAP>(v, n / 2)) / 2.0;
    } else {
        if (MODE == SHG_STACK_SIGMA && n >= 3) {
            for (int pass = 0; pass < a.iterations; ++pass) {
                const double size = (double)__popc(kept), mean = sum_of<CAP>(v, kept) / size;
                double q = 0.0;
#pragma unroll
                for (int j = 0; j < CAP; ++j)
                    if (kept >> j & 1u) {
                        const double d = v[j] - mean;
                        q = q + d * d;
                    }
                const double lim = a.kappa * sqrt(q / size);
                uint32_t next = 0;
#pragma unroll
                for (int j = 0; j < CAP; ++j)
                    if ((kept >> j & 1u) && fabs(v[j] - mean) <= lim) next |= 1u << j;
                if (next == 0 || next == kept) break;
                kept = next;
                if (__popc(kept) < 3) break;
            }
        }
        if constexpr (WEIGHT) {
            double num = 0.0, den = 0.0;
#pragma unroll
            for (int j = 0; j < CAP; ++j)
                if (kept >> j & 1u) {
                    const double t = wt[j] * v[j];
                    num = num + t, den = den + wt[j];
                }
            m = num / den;
        } else {
            m = sum_of<CAP>(v, kept) / (double)__popc(kept);
        }
    }
    *value = (uint32_t)fmin(fmax(rint(m), 0.0), 65535.0);
    *count = (uint32_t)__popc(kept);
}

// A thread's eight columns.
template <int CAP, int MODE, bool FIELD, bool WEIGHT = false>
__device__ __forceinline__ void combine_octet(const CombineArgs& a, const FieldArgs* f, const WeightArgs* w = nullptr) {
    const int c0 = (blockIdx.x * kLanesX + (int)threadIdx.x % kLanesX) * kOct, r = blockIdx.y * kRows + (int)threadIdx.x / kLanesX;
    if (r >= a.oh || c0 >= a.ow) return;
    const int nc = min(kOct, a.ow - c0);
    uint64_t lo = 0, hi = 0, counts = 0;          // columns 0 .. 3, columns 4 .. 7, a byte a column
    Cell cell{};
    int row0 = 0, row1 = 0, i = 0, rem = 0;       // the row's two lattice rows (element offsets), the column's cell and remainder
    double step_d = 0.0;
    if constexpr (FIELD) {
        const int j = r / f->step, j1 = min(j + 1, f->gh - 1);
        step_d = (double)f->step;
        cell.fy = (double)(r - j * f->step) / step_d;
        row0 = j * f->gw * 2, row1 = j1 * f->gw * 2;
        i = c0 / f->step, rem = c0 - i * f->step;
    }
#pragma unroll 1
    for (int j = 0; j < nc; ++j) {
        // A zero the compiler cannot see through, new for every column, in the index of the source records: they are then read
        // from the kernel's arguments where they are used.  Hoisted out of this loop as invariants, the 14 words of each of up
        // to 32 records outnumber the scalar registers and spill.
        int zero = 0;
        asm volatile("" : "+s"(zero));
        uint32_t value, count;
        if constexpr (FIELD) {
            const int i1 = min(i + 1, f->gw - 1);
            cell.n00 = row0 + 2 * i, cell.n01 = row0 + 2 * i1, cell.n10 = row1 + 2 * i, cell.n11 = row1 + 2 * i1;
            cell.fx = (double)rem / step_d;
            if (++rem == f->step) rem = 0, ++i;
        }
        combine_pixel<CAP, MODE, FIELD, WEIGHT>(a, f, w, r, c0 + j, zero, cell, &value, &count);
        if (j < 4) lo |= (uint64_t)value << (16 * j);
        else hi |= (uint64_t)value << (16 * (j - 4));
        counts |= (uint64_t)count << (8 * j);
    }
    uint16_t* orow = a.out + (int64_t)r * a.out_pitch + c0;
    if (nc == kOct && a.vec_out) {
        uint4 q;
        q.x = (uint32_t)lo, q.y = (uint32_t)(lo >> 32), q.z = (uint32_t)hi, q.w = (uint32_t)(hi >> 32);
        *reinterpret_cast<uint4*>(orow) = q;
    } else {
        for (int j = 0; j < nc; ++j) orow[j] = (uint16_t)((j < 4 ? lo >> (16 * j) : hi >> (16 * (j - 4))) & 0xFFFFu);
    }
    if (a.count) {
        uint8_t* crow = a.count + (int64_t)r * a.count_pitch + c0;
        if (nc == kOct && a.vec_count) {
            uint2 q;
            q.x = (uint32_t)counts, q.y = (uint32_t)(counts >> 32);
            *reinterpret_cast<uint2*>(crow) = q;
        } else {
            for (int j = 0; j < nc; ++j) crow[j] = (uint8_t)(counts >> (8 * j) & 0xFFu);
        }
    }
}

template <int CAP, int MODE>
__global__ __launch_bounds__(kThreads) void k_stack_combine(const CombineArgs a) {
    combine_octet<CAP, MODE, false>(a, nullptr);
}

template <int CAP, int MODE>
__global__ __launch_bounds__(kThreads) void k_stack_combine_field(const CombineArgs a, const FieldArgs f) {
    combine_octet<CAP, MODE, true>(a, &f);
}

template <int CAP, int MODE>
__global__ __launch_bounds__(kThreads) void k_stack_combine_weighted(const CombineArgs a, const FieldArgs f, const WeightArgs w) {
    combine_octet<CAP, MODE, true, true>(a, &f, &w);
}

// The one ladder over mode and capacity behind the three entry points.  f: the fields, null for the plain combine; w: the weight
// lattices (with f), null for none -- and never with the median: that combination is not instantiated.
template <int CAP, int MODE>
int launch_kernel(dim3 grid, hipStream_t st, const CombineArgs& a, const FieldArgs* f, const WeightArgs* w) {
    if (!f) return shg::launch(k_stack_combine<CAP, MODE>, grid, dim3(kThreads), 0, st, a, "k_stack_combine");
    if (!w) {
        hipLaunchKernelGGL((k_stack_combine_field<CAP, MODE>), grid, dim3(kThreads), 0, st, a, *f);
        return shg::check_launch("k_stack_combine_field");
    }
    if constexpr (MODE != SHG_STACK_MEDIAN) {
        hipLaunchKernelGGL((k_stack_combine_weighted<CAP, MODE>), grid, dim3(kThreads), 0, st, a, *f, *w);
        return shg::check_launch("k_stack_combine_weighted");
    }
    return SHG_E_ARG;                                                    // (the entry point has refused it)
}

template <int CAP>
int launch_modes(int mode, dim3 grid, hipStream_t st, const CombineArgs& a, const FieldArgs* f, const WeightArgs* w) {
    if (mode == SHG_STACK_MEAN) return launch_kernel<CAP, SHG_STACK_MEAN>(grid, st, a, f, w);
    if (mode == SHG_STACK_MEDIAN) return launch_kernel<CAP, SHG_STACK_MEDIAN>(grid, st, a, f, w);
    return launch_kernel<CAP, SHG_STACK_SIGMA>(grid, st, a, f, w);
}

int launch_combine(int mode, hipStream_t st, const CombineArgs& a, const FieldArgs* f, const WeightArgs* w) {
    const dim3 grid((unsigned)((a.ow + kLanesX * kOct - 1) / (kLanesX * kOct)), (unsigned)((a.oh + kRows - 1) / kRows));
    if (a.n <= 4) return launch_modes<4>(mode, grid, st, a, f, w);
    if (a.n <= 8) return launch_modes<8>(mode, grid, st, a, f, w);
    if (a.n <= 16) return launch_modes<16>(mode, grid, st, a, f, w);
    return launch_modes<32>(mode, grid, st, a, f, w);
}

using shg::overlap;
using shg::Span;
using shg::span_of;

// ---- SSD ----
constexpr int kTW = 64, kTH = 16;                 // the tile; a thread owns column threadIdx.x % 64 of rows threadIdx.x / 64 + 4 i
constexpr int kPerThread = kTW * kTH / kThreads;
constexpr int kRowStep = kThreads / kTW;
constexpr int kMaxS = 8;
constexpr int kLW = kTW + 2 * kMaxS, kLH = kTH + 2 * kMaxS;
constexpr int kMaxOffsets = (2 * kMaxS + 1) * (2 * kMaxS + 1);
constexpr int kSsdBlocks = 1024;

struct SsdArgs {
    const uint16_t* ref;
    const uint16_t* img;
    int64_t ref_pitch, img_pitch;
    int h, w, S, masked;
    double cx, cy, rad2;
    unsigned long long* ssd;
    int tiles_x, tiles;
};

__global__ __launch_bounds__(kThreads) void k_shift_ssd(const SsdArgs a) {
    __shared__ uint16_t tile[kLH * kLW];
    __shared__ unsigned long long acc[kMaxOffsets + 1];
    const int S = a.S, side = 2 * S + 1, n_off = side * side;
    for (int i = threadIdx.x; i <= n_off; i += kThreads) acc[i] = 0;
    const int lx = (int)threadIdx.x % kTW, ly = (int)threadIdx.x / kTW;
    const bool first_lane = shg::lane_id() == 0;
    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int tx0 = (t % a.tiles_x) * kTW, ty0 = (t / a.tiles_x) * kTH;
        const int c = tx0 + lx;
        const double dx = (double)c - a.cx, dx2 = dx * dx;
        uint32_t mine[kPerThread];
        bool valid[kPerThread];
        int n_valid = 0;
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
            const int r = ty0 + ly + i * kRowStep;
            bool ok = c >= S && c < a.w - S && r >= S && r < a.h - S;
            if (ok && a.masked) {
                const double dy = (double)r - a.cy, d2 = dx2 + dy * dy;
                ok = !(d2 > a.rad2);
            }
            valid[i] = ok;
            mine[i] = ok ? (uint32_t)a.ref[(int64_t)r * a.ref_pitch + c] : 0u;
            n_valid += ok ? 1 : 0;
        }
        // (a barrier too: the tile of the round before has been read by everyone, and the table is clear before its first use)
        if (!__syncthreads_or(n_valid)) continue;
        const int lw = kTW + 2 * S, lh = kTH + 2 * S;
        for (int i = threadIdx.x; i < lw * lh; i += kThreads) {
            const int y = i / lw, x = i % lw, gr = ty0 - S + y, gc = tx0 - S + x;
            // (outside the image: a pixel of the set never reads it)
            tile[y * kLW + x] = gr >= 0 && gr < a.h && gc >= 0 && gc < a.w ? a.img[(int64_t)gr * a.img_pitch + gc] : (uint16_t)0;
        }
        __syncthreads();
        const uint64_t total = shg::wave_sum((uint64_t)n_valid);
        if (first_lane && total) atomicAdd(&acc[n_off], (unsigned long long)total);
        for (int v = 0; v < side; ++v) {
            for (int u = 0; u < side; ++u) {
                uint64_t s = 0;
#pragma unroll
                for (int i = 0; i < kPerThread; ++i) {
                    const uint32_t other = tile[(ly + i * kRowStep + v) * kLW + lx + u];
                    const uint32_t d = mine[i] > other ? mine[i] - other : other - mine[i];
                    s += valid[i] ? (uint64_t)(d * d) : 0;           // d <= 65535: d * d < 2^32
                }
                s = shg::wave_sum(s);
                if (first_lane && s) atomicAdd(&acc[v * side + u], (unsigned long long)s);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= n_off; i += kThreads)
        if (acc[i]) atomicAdd(a.ssd + i, acc[i]);
}

// The byte spans of the two outputs (count: empty without a count plane, which overlaps nothing).
struct OutSpans {
    Span out, count;
};

// The checks and the argument struct the three combine entry points share, and the outputs' spans for the checks that follow.
// Nothing is written or launched.
int combine_args(const char* fn, const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4, int n, int mode,
                 double kappa, int iterations, uint16_t* out, int64_t oh, int64_t ow, int64_t out_pitch, uint8_t* count, int64_t count_pitch,
                 CombineArgs* args, OutSpans* spans) {
    SHG_REQUIRE(host_srcs && host_dims3 && host_xform4 && out, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(n >= 1 && n <= kMaxSources, SHG_E_ARG, "%s: %d sources (1 to %d)", fn, n, kMaxSources);
    SHG_REQUIRE(shg::image_dims_ok(oh, ow), SHG_E_UNSUPPORTED, "%s: an output of %lld x %lld (1 to %d either way)", fn, (long long)oh,
                (long long)ow, shg::kMaxImageDim);
    SHG_REQUIRE(out_pitch >= ow, SHG_E_ARG, "%s: output pitch < ow", fn);
    SHG_REQUIRE(!count || count_pitch >= ow, SHG_E_ARG, "%s: count pitch < ow", fn);
    SHG_REQUIRE(mode == SHG_STACK_MEAN || mode == SHG_STACK_MEDIAN || mode == SHG_STACK_SIGMA, SHG_E_ARG, "%s: unknown mode %d", fn, mode);
    SHG_REQUIRE(kappa >= 1.0, SHG_E_ARG, "%s: kappa %g is not a number or < 1", fn, kappa);
    SHG_REQUIRE(iterations >= 1 && iterations <= 3, SHG_E_ARG, "%s: %d iterations (1 to 3)", fn, iterations);
    const Span out_span = span_of(out, oh, ow, out_pitch, sizeof(uint16_t));
    const Span count_span = count ? span_of(count, oh, ow, count_pitch, 1) : Span{0, 0};
    SHG_REQUIRE(!overlap(out_span, count_span), SHG_E_ARG, "%s: the count plane overlaps the output", fn);
    *spans = OutSpans{out_span, count_span};
    CombineArgs& a = *args;
    for (int j = 0; j < n; ++j) {
        const int64_t h = host_dims3[3 * j], w = host_dims3[3 * j + 1], pitch = host_dims3[3 * j + 2];
        const double s = host_xform4[4 * j], tx = host_xform4[4 * j + 1], ty = host_xform4[4 * j + 2], gain = host_xform4[4 * j + 3];
        SHG_REQUIRE(host_srcs[j], SHG_E_ARG, "%s: source %d is a null pointer", fn, j);
        SHG_REQUIRE(shg::image_dims_ok(h, w), SHG_E_UNSUPPORTED, "%s: source %d of %lld x %lld (1 to %d either way)", fn, j, (long long)h,
                    (long long)w, shg::kMaxImageDim);
        SHG_REQUIRE(pitch >= w, SHG_E_ARG, "%s: source %d: pitch < w", fn, j);
        SHG_REQUIRE(isfinite(s) && s > 0.0, SHG_E_ARG, "%s: source %d: scale %g is not finite and > 0", fn, j, s);
        SHG_REQUIRE(isfinite(tx) && isfinite(ty), SHG_E_ARG, "%s: source %d: translation (%g, %g) is not finite", fn, j, tx, ty);
        SHG_REQUIRE(isfinite(gain) && gain >= 0.0, SHG_E_ARG, "%s: source %d: gain %g is negative or not finite", fn, j, gain);
        const Span src_span = span_of(host_srcs[j], h, w, pitch, sizeof(uint16_t));
        SHG_REQUIRE(!overlap(out_span, src_span), SHG_E_ARG, "%s: the output overlaps source %d", fn, j);
        SHG_REQUIRE(!overlap(count_span, src_span), SHG_E_ARG, "%s: the count plane overlaps source %d", fn, j);
        a.src[j] = SourceRec{host_srcs[j], (int)h, (int)w, pitch, s, tx, ty, gain};
    }
    a.out = out, a.count = count, a.oh = (int)oh, a.ow = (int)ow, a.out_pitch = out_pitch, a.count_pitch = count ? count_pitch : 0;
    a.n = n, a.iterations = iterations, a.kappa = kappa;
    a.vec_out = shg::rows_aligned(out, out_pitch, sizeof(uint16_t), 16);
    a.vec_count = count && shg::rows_aligned(count, count_pitch, sizeof(uint8_t), 8);
    return 0;
}

// The lattice `p` of source j -- `what`: "field" or "weight lattice", `row` doubles a row of nodes -- starts on `align` bytes and
// overlaps neither output.
int check_lattice(const char* fn, const char* what, int j, const double* p, int64_t gh, int64_t row, int align, const OutSpans& spans) {
    SHG_REQUIRE(reinterpret_cast<uintptr_t>(p) % align == 0, SHG_E_ARG, "%s: %s %d does not start on %d bytes", fn, what, j, align);
    const Span span = span_of(p, gh, row, row, sizeof(double));
    SHG_REQUIRE(!overlap(spans.out, span), SHG_E_ARG, "%s: the output overlaps %s %d", fn, what, j);
    SHG_REQUIRE(!overlap(spans.count, span), SHG_E_ARG, "%s: the count plane overlaps %s %d", fn, what, j);
    return 0;
}

// What the three entry points do.  lattice: the fields of `step` pixels a node (host_fields may be null as a whole: no source has
// one) and, with host_weights, the weight lattices; else the plain combine, and gh, gw, step are not read.
int combine(const char* fn, const char* tag, const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4,
            bool lattice, const double* const* host_fields, const double* const* host_weights, int64_t gh, int64_t gw, int step, int n, int mode,
            double kappa, int iterations, uint16_t* out, int64_t oh, int64_t ow, int64_t out_pitch, uint8_t* count, int64_t count_pitch,
            shg_stream_t stream) {
    SHG_REQUIRE(!lattice || (step >= kMinStep && step <= kMaxStep), SHG_E_ARG, "%s: a lattice step of %d pixels (%d to %d)", fn, step, kMinStep,
                kMaxStep);
    CombineArgs a{};
    FieldArgs f{};
    WeightArgs w{};
    OutSpans spans;
    if (const int e = combine_args(fn, host_srcs, host_dims3, host_xform4, n, mode, kappa, iterations, out, oh, ow, out_pitch, count,
                                   count_pitch, &a, &spans))
        return e;
    SHG_REQUIRE(!lattice || (gh == (oh - 1 + step - 1) / step + 1 && gw == (ow - 1 + step - 1) / step + 1), SHG_E_ARG,
                "%s: a lattice of %lld x %lld nodes does not cover %lld x %lld pixels at a step of %d", fn, (long long)gh, (long long)gw,
                (long long)oh, (long long)ow, step);
    for (int j = 0; lattice && host_fields && j < n; ++j) {
        f.field[j] = host_fields[j];
        if (const int e = f.field[j] ? check_lattice(fn, "field", j, f.field[j], gh, gw * 2, 16, spans) : 0) return e;
    }
    f.gh = (int)gh, f.gw = (int)gw, f.step = step;
    for (int j = 0; host_weights && j < n; ++j) {
        w.weight[j] = host_weights[j];
        if (const int e = w.weight[j] ? check_lattice(fn, "weight lattice", j, w.weight[j], gh, gw, 8, spans) : 0) return e;
    }
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF(tag, st);
    return launch_combine(mode, st, a, lattice ? &f : nullptr, host_weights ? &w : nullptr);
}

}  // namespace

extern "C" int shg_stack_combine_u16(const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4, int n, int mode,
                                     double kappa, int iterations, uint16_t* out, int64_t oh, int64_t ow, int64_t out_pitch, uint8_t* count,
                                     int64_t count_pitch, shg_stream_t stream) {
    return combine("shg_stack_combine_u16", "stack_combine", host_srcs, host_dims3, host_xform4, false, nullptr, nullptr, 0, 0, 0, n, mode, kappa,
                   iterations, out, oh, ow, out_pitch, count, count_pitch, stream);
}

extern "C" int shg_stack_combine_field_u16(const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4,
                                           const double* const* host_fields, int64_t gh, int64_t gw, int step, int n, int mode, double kappa,
                                           int iterations, uint16_t* out, int64_t oh, int64_t ow, int64_t out_pitch, uint8_t* count,
                                           int64_t count_pitch, shg_stream_t stream) {
    const char* fn = "shg_stack_combine_field_u16";
    SHG_REQUIRE(host_fields, SHG_E_ARG, "%s: null pointer", fn);
    return combine(fn, "stack_combine_field", host_srcs, host_dims3, host_xform4, true, host_fields, nullptr, gh, gw, step, n, mode, kappa,
                   iterations, out, oh, ow, out_pitch, count, count_pitch, stream);
}

extern "C" int shg_stack_combine_weighted_u16(const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4,
                                              const double* const* host_fields, const double* const* host_weights, int64_t gh, int64_t gw,
                                              int step, int n, int mode, double kappa, int iterations, uint16_t* out, int64_t oh, int64_t ow,
                                              int64_t out_pitch, uint8_t* count, int64_t count_pitch, shg_stream_t stream) {
    const char* fn = "shg_stack_combine_weighted_u16";
    SHG_REQUIRE(host_weights, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(mode != SHG_STACK_MEDIAN, SHG_E_ARG, "%s: there is no weighted median", fn);
    return combine(fn, "stack_combine_weighted", host_srcs, host_dims3, host_xform4, true, host_fields, host_weights, gh, gw, step, n, mode,
                   kappa, iterations, out, oh, ow, out_pitch, count, count_pitch, stream);
}

extern "C" int shg_shift_ssd_u16(const uint16_t* ref, int64_t ref_pitch, const uint16_t* img, int64_t img_pitch, int64_t h, int64_t w, int S,
                                 const double* circle3, uint64_t* ssd, shg_stream_t stream) {
    const char* fn = "shg_shift_ssd_u16";
    if (const int e = shg::check_images(fn, ref && img && ssd, "images", h, w, ref_pitch < img_pitch ? ref_pitch : img_pitch)) return e;
    SHG_REQUIRE(S >= 0 && S <= kMaxS, SHG_E_ARG, "%s: a search of %d pixels (0 to %d)", fn, S, kMaxS);
    SsdArgs a{};
    if (const int e = shg::parse_disk_mask(fn, circle3, &a.masked, &a.cx, &a.cy, &a.rad2)) return e;
    a.ref = ref, a.img = img, a.ref_pitch = ref_pitch, a.img_pitch = img_pitch, a.h = (int)h, a.w = (int)w, a.S = S;
    a.ssd = reinterpret_cast<unsigned long long*>(ssd);
    a.tiles_x = (int)((w + kTW - 1) / kTW);
    a.tiles = a.tiles_x * (int)((h + kTH - 1) / kTH);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("shift_ssd", st);
    const size_t words = (size_t)(2 * S + 1) * (2 * S + 1) + 1;
    if (const int e = shg::zero_async(fn, ssd, words * sizeof(uint64_t), st)) return e;
    if (w < 2 * S + 1 || h < 2 * S + 1) return 0;                        // the set is empty: the zeros are the result
    return shg::launch(k_shift_ssd, dim3((unsigned)(a.tiles < kSsdBlocks ? a.tiles : kSsdBlocks)), dim3(kThreads), 0, st, a, "k_shift_ssd");
}
