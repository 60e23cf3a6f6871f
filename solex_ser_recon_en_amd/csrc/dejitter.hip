// Scan jitter along the slit, taken out of the raw disks: the two limb crossings of every column (shg_column_limb_u16) and every
// column resampled along itself by its own sub-pixel shift (shg_column_shift_u16).  Not reference stages: the arithmetic is the one
// include/shg_hip.h states, all integers on the device, restated in NumPy by tests/dejitter_ref.py.  Both kernels put their lanes
// along the columns, eight columns a thread as k_ring_flatten (rings.hip) owns them: 16-byte accesses where every pitch and pointer
// allows, single elements otherwise.
//
// Crossings: a workgroup owns kLimbCols whole columns, so nothing is combined across workgroups.  Its kLimbSegs row segments -- one
// a thread of a column run -- each slide the window sum down their rows (one new row and the row that leaves the window per step:
// the second read hits the lines the first one fetched K rows earlier), keep the first rising and the last falling crossing they
// own, and meet in LDS: the minimum of the rising rows, the maximum of the falling rows and the two edge flags.  The thread whose
// crossing won writes its three words; every word of the table is written once, by plain stores.  No workspace, no scratch.
//
// Shifts: a copy with four taps a pixel.  The per-column offsets and weights travel by value in the kernel's arguments, as the other
// entry points pass small tables, kShiftCols columns a launch (16-bit fields: 10 bytes a column), one launch for all planes of a
// column chunk.  A thread walks kShiftRows rows of its eight columns and keeps the three taps it has already read: one two-byte
// read and a share of one 16-byte store a pixel.  Neighbouring columns read rows a few apart: the same few row segments.
#include "image_args.h"

#include <limits.h>

namespace {

constexpr int kOct = 8;                           // columns a thread owns

// ---- the crossings ----
constexpr int kLimbLanes = 8;                     // threads along the columns
constexpr int kLimbCols = kLimbLanes * kOct;      // columns a workgroup owns
constexpr int kLimbSegs = 128;                    // row segments a workgroup splits its columns into (ops.COLUMN_LIMB_SEGMENTS)
constexpr int kLimbThreads = kLimbLanes * kLimbSegs;

template <bool VEC, int LANES>
__device__ __forceinline__ int column_of(int base, int lx, int j) {
    return VEC ? base + lx * kOct + j : base + j * LANES + lx;
}

__device__ __forceinline__ void load8(const uint16_t* row, int c0, uint32_t* v) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + c0);
    v[0] = q.x & 0xFFFFu, v[1] = q.x >> 16, v[2] = q.y & 0xFFFFu, v[3] = q.y >> 16;
    v[4] = q.z & 0xFFFFu, v[5] = q.z >> 16, v[6] = q.w & 0xFFFFu, v[7] = q.w >> 16;
}

struct LimbArgs {
    const uint16_t* img;
    int32_t* out;                     // [w][6]
    int h, w;
    int64_t pitch;
    int k;                            // the window
    uint32_t kt;                      // K * T
};

template <bool VEC>
__device__ __forceinline__ void load_limb_run(const LimbArgs& a, int r, int base, int lx, bool whole, uint32_t* v) {
    const uint16_t* row = a.img + (int64_t)r * a.pitch;
    if (whole) {
        load8(row, base + lx * kOct, v);
    } else {
#pragma unroll
        for (int j = 0; j < kOct; ++j) {
            const int c = column_of<VEC, kLimbLanes>(base, lx, j);
            v[j] = c < a.w ? (uint32_t)row[c] : 0u;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kLimbThreads) void k_column_limb(const LimbArgs a) {
    __shared__ int s_top[kLimbCols], s_bot[kLimbCols], s_bad[kLimbCols];
    const int tid = (int)threadIdx.x, lx = tid % kLimbLanes, seg = tid / kLimbLanes;
    if (tid < kLimbCols) s_top[tid] = INT_MAX, s_bot[tid] = -1, s_bad[tid] = 0;
    __syncthreads();
    const int base = blockIdx.x * kLimbCols;
    const int c0 = column_of<VEC, kLimbLanes>(base, lx, 0);      // the thread's lowest column
    const bool whole = VEC && c0 + kOct <= a.w;
    const int ni = a.h - a.k + 1;                                // the window sums s[0 .. ni - 1]
    int top_i[kOct], bot_i[kOct];
    uint32_t top_p[kOct], top_c[kOct], bot_c[kOct], bot_n[kOct];
#pragma unroll
    for (int j = 0; j < kOct; ++j) top_i[j] = bot_i[j] = -1, top_p[j] = top_c[j] = bot_c[j] = bot_n[j] = 0u;
    const int len = (ni + kLimbSegs - 1) / kLimbSegs;
    const int own_lo = seg * len, own_hi = min(own_lo + len, ni);            // the segment owns the crossings at i in [own_lo, own_hi)
    if (c0 < a.w && ni >= 3 && own_lo < own_hi) {
        const int lo = max(own_lo - 1, 0), hi = min(own_hi, ni - 1);         // it needs s[lo .. hi]
        uint32_t s[kOct], v[kOct], u[kOct];
        bool bad[kOct];
#pragma unroll
        for (int j = 0; j < kOct; ++j) s[j] = 0u;
        for (int k = 0; k < a.k; ++k) {
            load_limb_run<VEC>(a, lo + k, base, lx, whole, v);
#pragma unroll
            for (int j = 0; j < kOct; ++j) s[j] += v[j];
        }
#pragma unroll
        for (int j = 0; j < kOct; ++j) bad[j] = own_lo == 0 && s[j] >= a.kt;             // A[0]
        for (int i = lo + 1; i <= hi; ++i) {
            load_limb_run<VEC>(a, i + a.k - 1, base, lx, whole, v);
            load_limb_run<VEC>(a, i - 1, base, lx, whole, u);
            const bool rise_mine = i < own_hi, fall_mine = i - 1 >= own_lo;
#pragma unroll
            for (int j = 0; j < kOct; ++j) {
                const uint32_t cur = s[j] + v[j] - u[j];
                const bool ap = s[j] >= a.kt, ac = cur >= a.kt;
                if (rise_mine && !ap && ac && top_i[j] < 0) top_i[j] = i, top_p[j] = s[j], top_c[j] = cur;
                if (fall_mine && ap && !ac) bot_i[j] = i - 1, bot_c[j] = s[j], bot_n[j] = cur;
                s[j] = cur;
            }
        }
#pragma unroll
        for (int j = 0; j < kOct; ++j) {
            if (own_hi == ni && s[j] >= a.kt) bad[j] = true;                             // A[ni - 1]: s is s[hi] = s[ni - 1] here
            const int c = column_of<VEC, kLimbLanes>(base, lx, j);
            if (c >= a.w) continue;
            if (top_i[j] >= 0) atomicMin(&s_top[c - base], top_i[j]);
            if (bot_i[j] >= 0) atomicMax(&s_bot[c - base], bot_i[j]);
            if (bad[j]) atomicOr(&s_bad[c - base], 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kOct; ++j) {
        const int c = column_of<VEC, kLimbLanes>(base, lx, j);
        if (c >= a.w) continue;
        const int top = s_top[c - base], bot = s_bot[c - base];
        int32_t* o = a.out + (int64_t)c * 6;
        // (a rising crossing between two sums below the threshold at both ends is followed by a falling one)
        if (s_bad[c - base] || top == INT_MAX) {
            if (seg == 0) o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = -1;
            continue;
        }
        if (top_i[j] == top) o[0] = top, o[1] = (int32_t)top_p[j], o[2] = (int32_t)top_c[j];
        if (bot_i[j] == bot) o[3] = bot, o[4] = (int32_t)bot_c[j], o[5] = (int32_t)bot_n[j];
    }
}

// ---- the shifts ----
constexpr int kShiftLanes = 32;                   // threads along the columns
constexpr int kShiftCols = kShiftLanes * kOct;    // columns a launch carries in its arguments
constexpr int kShiftRowLanes = 8;
constexpr int kShiftThreads = kShiftLanes * kShiftRowLanes;
constexpr int kShiftRows = 16;                    // rows a thread walks
constexpr int kMaxPlanes = 64;
constexpr int kMaxOffset = 16384;
constexpr int kWeightLo = -4096, kWeightHi = 20480, kWeightOne = 16384;

struct ShiftArgs {
    const uint16_t* img;
    uint16_t* out;
    int h, w, c_base;                 // c_base: the first column of this launch's chunk
    int64_t pitch, plane_stride, out_pitch, out_plane_stride;
    int16_t offset[kShiftCols];
    int16_t weight[kShiftCols][4];
};
static_assert(sizeof(ShiftArgs) <= 4096, "the kernel's arguments");

template <bool VEC>
__global__ __launch_bounds__(kShiftThreads) void k_column_shift(const ShiftArgs a) {
    const int tid = (int)threadIdx.x, lx = tid % kShiftLanes, ly = tid / kShiftLanes;
    const int c0 = column_of<VEC, kShiftLanes>(a.c_base, lx, 0);
    const int r0 = ((int)blockIdx.x * kShiftRowLanes + ly) * kShiftRows, r1 = min(r0 + kShiftRows, a.h);
    if (c0 >= a.w || r0 >= a.h) return;
    const bool whole = VEC && c0 + kOct <= a.w;
    const uint16_t* img = a.img + (int64_t)blockIdx.y * a.plane_stride;
    uint16_t* out = a.out + (int64_t)blockIdx.y * a.out_plane_stride;
    const int hm = a.h - 1;
    int off[kOct], wt[kOct][4];
    int p0[kOct], p1[kOct], p2[kOct];
    const uint16_t* col[kOct];
#pragma unroll
    for (int j = 0; j < kOct; ++j) {
        const int c = column_of<VEC, kShiftLanes>(a.c_base, lx, j);
        const int slot = c - a.c_base, cc = min(c, a.w - 1);                 // (a column beyond w reads the last one and stores nothing)
        off[j] = a.offset[slot];
#pragma unroll
        for (int k = 0; k < 4; ++k) wt[j][k] = a.weight[slot][k];
        col[j] = img + cc;
        const int r = r0 + off[j];
        p0[j] = col[j][(int64_t)min(max(r - 1, 0), hm) * a.pitch];
        p1[j] = col[j][(int64_t)min(max(r, 0), hm) * a.pitch];
        p2[j] = col[j][(int64_t)min(max(r + 1, 0), hm) * a.pitch];
    }
    for (int r = r0; r < r1; ++r) {
        uint32_t v[kOct];
#pragma unroll
        for (int j = 0; j < kOct; ++j) {
            const int p3 = col[j][(int64_t)min(max(r + off[j] + 2, 0), hm) * a.pitch];
            const int64_t acc = (int64_t)wt[j][0] * p0[j] + (int64_t)wt[j][1] * p1[j] + (int64_t)wt[j][2] * p2[j] + (int64_t)wt[j][3] * p3;
            const int64_t q = (acc + 8192) >> 14;
            v[j] = (uint32_t)(q < 0 ? 0 : q > 65535 ? 65535 : q);
            p0[j] = p1[j], p1[j] = p2[j], p2[j] = p3;
        }
        uint16_t* orow = out + (int64_t)r * a.out_pitch;
        if (whole) {
            uint4 q;
            q.x = v[0] | v[1] << 16, q.y = v[2] | v[3] << 16, q.z = v[4] | v[5] << 16, q.w = v[6] | v[7] << 16;
            *reinterpret_cast<uint4*>(orow + c0) = q;
        } else {
#pragma unroll
            for (int j = 0; j < kOct; ++j) {
                const int c = column_of<VEC, kShiftLanes>(a.c_base, lx, j);
                if (c < a.w) orow[c] = (uint16_t)v[j];
            }
        }
    }
}

// [p, ...) of n planes of h x w
shg::Span stack_span(const void* p, int64_t n, int64_t h, int64_t w, int64_t pitch, int64_t plane_stride) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + (uintptr_t)((n - 1) * plane_stride + (h - 1) * pitch + w) * sizeof(uint16_t)};
}

}  // namespace

extern "C" int shg_column_limb_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, int window, int threshold, int32_t* out6,
                                   shg_stream_t stream) {
    const char* fn = "shg_column_limb_u16";
    if (const int e = shg::check_images(fn, img && out6, "an image", h, w, pitch)) return e;
    SHG_REQUIRE(window >= 1 && window <= 15 && window % 2 == 1, SHG_E_ARG, "%s: a window of %d (odd, 1 to 15)", fn, window);
    SHG_REQUIRE(threshold >= 0 && threshold <= 65535, SHG_E_ARG, "%s: a threshold of %d (0 to 65535)", fn, threshold);
    const shg::Span table{reinterpret_cast<uintptr_t>(out6), reinterpret_cast<uintptr_t>(out6) + (uintptr_t)w * 6 * sizeof(int32_t)};
    SHG_REQUIRE(!shg::overlap(table, shg::span_of(img, h, w, pitch, sizeof(uint16_t))), SHG_E_ARG, "%s: the table overlaps the image", fn);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("column_limb", st);
    LimbArgs a{};
    a.img = img, a.out = out6, a.h = (int)h, a.w = (int)w, a.pitch = pitch, a.k = window, a.kt = (uint32_t)window * (uint32_t)threshold;
    const bool vec = shg::rows_aligned(img, pitch, sizeof(uint16_t), 16);
    const dim3 grid((unsigned)((w + kLimbCols - 1) / kLimbCols));
    return shg::launch(vec ? k_column_limb<true> : k_column_limb<false>, grid, dim3(kLimbThreads), 0, st, a, "k_column_limb");
}

extern "C" int shg_column_shift_u16(const uint16_t* img, int n, int64_t h, int64_t w, int64_t pitch, int64_t plane_stride,
                                    const int32_t* host_offset, const int32_t* host_weight4, uint16_t* out, int64_t out_pitch,
                                    int64_t out_plane_stride, shg_stream_t stream) {
    const char* fn = "shg_column_shift_u16";
    if (const int e = shg::check_images(fn, img && out && host_offset && host_weight4, "images", h, w, pitch < out_pitch ? pitch : out_pitch))
        return e;
    SHG_REQUIRE(n >= 1 && n <= kMaxPlanes, SHG_E_ARG, "%s: %d planes (1 to %d)", fn, n, kMaxPlanes);
    const int64_t plane = (h - 1) * pitch + w, out_plane = (h - 1) * out_pitch + w;
    SHG_REQUIRE(n == 1 || (plane_stride >= plane && out_plane_stride >= out_plane), SHG_E_ARG, "%s: a plane stride below a plane", fn);
    SHG_REQUIRE(plane_stride >= 0 && plane_stride <= ((int64_t)1 << 40) && out_plane_stride >= 0 && out_plane_stride <= ((int64_t)1 << 40),
                SHG_E_ARG, "%s: a plane stride outside [0, 2^40]", fn);
    for (int64_t c = 0; c < w; ++c) {
        const int32_t* q = host_weight4 + 4 * c;
        SHG_REQUIRE(host_offset[c] >= -kMaxOffset && host_offset[c] <= kMaxOffset, SHG_E_ARG, "%s: column %lld has an offset of %d (|offset| <= %d)",
                    fn, (long long)c, host_offset[c], kMaxOffset);
        for (int k = 0; k < 4; ++k)
            SHG_REQUIRE(q[k] >= kWeightLo && q[k] <= kWeightHi, SHG_E_ARG, "%s: column %lld has a weight of %d (%d to %d)", fn, (long long)c, q[k],
                        kWeightLo, kWeightHi);
        SHG_REQUIRE(q[0] + q[1] + q[2] + q[3] == kWeightOne, SHG_E_ARG, "%s: the weights of column %lld sum to %d, not %d", fn, (long long)c,
                    q[0] + q[1] + q[2] + q[3], kWeightOne);
    }
    SHG_REQUIRE(!shg::overlap(stack_span(out, n, h, w, out_pitch, out_plane_stride), stack_span(img, n, h, w, pitch, plane_stride)), SHG_E_ARG,
                "%s: the output overlaps the image", fn);
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("column_shift", st);
    const bool vec = shg::rows_aligned(out, out_pitch, sizeof(uint16_t), 16) && (out_plane_stride * (int64_t)sizeof(uint16_t)) % 16 == 0;
    const dim3 grid((unsigned)((h + kShiftRowLanes * kShiftRows - 1) / (kShiftRowLanes * kShiftRows)), (unsigned)n);
    ShiftArgs a{};
    a.img = img, a.out = out, a.h = (int)h, a.w = (int)w;
    a.pitch = pitch, a.plane_stride = plane_stride, a.out_pitch = out_pitch, a.out_plane_stride = out_plane_stride;
    for (int64_t c_base = 0; c_base < w; c_base += kShiftCols) {
        a.c_base = (int)c_base;
        for (int i = 0; i < kShiftCols; ++i) {
            const int64_t c = c_base + i < w ? c_base + i : w - 1;
            a.offset[i] = (int16_t)host_offset[c];
            for (int k = 0; k < 4; ++k) a.weight[i][k] = (int16_t)host_weight4[4 * c + k];
        }
        if (const int e = shg::launch(vec ? k_column_shift<true> : k_column_shift<false>, grid, dim3(kShiftThreads), 0, st, a, "k_column_shift"))
            return e;
    }
    return 0;
}
