// Flattening the disk: the median of every one-pixel annulus around the fitted centre (shg_ring_medians_u16) and the division by
// that profile (shg_ring_flatten_u16).  Not a reference stage: the arithmetic is the one include/shg_hip.h states, restated in NumPy
// by tests/flatten_ref.py.  The host turns the medians into a gain a ring (flatten.py); the GPU counts and multiplies.
//
// Ring medians: a two-level radix select a ring, high byte then low byte, over [K][256] tables of 32-bit counts in the workspace.
//   hipMemsetAsync          the three tables
//   k_ring_hist<.., false>  T0[k][v >> 8] += 1 for every on-disk pixel of ring k
//   k_ring_pick_high        a wave a ring: count[k], the high bytes that hold the ranks (n - 1) / 2 and n / 2, the ranks left in them
//   k_ring_hist<.., true>   T1[k][v & 255] += 1 where v >> 8 is the lower rank's high byte; T2 the same for the upper rank's, only
//                           where the two differ (an even count whose middle pair straddles a high byte)
//   k_ring_pick_low         a wave a ring: lo[k], hi[k]
// The histogram passes work on Cartesian tiles.  The pixel centres of a TW x TH tile lie in a rectangle whose diagonal is
// D = sqrt((TW - 1)^2 + (TH - 1)^2); by the triangle inequality the distances from ANY point -- a centre far outside the image
// included -- to two points of the rectangle differ by at most D, so the rings floor(distance) a tile touches number at most
// floor(D) + 2.  The rounding of d2 (2^-52 relative) moves a distance by far less than D's distance to the next integer for the two
// tiles used: 64 x 64 (D = 89.1: 91 rings, 96 kept) and 32 x 32 (D = 43.8: 45 rings, 48 kept).  A workgroup finds its lowest ring,
// counts into [rings][256] 16-bit counters in LDS, two a word (a tile holds at most 4096 pixels: a counter cannot reach 65536, so
// the lower half never carries into the upper), and adds only the non-zero ones to the tables with device-scope integer atomics.
// A ring beyond the kept ones -- which the bound rules out -- would be counted straight into the tables, never out of bounds.
// Everything accumulated is an integer count: neither the grid nor the order of the atomics can change a bit.
//
// Flatten: the column ownership of k_map_detrend (detrend.hip), eight columns a thread, 16-byte loads and stores where both pitches
// and pointers allow.  The gain table reaches the kernel by value, in the kernel's arguments, as the other entry points pass small
// host arrays; 4 KB of arguments hold 449 doubles, so a call is cut into launches that each own 448 consecutive table intervals
// (one launch up to K = 448, three for a 2000 x 2000 product).  A launch skips, before it loads anything, the thread rows whose
// pixels all lie clear of its annulus.  A pixel is written by one launch only, and by the thread that read it: in place is safe.
#include "image_args.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRings = 16384;
constexpr size_t kTableBytes = 256 * sizeof(uint32_t);        // one ring's 256 counts
constexpr size_t kStateBytes = 4 * sizeof(uint32_t);          // one ring's {high byte, rank left} x {lower, upper}
constexpr uint32_t kNoByte = 0xFFFF;                          // the "high byte" of a ring without pixels: no sample has it

// The ring of a pixel: the largest k with (double)k * (double)k <= d2.  sqrt is within an ulp, so its truncation is within one of k.
__device__ __forceinline__ int ring_of(double d2) {
    int k = (int)sqrt(d2);
    if ((double)k * (double)k > d2) --k;
    else if ((double)(k + 1) * (double)(k + 1) <= d2) ++k;
    return k;
}

struct HistArgs {
    const uint16_t* img;
    int h, w;
    int64_t pitch;
    double cx, cy, rad2;
    int n_rings;
    uint32_t* tables;                 // first pass: T0; second pass: T1, with T2 n_rings * 256 words behind it
    const uint4* state;               // second pass: what k_ring_pick_high left
};

// One workgroup: the TW x TH tile at (blockIdx.x * TW, blockIdx.y * TH).  SECOND: the low-byte pass.
template <int TW, int TH, int RINGS, bool SECOND>
__global__ __launch_bounds__(kThreads) void k_ring_hist(const HistArgs a) {
    constexpr int kPerThread = TW * TH / kThreads, kRowStep = kThreads / TW, kTables = SECOND ? 2 : 1, kWords = RINGS * kTables * 128;
    static_assert(TW * TH % kThreads == 0 && kThreads % TW == 0 && TW * TH < 65536, "tile");
    __shared__ uint32_t cnt[kWords];              // [ring][table][128]: two 16-bit counters a word
    __shared__ uint32_t sel[RINGS];               // SECOND: lower rank's high byte | upper rank's << 16
    __shared__ int s_base;
    for (int i = threadIdx.x; i < kWords; i += kThreads) cnt[i] = 0;
    if (threadIdx.x == 0) s_base = INT_MAX;
    __syncthreads();
    const int c = blockIdx.x * TW + (int)threadIdx.x % TW, r0 = blockIdx.y * TH + (int)threadIdx.x / TW;
    const double dx = (double)c - a.cx, dx2 = dx * dx;
    int ring[kPerThread];
    uint32_t v[kPerThread];
    int lowest = INT_MAX;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        const int r = r0 + i * kRowStep;
        const double dy = (double)r - a.cy, d2 = dx2 + dy * dy;
        ring[i] = -1;
        v[i] = 0;
        if (c < a.w && r < a.h && !(d2 > a.rad2)) {
            const int k = ring_of(d2);
            if (k < a.n_rings) {                  // (always: rad < floor(rad) + 1)
                ring[i] = k;
                v[i] = a.img[(int64_t)r * a.pitch + c];
                lowest = min(lowest, k);
            }
        }
    }
    if (lowest != INT_MAX) atomicMin(&s_base, lowest);
    __syncthreads();
    const int base = s_base;
    if (base == INT_MAX) return;                  // no pixel of the tile lies on the disk
    if (SECOND) {
        for (int i = threadIdx.x; i < RINGS; i += kThreads) {
            const int k = base + i;
            uint32_t s = kNoByte | (kNoByte << 16);
            if (k < a.n_rings) {
                const uint4 st = a.state[k];
                s = st.x | (st.z << 16);
            }
            sel[i] = s;
        }
        __syncthreads();
    }
    uint32_t* const upper = a.tables + (int64_t)a.n_rings * 256;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
        if (ring[i] < 0) continue;
        const int idx = ring[i] - base;
        if (!SECOND) {
            const uint32_t bin = v[i] >> 8;
            if (idx < RINGS) atomicAdd(&cnt[idx * 128 + (bin >> 1)], 1u << (16 * (bin & 1)));
            else atomicAdd(a.tables + (int64_t)ring[i] * 256 + bin, 1u);
        } else {
            const uint32_t high = v[i] >> 8, bin = v[i] & 255u;
            uint32_t s;
            if (idx < RINGS) {
                s = sel[idx];
            } else {
                const uint4 st = a.state[ring[i]];
                s = st.x | (st.z << 16);
            }
            const uint32_t b_lo = s & 0xFFFFu, b_hi = s >> 16;
            const bool in_lo = high == b_lo, in_hi = high == b_hi && b_hi != b_lo;
            if (idx < RINGS) {
                if (in_lo) atomicAdd(&cnt[idx * 256 + (bin >> 1)], 1u << (16 * (bin & 1)));
                if (in_hi) atomicAdd(&cnt[idx * 256 + 128 + (bin >> 1)], 1u << (16 * (bin & 1)));
            } else {
                if (in_lo) atomicAdd(a.tables + (int64_t)ring[i] * 256 + bin, 1u);
                if (in_hi) atomicAdd(upper + (int64_t)ring[i] * 256 + bin, 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kWords; i += kThreads) {
        const uint32_t word = cnt[i];
        if (word == 0) continue;
        const int idx = i / (kTables * 128), rest = i % (kTables * 128), k = base + idx;
        if (k >= a.n_rings) continue;             // (a counter of a ring that does not exist is never touched)
        uint32_t* dst = (rest >= 128 ? upper : a.tables) + (int64_t)k * 256 + (rest % 128) * 2;
        if (word & 0xFFFFu) atomicAdd(dst, word & 0xFFFFu);
        if (word >> 16) atomicAdd(dst + 1, word >> 16);
    }
}

// The bin of a ring's 256 counts that holds rank `rank` (0-based): four bins a lane, a prefix sum over the wave.  -> true in the one
// lane whose bins hold it, with the bin and the rank left inside it; *total (every lane): the sum of the counts.
__device__ __forceinline__ bool wave_pick(const uint32_t* table, uint32_t rank, uint32_t* bin, uint32_t* left, uint32_t* total) {
    const int lane = shg::lane_id();
    const uint4 c = *reinterpret_cast<const uint4*>(table + lane * 4);
    const uint32_t s = c.x + c.y + c.z + c.w;
    const uint32_t incl = (uint32_t)shg::wave_scan((int)s);          // (a ring holds fewer than 2^28 pixels)
    *total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t before = incl - s;
    if (!(before <= rank && rank < incl)) return false;
    uint32_t b = 0;
    if (rank >= before + c.x) {
        before += c.x, b = 1;
        if (rank >= before + c.y) {
            before += c.y, b = 2;
            if (rank >= before + c.z) before += c.z, b = 3;
        }
    }
    *bin = (uint32_t)lane * 4 + b;
    *left = rank - before;
    return true;
}

struct PickArgs {
    uint32_t* tables;                 // T0 | T1 | T2
    uint32_t* state;                  // [K][4]: high byte and rank left of the lower rank, then of the upper
    int n_rings;
    uint32_t* count;
    uint16_t* lo;
    uint16_t* hi;
};

// One wave a ring: n = the ring's pixels, the high bytes holding the ranks (n - 1) / 2 and n / 2.
__global__ __launch_bounds__(kThreads) void k_ring_pick_high(const PickArgs a) {
    const int k = blockIdx.x * (kThreads / shg::kWave) + (int)threadIdx.x / shg::kWave;
    if (k >= a.n_rings) return;
    const uint32_t* t0 = a.tables + (int64_t)k * 256;
    uint32_t* st = a.state + (int64_t)k * 4;
    uint32_t bin = 0, left = 0, n = 0;
    const uint4 c = *reinterpret_cast<const uint4*>(t0 + shg::lane_id() * 4);
    n = shg::wave_sum(c.x + c.y + c.z + c.w);
    if (n == 0) {
        if (shg::lane_id() == 0) {
            a.count[k] = 0;
            st[0] = kNoByte, st[1] = 0, st[2] = kNoByte, st[3] = 0;
        }
        return;
    }
    if (shg::lane_id() == 0) a.count[k] = n;
    uint32_t total;
    if (wave_pick(t0, (n - 1) / 2, &bin, &left, &total)) st[0] = bin, st[1] = left;
    if (wave_pick(t0, n / 2, &bin, &left, &total)) st[2] = bin, st[3] = left;
}

// One wave a ring: the low bytes.
__global__ __launch_bounds__(kThreads) void k_ring_pick_low(const PickArgs a) {
    const int k = blockIdx.x * (kThreads / shg::kWave) + (int)threadIdx.x / shg::kWave;
    if (k >= a.n_rings) return;
    const uint32_t* st = a.state + (int64_t)k * 4;
    const uint32_t b_lo = st[0], r_lo = st[1], b_hi = st[2], r_hi = st[3];
    if (b_lo == kNoByte) {
        if (shg::lane_id() == 0) a.lo[k] = 0, a.hi[k] = 0;
        return;
    }
    const uint32_t* t1 = a.tables + ((int64_t)a.n_rings + k) * 256;
    const uint32_t* t2 = b_hi == b_lo ? t1 : a.tables + (2 * (int64_t)a.n_rings + k) * 256;
    uint32_t bin = 0, left = 0, total;
    if (wave_pick(t1, r_lo, &bin, &left, &total)) a.lo[k] = (uint16_t)(b_lo << 8 | bin);
    if (wave_pick(t2, r_hi, &bin, &left, &total)) a.hi[k] = (uint16_t)(b_hi << 8 | bin);
}

// ---- flatten ----
constexpr int kOct = 8;                           // columns a thread owns
constexpr int kChunk = kThreads * kOct;           // columns a workgroup spans
constexpr int kWindow = 448;                      // table intervals a launch owns: 449 doubles and the rest stay below 4 KB
constexpr int kFlattenRows = 8;                   // rows a workgroup handles

struct FlattenArgs {
    const uint16_t* src;
    uint16_t* out;
    int h, w;
    int64_t pitch, out_pitch;
    double cx, cy, rad2;
    int n_rings;
    int j0, j1;                       // the launch owns the on-disk pixels whose table index lies in [j0, j1)
    int copy;                         // 1: it also writes every other pixel as it is (the first launch of a call out of place)
    double gain[kWindow + 1];         // gain[j0 ..]
};
static_assert(sizeof(FlattenArgs) <= 4096, "kernel arguments");

template <bool VEC>
__device__ __forceinline__ int flatten_column(int j) {
    const int base = blockIdx.x * kChunk;
    return VEC ? base + (int)threadIdx.x * kOct + j : base + j * kThreads + (int)threadIdx.x;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_ring_flatten(const FlattenArgs a) {
    const int c0 = flatten_column<VEC>(0);
    if (c0 >= a.w) return;
    double dx2[kOct], near2 = INFINITY, far2 = 0.0;
#pragma unroll
    for (int j = 0; j < kOct; ++j) {
        const int c = flatten_column<VEC>(j);
        const double dx = (double)c - a.cx;
        dx2[j] = dx * dx;
        if (c < a.w) near2 = fmin(near2, dx2[j]), far2 = fmax(far2, dx2[j]);
    }
    const bool whole = VEC && c0 + kOct <= a.w;
    // the annulus of the launch, a pixel and a half wider either way than the radii its table indices stand for
    const double inner = (double)(a.j0 - 1), outer = (double)(a.j1 + 2), inner2 = inner * inner, outer2 = outer * outer;
    const double top = (double)(a.n_rings - 1);
    const int r0 = blockIdx.y * kFlattenRows, r1 = min(r0 + kFlattenRows, a.h);
    for (int r = r0; r < r1; ++r) {
        const double dy = (double)r - a.cy, dy2 = dy * dy;
        if (!a.copy && ((a.j0 > 0 && far2 + dy2 < inner2) || (a.j1 < a.n_rings && near2 + dy2 > outer2))) continue;
        const uint16_t* srow = a.src + (int64_t)r * a.pitch;
        uint16_t v[kOct];
        if (whole) {
            const uint4 q = *reinterpret_cast<const uint4*>(srow + c0);
            v[0] = (uint16_t)q.x, v[1] = (uint16_t)(q.x >> 16), v[2] = (uint16_t)q.y, v[3] = (uint16_t)(q.y >> 16);
            v[4] = (uint16_t)q.z, v[5] = (uint16_t)(q.z >> 16), v[6] = (uint16_t)q.w, v[7] = (uint16_t)(q.w >> 16);
        } else {
#pragma unroll
            for (int j = 0; j < kOct; ++j) {
                const int c = flatten_column<VEC>(j);
                v[j] = c < a.w ? srow[c] : (uint16_t)0;
            }
        }
        bool mine[kOct], any = false;
#pragma unroll
        for (int j = 0; j < kOct; ++j) {
            const double d2 = dx2[j] + dy2;
            mine[j] = false;
            if (d2 > a.rad2) continue;
            const double u = sqrt(d2) - 0.5;
            const bool between = u > 0.0 && u < top;
            const int e = u <= 0.0 ? 0 : between ? (int)u : a.n_rings - 1;      // the table index the pixel belongs to (u < 16384)
            if (e < a.j0 || e >= a.j1) continue;
            double g = a.gain[e - a.j0];
            if (between) {
                const double t = u - (double)e, g1 = a.gain[e - a.j0 + 1];
                g = g + (g1 - g) * t;
            }
            v[j] = (uint16_t)fmin(fmax(rint((double)v[j] * g), 0.0), 65535.0);
            mine[j] = true;
            any = true;
        }
        if (!any && !a.copy) continue;
        uint16_t* orow = a.out + (int64_t)r * a.out_pitch;
        if (whole) {
            uint4 q;
            q.x = (uint32_t)v[0] | (uint32_t)v[1] << 16, q.y = (uint32_t)v[2] | (uint32_t)v[3] << 16;
            q.z = (uint32_t)v[4] | (uint32_t)v[5] << 16, q.w = (uint32_t)v[6] | (uint32_t)v[7] << 16;
            *reinterpret_cast<uint4*>(orow + c0) = q;        // (the pixels of other launches go back as they were read)
        } else {
#pragma unroll
            for (int j = 0; j < kOct; ++j) {
                const int c = flatten_column<VEC>(j);
                if (c < a.w && (mine[j] || a.copy)) orow[c] = v[j];
            }
        }
    }
}

int check_circle(const char* fn, const double* circle3, int64_t n_rings) {
    SHG_REQUIRE(circle3, SHG_E_ARG, "%s: null pointer", fn);
    const double cx = circle3[0], cy = circle3[1], rad = circle3[2];
    SHG_REQUIRE(isfinite(cx) && isfinite(cy) && isfinite(rad), SHG_E_ARG, "%s: the circle (%g, %g, %g) is not finite", fn, cx, cy, rad);
    SHG_REQUIRE(rad >= 0.0 && rad < (double)kMaxRings, SHG_E_ARG, "%s: radius %g outside [0, %d)", fn, rad, kMaxRings);
    SHG_REQUIRE(fabs(cx) < 65536.0 && fabs(cy) < 65536.0, SHG_E_ARG, "%s: centre (%g, %g) beyond 65536", fn, cx, cy);
    SHG_REQUIRE(n_rings == (int64_t)floor(rad) + 1, SHG_E_ARG, "%s: %lld rings for radius %g (floor(rad) + 1 = %lld)", fn, (long long)n_rings,
                rad, (long long)floor(rad) + 1);
    return 0;
}

size_t medians_bytes(int64_t n_rings) { return (size_t)n_rings * (3 * kTableBytes + kStateBytes) + shg::kWorkspaceAlign; }

}  // namespace

extern "C" size_t shg_ring_medians_u16_workspace_bytes(int64_t n_rings) {
    return n_rings >= 1 && n_rings <= kMaxRings ? medians_bytes(n_rings) : 0;
}

extern "C" int shg_ring_medians_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, int64_t n_rings,
                                    uint32_t* count, uint16_t* lo, uint16_t* hi, void* workspace, size_t workspace_bytes,
                                    shg_stream_t stream) {
    const char* fn = "shg_ring_medians_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(count && lo && hi && workspace, SHG_E_ARG, "%s: null pointer", fn);
    if (const int e = check_circle(fn, circle3, n_rings)) return e;
    SHG_REQUIRE(workspace_bytes >= medians_bytes(n_rings), SHG_E_ARG, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes,
                medians_bytes(n_rings));
    const int K = (int)n_rings;
    uint32_t* tables = reinterpret_cast<uint32_t*>(shg::align_up(workspace, shg::kWorkspaceAlign));
    uint32_t* state = tables + 3 * (size_t)K * 256;
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("ring_medians", st);
    if (const int e = shg::zero_async(fn, tables, 3 * (size_t)K * kTableBytes, st)) return e;
    HistArgs ha{img, (int)h, (int)w, pitch, circle3[0], circle3[1], circle3[2] * circle3[2], K, tables, nullptr};
    const PickArgs pa{tables, state, K, count, lo, hi};
    const dim3 picks((unsigned)((K + 3) / 4));
    if (const int e = shg::launch(k_ring_hist<64, 64, 96, false>, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 63) / 64)), dim3(kThreads),
                                  0, st, ha, "k_ring_hist (high bytes)"))
        return e;
    if (const int e = shg::launch(k_ring_pick_high, picks, dim3(kThreads), 0, st, pa, "k_ring_pick_high")) return e;
    ha.tables = tables + (size_t)K * 256;
    ha.state = reinterpret_cast<const uint4*>(state);
    if (const int e = shg::launch(k_ring_hist<32, 32, 48, true>, dim3((unsigned)((w + 31) / 32), (unsigned)((h + 31) / 32)), dim3(kThreads),
                                  0, st, ha, "k_ring_hist (low bytes)"))
        return e;
    return shg::launch(k_ring_pick_low, picks, dim3(kThreads), 0, st, pa, "k_ring_pick_low");
}

extern "C" int shg_ring_flatten_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, const double* gain,
                                    int64_t n_rings, uint16_t* out, int64_t out_pitch, shg_stream_t stream) {
    const char* fn = "shg_ring_flatten_u16";
    if (const int e = shg::check_image(fn, img, h, w, pitch)) return e;
    SHG_REQUIRE(gain && out, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(out_pitch >= w, SHG_E_ARG, "%s: output pitch < w", fn);
    if (const int e = check_circle(fn, circle3, n_rings)) return e;
    for (int64_t k = 0; k < n_rings; ++k)
        SHG_REQUIRE(isfinite(gain[k]) && gain[k] >= 0.0, SHG_E_ARG, "%s: gain[%lld] = %g is negative or not finite", fn, (long long)k, gain[k]);
    SHG_REQUIRE(out != img || out_pitch == pitch, SHG_E_ARG, "%s: in place needs equal pitches", fn);
    const int K = (int)n_rings;
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("ring_flatten", st);
    const dim3 grid((unsigned)((w + kChunk - 1) / kChunk), (unsigned)((h + kFlattenRows - 1) / kFlattenRows));
    FlattenArgs a{};
    a.out = out, a.h = (int)h, a.w = (int)w, a.out_pitch = out_pitch;
    a.cx = circle3[0], a.cy = circle3[1], a.rad2 = circle3[2] * circle3[2], a.n_rings = K;
    for (int j0 = 0; j0 < K; j0 += kWindow) {
        // the first launch of a call out of place writes the whole output; the others then work in place on it
        a.src = j0 == 0 ? img : out;
        a.pitch = j0 == 0 ? pitch : out_pitch;
        a.copy = j0 == 0 && out != img;
        a.j0 = j0, a.j1 = j0 + kWindow < K ? j0 + kWindow : K;
        const int last = a.j1 < K ? a.j1 : K - 1;                    // the interval [j1 - 1, j1) reads gain[j1] too
        for (int j = j0; j <= last; ++j) a.gain[j - j0] = gain[j];
        const bool vec = shg::rows_aligned(a.src, a.pitch, sizeof(uint16_t), 16) && shg::rows_aligned(out, out_pitch, sizeof(uint16_t), 16);
        if (const int e = shg::launch(vec ? k_ring_flatten<true> : k_ring_flatten<false>, grid, dim3(kThreads), 0, st, a, "k_ring_flatten"))
            return e;
    }
    return 0;
}
