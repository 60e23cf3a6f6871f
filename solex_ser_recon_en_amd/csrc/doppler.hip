// The Dopplergram: where the line core sits in every (slit row, frame) of a scan, and that raw map taken to the products'
// geometry.  Not a reference stage (the reference has no velocity map): the arithmetic is the one include/shg_hip.h states and
// tests/doppler_ref.py restates in NumPy, bit for bit.
//
// k_line_core_rot (rotated files, the usual layout): the samples of one wavelength column are one contiguous raw row across the
// slit, so a lane owns eight consecutive raw columns (eight slit rows), loads them as ONE 16-byte piece (8 bytes for 8-bit files)
// per raw row, and a wave's 64 lanes read 1 KiB of the row at once.  The wave walks the band [min lo, max hi] of its 512 slit rows
// row by row (wave-uniform j: every load instruction covers one contiguous stretch), eight rows in flight; a lane skips the rows
// outside its own eight windows.  Each slit row keeps a streaming state (minimum, its position, the samples either side), so
// nothing but the band is read, once.  A workgroup (eight waves, two frames each) does 16 frames of the same 512 rows and writes
// the map through LDS: 16 consecutive columns (64 bytes) of a row at a time instead of one scattered float per row and frame.
// Measured (rocprofv3, MI355X, H = 5): 37.8 us at C2 (2000 x 2000x200, 16-bit: 0.56 of 8 TB/s on the band's bytes), 88.8 us at C5's
// frame shape (0.75); four waves of four frames each gave 43.1 / 96.3 us (too few waves in flight at C2: 2000 for 1024 SIMDs).
// k_line_core_plain (un-rotated files): a wave is one slit row of 64 frames, the window wave-uniform, the stores coalesced.
// k_doppler_finish: the ellipse -> circle resample of k_warp_rows with NaN for taps outside, the limb mask, the crop / pad of
// crop_plan, and the 16-bit display plane; one thread per output pixel.
#include "shg_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kMaxHalfWidth = 32;
constexpr int kRowsPerLane = 8;
constexpr int kTileRows = 64 * kRowsPerLane;   // slit rows of a workgroup
constexpr int kWaves = 8;
constexpr int kTileFrames = 16;                // frames of a workgroup: two a wave
constexpr int kInFlight = 8;                   // raw rows a lane has loads in flight for

struct LineCoreArgs {
    const void* stack;
    int n;
    int64_t height, width, fstride;            // file layout
    const double* fit;                         // [ih][4]
    int hw;
    float* map;
    int64_t pitch, n_cols, k_offset;
    int flip_x;
};

// Window of a slit row: lo > hi when the row has none (then its shift is NaN).
__device__ __forceinline__ void window_of(double f0, int hw, int iw, int& lo, int& hi) {
    lo = 1;
    hi = 0;
    if (!isfinite(f0)) return;
    const int c = (int)fmin(fmax(f0, -0x1p+30), 0x1p+30);     // truncation toward zero, as astype(int) (a5); beyond 2^30 no window survives
    const int l = max(c - hw, 1), h = min(c + hw, iw - 2);
    if (h - l < 2) return;
    lo = l;
    hi = h;
}

// The streaming arg-minimum of one slit row: the first minimum of p over [lo, hi] and the samples either side of it.
struct Core {
    int best, jb, a, e, prev;
};

__device__ __forceinline__ void core_init(Core& s) {
    s.best = INT_MAX;
    s.jb = -2;
    s.a = s.e = s.prev = 0;
}

__device__ __forceinline__ void core_step(Core& s, int j, int p, int lo, int hi) {
    if (j == s.jb + 1) s.e = p;
    if (j >= lo && j <= hi && p < s.best) {
        s.best = p;
        s.jb = j;
        s.a = s.prev;
    }
    s.prev = p;
}

// d = (float)(((double)j* + delta) - fit[y, 3]), NaN unless lo < j* < hi.  a > b strictly (first occurrence) and e >= b, so the
// denominator is positive; every integer is exact in float64 and the quotient is one IEEE division.
__device__ __forceinline__ float core_shift(const Core& s, int lo, int hi, double f3) {
    if (!(s.jb > lo && s.jb < hi)) return __builtin_nanf("");
    const double delta = (double)(s.a - s.e) / (double)(2 * (s.a + s.e - 2 * s.best));
    return (float)(((double)s.jb + delta) - f3);
}

// eight samples of one raw row, as four dwords of u16 pairs (sample r in the (r & 1) half of dword r >> 1)
struct Row8 {
    uint32_t w[4];
};

template <typename T, bool VEC>
__device__ __forceinline__ Row8 load_row8(const char* frame, uint32_t off, int64_t x0, int64_t width) {
    Row8 v;
    if (VEC) {
        if (sizeof(T) == 2) {
            const uint4 q = *reinterpret_cast<const uint4*>(frame + off);
            v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
        } else {
            const uint2 q = *reinterpret_cast<const uint2*>(frame + off);
            v.w[0] = (q.x & 0xffu) | ((q.x << 8) & 0xff0000u);
            v.w[1] = ((q.x >> 16) & 0xffu) | ((q.x >> 8) & 0xff0000u);
            v.w[2] = (q.y & 0xffu) | ((q.y << 8) & 0xff0000u);
            v.w[3] = ((q.y >> 16) & 0xffu) | ((q.y >> 8) & 0xff0000u);
        }
    } else {
        const T* p = reinterpret_cast<const T*>(frame + off);
        uint32_t s[kRowsPerLane];
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) s[r] = x0 + r < width ? (uint32_t)p[r] : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) v.w[i] = s[2 * i] | (s[2 * i + 1] << 16);
    }
    return v;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kWaves) void k_line_core_rot(const LineCoreArgs a) {
    __shared__ float tile[kTileRows][kTileFrames + 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t width = a.width;                                   // = ih
    const int iw = (int)a.height, hw = a.hw;
    const int64_t x0 = (int64_t)blockIdx.x * kTileRows + lane * kRowsPerLane;     // the lane's first raw column
    constexpr int scale = sizeof(T) == 1 ? 256 : 1;                  // video_reader.py:121-122
    int lo[kRowsPerLane], hi[kRowsPerLane];
    double f3[kRowsPerLane];
    int llo = INT_MAX, lhi = INT_MIN;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
        const int64_t x = x0 + r;
        const bool ok = x < width;
        const int64_t y = width - 1 - x;                            // a1: out[i, j] = raw[j, W - 1 - i]
        window_of(ok ? a.fit[y * 4] : (double)NAN, hw, iw, lo[r], hi[r]);
        f3[r] = ok ? a.fit[y * 4 + 3] : 0.0;
        if (lo[r] <= hi[r]) {
            llo = min(llo, lo[r]);
            lhi = max(lhi, hi[r]);
        }
    }
    int wlo = llo, whi = lhi;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        wlo = min(wlo, __shfl_xor(wlo, d));
        whi = max(whi, __shfl_xor(whi, d));
    }
    wlo = __builtin_amdgcn_readfirstlane(wlo);
    whi = __builtin_amdgcn_readfirstlane(whi);
    const uint32_t rowb = (uint32_t)(width * (int64_t)sizeof(T));   // (the entry point checks a frame's bytes < 4 GiB)
    const uint32_t colb = (uint32_t)(x0 * (int64_t)sizeof(T));
    for (int i = 0; i < kTileFrames / kWaves; ++i) {
        const int f = wave + kWaves * i;
        const int64_t k = (int64_t)blockIdx.y * kTileFrames + f;
        if (k >= a.n) break;
        const char* frame = static_cast<const char*>(a.stack) + k * a.fstride * (int64_t)sizeof(T);
        Core s[kRowsPerLane];
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) core_init(s[r]);
        for (int j0 = wlo; j0 <= whi; j0 += kInFlight) {
            Row8 v[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const int j = j0 + u;
                if (j <= whi && j >= llo && j <= lhi) {
                    v[u] = load_row8<T, VEC>(frame, (uint32_t)j * rowb + colb, x0, width);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[u].w[q] = 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const int j = j0 + u;
                if (j > lhi) break;
#pragma unroll
                for (int r = 0; r < kRowsPerLane; ++r) {
                    const int p = (int)((v[u].w[r >> 1] >> (16 * (r & 1))) & 0xffffu) * scale;
                    core_step(s[r], j, p, lo[r], hi[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kRowsPerLane; ++r) tile[lane * kRowsPerLane + r][f] = core_shift(s[r], lo[r], hi[r], f3[r]);
    }
    __syncthreads();
    // 16 threads write 16 consecutive columns of one map row
    const int64_t kb = (int64_t)blockIdx.y * kTileFrames;
    for (int idx = threadIdx.x; idx < kTileRows * kTileFrames; idx += 64 * kWaves) {
        const int rl = idx / kTileFrames, f = idx % kTileFrames;
        const int64_t x = (int64_t)blockIdx.x * kTileRows + rl, k = kb + f;
        if (x < width && k < a.n) {
            const int64_t c = a.k_offset + k;
            a.map[(width - 1 - x) * a.pitch + (a.flip_x ? a.n_cols - 1 - c : c)] = tile[rl][f];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kWaves) void k_line_core_plain(const LineCoreArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t y = (int64_t)blockIdx.y * kWaves + (threadIdx.x >> 6);
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    const int64_t ih = a.height;
    if (y >= ih || k >= a.n) return;
    constexpr int scale = sizeof(T) == 1 ? 256 : 1;
    int lo, hi;
    window_of(a.fit[y * 4], a.hw, (int)a.width, lo, hi);
    const T* row = static_cast<const T*>(a.stack) + k * a.fstride + y * a.width;
    Core s;
    core_init(s);
    for (int j = lo; j <= hi; ++j) core_step(s, j, (int)row[j] * scale, lo, hi);
    const int64_t c = a.k_offset + k;
    a.map[y * a.pitch + (a.flip_x ? a.n_cols - 1 - c : c)] = core_shift(s, lo, hi, a.fit[y * 4 + 3]);
}

struct FinishArgs {
    const float* raw;
    int64_t h, w, raw_pitch;
    double h00, h01, h02;
    int64_t out_h, out_w;
    int masked;
    double cx, cy, rad;
    int64_t nw, lo, dx0, n;                    // crop_plan: new[:, dx0:dx0+n] = img[:, lo:lo+n]
    float* map;
    int64_t map_pitch;
    uint16_t* png;
    int64_t png_pitch;
    double png_scale;                          // 32767 / R
};

__global__ __launch_bounds__(256) void k_doppler_finish(const FinishArgs a) {
    const int64_t oc = (int64_t)blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (oc >= a.nw) return;
    float v = __builtin_nanf("");
    const int64_t c = oc - a.dx0 + a.lo;
    if (oc >= a.dx0 && oc < a.dx0 + a.n && r < a.h) {
        const double x = (a.h00 * (double)c + a.h01 * (double)r) + a.h02;
        const double x0 = floor(x), x1 = ceil(x), t = x - x0;
        const float* row = a.raw + r * a.raw_pitch;
        const double w = (double)a.w;
        const double left = x0 >= 0.0 && x0 < w ? (double)row[(int64_t)x0] : (double)NAN;
        const double right = x1 >= 0.0 && x1 < w ? (double)row[(int64_t)x1] : (double)NAN;
        v = (float)((1.0 - t) * left + t * right);
        if (a.masked) {
            const double dx = (double)c - a.cx, dy = (double)r - a.cy;
            if (dx * dx + dy * dy > a.rad * a.rad) v = __builtin_nanf("");
        }
    }
    a.map[r * a.map_pitch + oc] = v;
    if (a.png) {
        uint16_t q = 0;
        if (!isnan(v)) q = (uint16_t)fmin(fmax(rint(32768.0 + (double)v * a.png_scale), 1.0), 65535.0);
        a.png[r * a.png_pitch + oc] = q;
    }
}

}  // namespace

extern "C" int shg_line_core_shift(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                                   int64_t frame_stride_px, const double* fit, int half_width, int flip_x, float* map,
                                   int64_t row_pitch, int64_t n_cols, int64_t k_offset, shg_stream_t stream) {
    SHG_REQUIRE(stack && fit && map, SHG_E_ARG, "shg_line_core_shift: null pointer");
    SHG_REQUIRE(n_frames > 0 && height > 0 && width > 0, SHG_E_ARG, "shg_line_core_shift: empty input");
    SHG_REQUIRE(bytes_per_px == 1 || bytes_per_px == 2, SHG_E_ARG, "shg_line_core_shift: bytes_per_px must be 1 or 2");
    SHG_REQUIRE(half_width >= 1 && half_width <= kMaxHalfWidth, SHG_E_UNSUPPORTED, "shg_line_core_shift: half-width %d outside [1, %d]",
                half_width, kMaxHalfWidth);
    SHG_REQUIRE(n_frames < (1ll << 31) && n_cols < (1ll << 31), SHG_E_UNSUPPORTED, "shg_line_core_shift: %lld frames / %lld columns",
                (long long)n_frames, (long long)n_cols);
    SHG_REQUIRE(n_cols >= n_frames && k_offset >= 0 && k_offset + n_frames <= n_cols, SHG_E_ARG,
                "shg_line_core_shift: frames [%lld, %lld) do not fit %lld columns", (long long)k_offset, (long long)(k_offset + n_frames),
                (long long)n_cols);
    SHG_REQUIRE(row_pitch >= n_cols, SHG_E_ARG, "shg_line_core_shift: row_pitch < n_cols");
    SHG_REQUIRE(frame_stride_px == 0 || frame_stride_px >= height * width, SHG_E_ARG, "shg_line_core_shift: frame stride smaller than a frame");
    // (the rotated kernel addresses a sample as `frame base + 32-bit byte offset`, its spectral rows as int)
    SHG_REQUIRE(height * width * bytes_per_px < (1ll << 32) && height < (1ll << 31) && width < (1ll << 31), SHG_E_UNSUPPORTED,
                "shg_line_core_shift: a frame of %lld x %lld samples is larger than 4 GiB", (long long)height, (long long)width);
    const int64_t fstride = frame_stride_px > 0 ? frame_stride_px : height * width;
    const bool rot = width > height;
    const int64_t ih = rot ? width : height;
    LineCoreArgs a{stack, (int)n_frames, height, width, fstride, fit, half_width, map, row_pitch, n_cols, k_offset, flip_x ? 1 : 0};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("line_core_shift", st);
    if (rot) {
        // 16-byte pieces (8 for 8-bit samples) when every row of every frame starts on that boundary
        const int64_t piece = kRowsPerLane * bytes_per_px;
        const bool vec = (reinterpret_cast<uintptr_t>(stack) % piece) == 0 && (width * bytes_per_px) % piece == 0 &&
                         (fstride * bytes_per_px) % piece == 0;
        const dim3 grid((unsigned)((ih + kTileRows - 1) / kTileRows), (unsigned)((n_frames + kTileFrames - 1) / kTileFrames));
        if (bytes_per_px == 2)
            return vec ? shg::launch(k_line_core_rot<uint16_t, true>, grid, dim3(64 * kWaves), 0, st, a, "k_line_core_rot")
                       : shg::launch(k_line_core_rot<uint16_t, false>, grid, dim3(64 * kWaves), 0, st, a, "k_line_core_rot");
        return vec ? shg::launch(k_line_core_rot<uint8_t, true>, grid, dim3(64 * kWaves), 0, st, a, "k_line_core_rot")
                   : shg::launch(k_line_core_rot<uint8_t, false>, grid, dim3(64 * kWaves), 0, st, a, "k_line_core_rot");
    }
    const dim3 grid((unsigned)((n_frames + 63) / 64), (unsigned)((ih + kWaves - 1) / kWaves));
    if (bytes_per_px == 2) return shg::launch(k_line_core_plain<uint16_t>, grid, dim3(64 * kWaves), 0, st, a, "k_line_core_plain");
    return shg::launch(k_line_core_plain<uint8_t>, grid, dim3(64 * kWaves), 0, st, a, "k_line_core_plain");
}

extern "C" int shg_doppler_finish(const float* raw, int64_t h, int64_t w, int64_t raw_pitch, double h00, double h01, double h02,
                                  int64_t out_h, int64_t out_w, const double* circle3, const int64_t* crop4, float* map,
                                  int64_t map_pitch, uint16_t* png, int64_t png_pitch, double display_range, shg_stream_t stream) {
    SHG_REQUIRE(raw && map, SHG_E_ARG, "shg_doppler_finish: null pointer");
    SHG_REQUIRE(h > 0 && w > 0 && raw_pitch >= w && out_h > 0 && out_w > 0, SHG_E_ARG, "shg_doppler_finish: empty or mis-pitched input");
    SHG_REQUIRE(out_h < (1ll << 31), SHG_E_UNSUPPORTED, "shg_doppler_finish: %lld output rows", (long long)out_h);
    int64_t nw = out_w, lo = 0, dx0 = 0, n = out_w;
    if (crop4) {
        nw = crop4[0];
        lo = crop4[1];
        dx0 = crop4[2];
        n = crop4[3];
        SHG_REQUIRE(nw > 0 && lo >= 0 && dx0 >= 0 && n >= 0 && dx0 + n <= nw && lo + n <= out_w, SHG_E_ARG,
                    "shg_doppler_finish: crop (%lld, %lld, %lld, %lld) does not fit %lld columns", (long long)nw, (long long)lo,
                    (long long)dx0, (long long)n, (long long)out_w);
    }
    SHG_REQUIRE(map_pitch >= nw && (!png || png_pitch >= nw), SHG_E_ARG, "shg_doppler_finish: output pitch < %lld", (long long)nw);
    SHG_REQUIRE(!png || (isfinite(display_range) && display_range > 0.0), SHG_E_ARG, "shg_doppler_finish: display range must be positive");
    const bool masked = circle3 && !(circle3[0] == -1.0 && circle3[1] == -1.0 && circle3[2] == -1.0);
    FinishArgs a{raw, h, w, raw_pitch, h00, h01, h02, out_h, out_w, masked ? 1 : 0, masked ? circle3[0] : 0.0, masked ? circle3[1] : 0.0,
                 masked ? circle3[2] : 0.0, nw, lo, dx0, n, map, map_pitch, png, png_pitch, png ? 32767.0 / display_range : 0.0};
    hipStream_t st = shg::as_stream(stream);
    SHG_PROF("doppler_finish", st);
    return shg::launch(k_doppler_finish, dim3((unsigned)((nw + 255) / 256), (unsigned)out_h), dim3(256), 0, st, a, "k_doppler_finish");
}
