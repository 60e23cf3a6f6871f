/*
 * shg_hip.h -- C ABI of libshg_hip.so, the MI355X (gfx950) implementation of the
 * SHG reconstruction hot path of thelondonsmiths/Solex_ser_recon_EN.
 *
 * The reference is pure Python and has no FFI; the seam is its set of Python
 * functions.  Each entry point below replaces the NumPy /
 * OpenCV / scikit-image call sites named in its comment (reference file:line).
 * The only consumer is a ctypes binding (solex_ser_recon_en_amd/_lib.py); the
 * binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name starts with host_;
 *  - the caller owns every image, workspace and staging buffer: the kernel entry points, the stage composites and
 *    shg_scan_file allocate nothing on the device and keep nothing between calls;
 *  - `stream` is a hipStream_t (0 = default stream); all calls are asynchronous
 *    with respect to that stream and re-entrant (any number of threads, each with
 *    its own stream and buffers);
 *  - process-global state, all of it: (1) the per-thread error string; (2) the frame-pass lane of each device
 *    (shg_frame_pass_lane_set: one stream handle per device, set once) and an event per (thread, device) that
 *    uses it from a stream with work pending; (3) the registry of passes launched ahead of their scans (shg_pass_a_prelaunch: workspace address ->
 *    launch plan + event, an entry lives from the prelaunch to the scan's first stage or shg_pass_a_forget); (4) every
 *    shg_pool: its threads, its queue and job map; (5) function-local
 *    one-time settings of kernel attributes (dynamic LDS sizes) and cached environment knobs (SHG_*); (6) the BLAS /
 *    LAPACK entry points and callbacks the host control plane was given (shg_host_set_*);
 *  - return value: 0 = OK, >0 = hipError_t, <0 = SHG_E_* argument error; the
 *    message is available per thread from shg_last_error_string();
 *  - "file layout" = the SER frame as stored: [Height][Width], little-endian,
 *    1 or 2 bytes per pixel.  When Width > Height the reference rotates every
 *    frame (video_reader.py:119-120): img[y][x] = raw[x][Width-1-y], ih = Width,
 *    iw = Height.  The kernels never materialise that rotation for the stack.
 */
#ifndef SHG_HIP_H
#define SHG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHG_ABI_VERSION 16

#define SHG_E_ARG        (-1)   /* bad argument (null pointer, non-positive size, ...) */
#define SHG_E_WORKSPACE  (-2)   /* workspace too small                                 */
#define SHG_E_UNSUPPORTED (-3)  /* size outside what the kernel supports               */
/* host control plane: the failure the reference's NumPy / SciPy call would raise at that point */
#define SHG_E_VALUE      (-4)   /* ValueError                                          */
#define SHG_E_TYPE       (-5)   /* TypeError                                           */
#define SHG_E_LINALG     (-6)   /* numpy.linalg.LinAlgError                            */
#define SHG_E_RUNTIME    (-7)   /* RuntimeError                                        */
#define SHG_E_QHULL      (-8)   /* scipy.spatial.QhullError                            */
#define SHG_E_ASSERT     (-9)   /* AssertionError (rescale_brightness's assert)        */
#define SHG_E_INDEX      (-10)  /* IndexError                                          */

typedef void* shg_stream_t;

int         shg_abi_version(void);
const char* shg_last_error_string(void);

/* Optional per-kernel timing (bench.py roofline leg): HIP events recorded on the launch stream
 * directly around each kernel launch, keyed by kernel tag ("accumulate", "reduce_partials",
 * "extract", "warp", "rowpair_stats", "scale_rows", "clahe_hist", "clahe_lut", "clahe_interp",
 * "hist", "rescale", ...); the two frame passes ("accumulate", "extract") have theirs bound to the kernel's
 * own dispatch as its start and stop events instead, which queues nothing between two kernels.
 * Off by default.  shg_profile_get waits for the events of `tag`. */
int shg_profile_enable(int on);
int shg_profile_select(const char* tags_csv);   /* only time these tags (NULL or "" = all) */
int shg_profile_reset(void);
int shg_profile_get(const char* tag, double* total_ms, int64_t* launches);
int shg_profile_total(double* total_ms, int64_t* launches);   /* every timed entry point since the last reset */
/* Where a scan worker's HOST time goes inside the stage composites (waiting in stream synchronises, control-plane routines):
 * wall clock per section tag while enabled; the report is "tag seconds calls" lines.  Measurement aid (tools/host_budget.py). */
int shg_host_timing_enable(int on);
int shg_host_timing_report(char* buf, size_t cap);
int shg_profile_dump(const char* path);   /* "tag,stream,start_ms,stop_ms" per sample: the streams' timeline without a profiler */

/* Measurement aid: trivial read-only kernels over `bytes` bytes (16 B/lane non-temporal loads, XOR-folded;
 * out1024: 1024 uint32 words) that bench.py times to quote MEASURED read ceilings beside the spec peak
 * (SURVEY.md section 8d).  mode 0: grid-strided contiguous sweep with `blocks` workgroups; mode 1: the same with
 * pass A's arithmetic; mode 2: pass A's address pattern for frames of vecs_per_frame 16-byte vectors, `blocks`
 * = frame-axis splits.  unroll: 1, 2, 4 or 8 loads in flight per lane. */
int shg_stream_read_probe(const void* buf, int64_t bytes, int mode, int blocks, int unroll,
                          int64_t vecs_per_frame, uint32_t* out1024, shg_stream_t stream);

/* ---- pass A: sum and max over frames -------- solex_util.py:174-188 (compute_mean_max)
 * stack: n_frames frames in file layout.  sum_out[H*W] (file layout) receives the
 * integer sum of the raw samples, max_out[H*W] their maximum (raw sample units;
 * the 8-bit x256 scaling of video_reader.py:121-122 is applied in
 * shg_finalize_mean_max).  Integer sums are order independent, so the result is
 * bit-identical for any sharding of the frames (RCCL SUM / MAX all-reduce). */
size_t shg_accumulate_workspace_bytes(int64_t n_frames, int64_t height, int64_t width, int bytes_per_px);
int shg_accumulate_sum_max(const void* stack, int64_t n_frames, int64_t height, int64_t width,
                           int bytes_per_px, int64_t frame_stride_px, uint64_t* sum_out, uint16_t* max_out,
                           void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* ---- decode: frames into HBM ---------------------- video_reader.py:94-123
 * The stack may keep a padded frame pitch: frame k starts frame_stride_px samples after frame k-1
 * (0 = dense, height*width).  shg_frame_pitch_bytes gives the pitch the frame-walking kernels read fastest
 * (the frame size rounded up to 8 KiB); shg_upload_frames copies n_frames dense frames from PINNED host
 * memory into such a stack with one asynchronous 2-D hipMemcpy on `stream`. */
int64_t shg_frame_pitch_bytes(int64_t frame_bytes);
int shg_upload_frames(void* dst, int64_t dst_pitch_bytes, const void* host_src, int64_t frame_bytes,
                      int64_t n_frames, shg_stream_t stream);

/* Uncompressed AVI frames (cv2.VideoCapture + COLOR_BGR2GRAY, video_reader.py:68-80, 111-113) into the
 * uint8 stack: raw holds n_frames chunk payloads raw_pitch_bytes apart, each `height` rows of row_bytes
 * (bottom_up: last row first); bits 8 (optional 256-entry grey table for palettised frames, NULL =
 * identity) or 24 (B, G, R; OpenCV 4's (B*3735 + G*19235 + R*9798 + 2^14) >> 15).  At most 65535
 * frames per call. */
int shg_unpack_dib_frames(const uint8_t* raw, int64_t n_frames, int64_t raw_pitch_bytes, int64_t height,
                          int64_t width, int bits, int64_t row_bytes, int bottom_up,
                          const uint8_t* gray_lut, uint8_t* stack, int64_t frame_stride_px,
                          shg_stream_t stream);

/* mean = trunc(sum / n_total) as uint16 (solex_util.py:188), 8-bit samples scaled by
 * 256, both images rotated into the reference's [ih][iw] orientation. */
int shg_finalize_mean_max(const uint64_t* sum, const uint16_t* max_raw, int64_t n_total,
                          int64_t height, int64_t width, int bytes_per_px,
                          uint16_t* mean_out, uint16_t* max_out, shg_stream_t stream);
/* The frame statistics of a frame-sharded scan after their exchange (the reference has no such step: its compute_mean_max,
 * solex_util.py:174-188, sees every frame): n_pieces records of piece_words 32-bit words, one per rank, each
 * [npix partial sums as 32-bit words | npix partial maxima as 16-bit words, padded to a whole word | ...] -- what ONE all-gather of
 * every rank's packed statistics brings (dist.exchange_frame_stats) -- folded into the 64-bit sums and the maxima
 * shg_finalize_mean_max takes.  Integer: the result does not depend on the number of pieces. */
int shg_reduce_frame_stats(const uint32_t* pieces, int n_pieces, int64_t piece_words, int64_t npix, uint64_t* sum_out,
                           uint16_t* max_out, shg_stream_t stream);
/* compute_mean_max (solex_util.py:174-188) for a scan that is whole on this GPU: pass A, then mean and max images straight
 * from its per-slab partials (shg_accumulate_sum_max + shg_finalize_mean_max without the 64-bit totals in between).
 * workspace: shg_accumulate_workspace_bytes. */
int shg_accumulate_mean_max(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                            int64_t frame_stride_px, uint16_t* mean_out, uint16_t* max_out, void* workspace,
                            size_t workspace_bytes, shg_stream_t stream);

/* ---- cv2.blur(img_u16, (kw, kh)) ------------- solex_util.py:166, 230
 * Normalised box filter, anchor (kw/2, kh/2), BORDER_REFLECT_101, round half even.
 * tmp: uint32 scratch of h*w elements. */
int shg_box_blur_u16(const uint16_t* src, int64_t h, int64_t w, int kw, int kh,
                     uint16_t* dst, uint32_t* tmp, shg_stream_t stream);

/* first-occurrence argmin over columns [x0, x1) of every row: np.argmin(img[:, x0:x1], axis=1)
 * (solex_util.py:231, 242).  out[h] int32, relative to x0. */
int shg_row_argmin_u16(const uint16_t* img, int64_t h, int64_t w, int64_t x0, int64_t x1,
                       int32_t* out, shg_stream_t stream);

/* np.mean(img, axis=1) in float64 (solex_util.py:167). out[h]. */
int shg_row_mean_u16(const uint16_t* img, int64_t h, int64_t w, double* out, shg_stream_t stream);

/* ---- the spectral analyser's auto-dispersion loop ----- spectralAnalyserUI.py:271-300 (not on the SHG path)
 * For each guess g (one workgroup each), s = scales[g], the atlas point k at x[k] = ((first + k * step_d) - anchor_wavelength)
 * / s + anchor_x (NumPy's arange of :61 gives first + k * step_d exactly, step_d = (first + step) - first); the run of points
 * with 0 <= x < w (select, :41-48) interpolated at pixels 0 .. w-1 by np.interp's rules from atlas_y[k] / 255 (:280);
 * u[fill_lo:fill_hi] = np.mean(u) (:284, NumPy's pairwise sum: the rows are NumPy's to the bit); corr[g] =
 * np.corrcoef(u, log_spectrum)[0, 1] (:289) within 1e-12.  log_spectrum[w] is float32 np.log(spectrum2) with its own window
 * already filled (:286-287, the caller's).  run[g][2] (may be NULL) = the run's first and last point, first > last (and
 * corr[g] NaN) when the run is empty.  row_of_guess[n_guesses] (NULL when n_rows = 0): the slot of rows[n_rows][w] that
 * receives guess g's filled u, -1 for none.  2 <= w <= 8192, else SHG_E_ARG / SHG_E_UNSUPPORTED.  Every scale must be finite
 * and positive (not checked: the run search assumes x rises with k; another scale gives a run with no meaning, and a negative one
 * walks the whole atlas per thread). */
int shg_atlas_correlate(const uint8_t* atlas_y, int64_t n_atlas, double first, double step_d, double anchor_wavelength,
                        double anchor_x, const float* log_spectrum, int64_t w, int64_t fill_lo, int64_t fill_hi,
                        const double* scales, int64_t n_guesses, double* corr, int32_t* run, const int32_t* row_of_guess,
                        int64_t n_rows, double* rows, shg_stream_t stream);

/* ---- the Dopplergram (not a reference stage; tests/linemaps_ref.py restates both calls in NumPy, bit for bit)
 * shg_line_core_shift: the line-core position of every (slit row y, frame k) of a frame stack in file layout (n_frames, height,
 * width, bytes_per_px, frame_stride_px as shg_extract_columns takes them).  p(j) = sample (y, j) of frame k after a1's rotation
 * (out[i, j] = raw[j, W - 1 - i] when width > height), 8-bit samples x 256.  fit[ih][4] float64 (device); c = int(fit[y][0])
 * (truncated, as a5), lo = max(c - H, 1), hi = min(c + H, iw - 2); NaN when fit[y][0] is not finite or hi - lo < 2.  j* = the
 * first j in [lo, hi] with minimal p(j); NaN when j* == lo or j* == hi.  a, b, e = p(j* - 1), p(j*), p(j* + 1);
 * delta = (double)(a - e) / (double)(2 * (a + e - 2 b)); d = (float)(((double)j* + delta) - fit[y][3]).
 * map[y * row_pitch + col(k)] = d, col(k) = k_offset + k, or n_cols - 1 - (k_offset + k) with flip_x (as the disks).
 * 1 <= half_width H <= 32, else SHG_E_UNSUPPORTED; a frame must hold < 4 GiB and n_cols < 2^31 (SHG_E_UNSUPPORTED). */
int shg_line_core_shift(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px, int64_t frame_stride_px,
                        const double* fit, int half_width, int flip_x, float* map, int64_t row_pitch, int64_t n_cols, int64_t k_offset,
                        shg_stream_t stream);

/* shg_doppler_finish: the raw map raw[h][w] (row pitch raw_pitch) in the products' geometry.  For every output pixel (r, c) of the
 * corrected image (out_h x out_w, h00 h01 h02 = mat3 row 0 of ellipse_to_circle._warp_geometry, as shg_warp_rows_u16):
 * x = (h00 c + h01 r) + h02, taps floor(x) and ceil(x) of raw row r, a tap outside [0, w) (or a row r >= h) NaN;
 * v = (float)((1 - t) L + t R) in float64, t = x - floor(x), NaN propagating.  circle3 (host: cx, cy, rad; NULL or (-1, -1, -1): no mask):
 * v = NaN where (c - cx)^2 + (r - cy)^2 > rad^2 (float64).  crop4 (host, NULL: none) = Solex_recon.crop_plan's (nw, lo, dx0, n):
 * map[r][dx0 + i] = v(r, lo + i) for i < n, NaN elsewhere; map is out_h x nw (nw = out_w without a crop), row pitch map_pitch.
 * png (may be NULL, row pitch png_pitch): 0 where v is NaN, else clip(rint(32768 + (double)v * (32767 / display_range)), 1, 65535). */
int shg_doppler_finish(const float* raw, int64_t h, int64_t w, int64_t raw_pitch, double h00, double h01, double h02,
                       int64_t out_h, int64_t out_w, const double* circle3, const int64_t* crop4, float* map, int64_t map_pitch,
                       uint16_t* png, int64_t png_pitch, double display_range, shg_stream_t stream);

/* ---- line-profile maps (not a reference stage; tests/linemaps_ref.py restates both calls in NumPy, bit for bit)
 * shg_line_profile: five planes of every (slit row y, frame k) of a frame stack in shg_line_core_shift's layout and with its p(j),
 * measured around the line shifted by the integer S (`shift`, the -w shift; 0 = the fitted line).  c = (int64)(fit[y][0] + (double)S)
 * (truncated), lo = max(c - H, 1), hi = min(c + H, iw - 2); every plane NaN when fit[y][0] is not finite or hi - lo < 2.
 * ref = fit[y][3] + (double)S.  j* = the first j in [lo, hi] with minimal p(j); a, b, e = p(j* - 1), p(j*), p(j* + 1), den = a + e - 2b;
 * shift, core and width are NaN when j* == lo or j* == hi.  Every integer below is exact in float64, every step one IEEE operation:
 *   shift = (float)(((double)j* + (double)(a - e) / (double)(2 den)) - ref)            (= shg_line_core_shift's at S = 0)
 *   core_d = (double)b - (double)((a - e)^2) / (8.0 (double)den), core = (float)core_d
 *   C2 = p(lo) + p(hi) (integer), half = 0.5 (0.5 (double)C2 + core_d); width NaN unless p(j*) < half;
 *   jl = the largest j in [lo, j*) with p(j) >= half, xl = (double)jl + ((double)p(jl) - half) / (double)(p(jl) - p(jl + 1));
 *   jr = the smallest j in (j*, hi] with p(j) >= half, xr = (double)jr - ((double)p(jr) - half) / (double)(p(jr) - p(jr - 1));
 *   width = (float)(xr - xl), NaN when jl or jr does not exist
 *   n = hi - lo + 1, int64 S0 = n C2 - 2 sum p, S1 = C2 sum j - 2 sum j p over [lo, hi];
 *   cog = (float)((double)S1 / (double)S0 - ref), NaN when S0 <= 0;  ew = (float)((double)S0 / (double)C2), NaN when C2 == 0.
 * planes[q * plane_stride + y * row_pitch + col(k)], q = 0 shift, 1 core, 2 width, 3 cog, 4 ew; col(k) as shg_line_core_shift.
 * 1 <= H <= 32, a frame < 4 GiB, n_cols < 2^31 (else SHG_E_UNSUPPORTED); 3 - iw - H < S < iw - 3 + H (else no line inside the
 * frame has a window: SHG_E_ARG). */
int shg_line_profile(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px, int64_t frame_stride_px,
                     const double* fit, int half_width, int shift, int flip_x, float* planes, int64_t plane_stride, int64_t row_pitch,
                     int64_t n_cols, int64_t k_offset, shg_stream_t stream);

/* shg_line_profile_finish: the five raw planes raw[q][h][w] (plane stride raw_plane_stride, row pitch raw_pitch) in the products'
 * geometry, each plane bit-identical to shg_doppler_finish with png = NULL: maps[q * map_plane_stride + r * map_pitch + c].
 * png (may be NULL; png[q * png_plane_stride + r * png_pitch + c]): 0 where the value v is NaN, else clip(rint(e), 1, 65535) with
 * e = 32768 + (double)v * (32767 / display_range) for shift and cog, (double)v for core, 1 + (double)v * (65534 / (2 H + 1)) for
 * width and ew (H = half_width, 1 <= H <= 32). */
int shg_line_profile_finish(const float* raw, int64_t raw_plane_stride, int64_t h, int64_t w, int64_t raw_pitch, double h00,
                            double h01, double h02, int64_t out_h, int64_t out_w, const double* circle3, const int64_t* crop4,
                            float* maps, int64_t map_plane_stride, int64_t map_pitch, uint16_t* png, int64_t png_plane_stride,
                            int64_t png_pitch, int half_width, double display_range, shg_stream_t stream);

/* ---- line-bisector maps (not a reference stage; tests/linemaps_ref.py restates both calls in NumPy, bit for bit)
 * shg_line_bisector: the line's bisector and chord at K = n_levels depths of every (slit row y, frame k), in shg_line_profile's layout,
 * with its p(j), window [lo, hi] (and SHG_E_ARG for S), ref = fit[y][3] + (double)S, j*, a, b, e, den, core_d and C2.  levels: a host
 * array of K fractions f_i, 1 <= K <= 8, finite, strictly increasing, 0 < f_1 and f_K < 1 (else SHG_E_ARG, nothing written);
 * f = 0 is the core, f = 1 the continuum C2 / 2.  For each level, one IEEE operation a step:
 *   level = ((1.0 - f) * core_d) + (f * (0.5 * (double)C2))
 * (at f = 0.5 this is shg_line_profile's half bit for bit: each half-scaling is exact), and shg_line_profile's width rule with half
 * replaced by level: NaN unless lo < j* < hi and p(j*) < level; jl = the largest j in [lo, j*) with p(j) >= level, jr = the smallest
 * j in (j*, hi] with p(j) >= level (for integer p: p >= ceil(level)); xl, xr interpolated as the width's; NaN when jl or jr does not
 * exist.  bis_i = (float)((0.5 * (xl + xr)) - ref), chord_i = (float)(xr - xl) (= shg_line_profile's width at f = 0.5, bit for bit).
 * planes[q * plane_stride + y * row_pitch + col(k)], q = i for bis_i and K + i for chord_i; col(k) as shg_line_core_shift.  Each
 * level's values depend on that level alone, not on the other levels requested.  Limits and the other codes as shg_line_profile. */
int shg_line_bisector(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px, int64_t frame_stride_px,
                      const double* fit, int half_width, int shift, const double* levels, int n_levels, int flip_x, float* planes,
                      int64_t plane_stride, int64_t row_pitch, int64_t n_cols, int64_t k_offset, shg_stream_t stream);

/* shg_line_bisector_finish: the 2K raw planes raw[q][h][w] of shg_line_bisector (K = n_levels, 1 <= K <= 8, else SHG_E_ARG) in the
 * products' geometry, each plane bit-identical to shg_doppler_finish with png = NULL: maps[q * map_plane_stride + r * map_pitch + c].
 * png (may be NULL): 0 where v is NaN, else clip(rint(e), 1, 65535) with e = 32768 + (double)v * (32767 / display_range) for the
 * bisector planes (q < K) and 1 + (double)v * (65534 / (2 H + 1)) for the chords (H = half_width, 1 <= H <= 32).  Argument checks and
 * SHG_E_UNSUPPORTED limits as shg_line_profile_finish's. */
int shg_line_bisector_finish(const float* raw, int64_t raw_plane_stride, int n_levels, int64_t h, int64_t w, int64_t raw_pitch,
                             double h00, double h01, double h02, int64_t out_h, int64_t out_w, const double* circle3, const int64_t* crop4,
                             float* maps, int64_t map_plane_stride, int64_t map_pitch, uint16_t* png, int64_t png_plane_stride,
                             int64_t png_pitch, int half_width, double display_range, shg_stream_t stream);

/* ---- emission-line maps (not a reference stage; tests/emission_ref.py restates both calls in NumPy, bit for bit)
 * shg_line_emission: five planes of every (slit row y, frame k) for a line seen in EMISSION (prominences off the limb, flares), in
 * shg_line_profile's layout and with its p(j), c, window [lo, hi], ref = fit[y][3] + (double)S, col(k), limits on H and SHG_E_ARG
 * range of S.  j* = the first j in [lo, hi] with MAXIMAL p(j); a, b, e = p(j* - 1), p(j*), p(j* + 1), den = a + e - 2b (at a bracketed
 * first maximum a < b and e <= b: den < 0, never zero).  Every integer below is exact in float64, every step one IEEE operation:
 *   B2 = p(lo) + p(hi) (integer, twice the background);
 *   peak_d = (double)b - (double)((a - e)^2) / (8.0 (double)den), excess_d = peak_d - 0.5 (double)B2.
 * The gate: all five planes are NaN unless lo < j* < hi and excess_d >= min_excess (min_excess finite and >= 0, else SHG_E_ARG and
 * nothing written).  Scattered disk light off the limb carries the absorption line, whose maximum sits on the window's edge; min_excess
 * rejects noise bumps.  Past the gate:
 *   shift = (float)(((double)j* + (double)(a - e) / (double)(2 den)) - ref)
 *   peak = (float)excess_d
 *   half = 0.5 (0.5 (double)B2 + peak_d); width NaN unless p(j*) > half;
 *   jl = the largest j in [lo, j*) with p(j) <= half, xl = (double)jl + (half - (double)p(jl)) / (double)(p(jl + 1) - p(jl));
 *   jr = the smallest j in (j*, hi] with p(j) <= half, xr = (double)jr - (half - (double)p(jr)) / (double)(p(jr - 1) - p(jr));
 *   width = (float)(xr - xl), NaN when jl or jr does not exist
 *   n = hi - lo + 1, int64 S0 = 2 sum p - n B2, S1 = 2 sum j p - B2 sum j over [lo, hi];
 *   cog = (float)((double)S1 / (double)S0 - ref), flux = (float)(0.5 (double)S0); both NaN when S0 <= 0.
 * The bound: p < 2^16, n <= 65 and j < 2^16 (a frame holds < 2^32 samples and iw is its shorter side), so |S0| < 2^24 and |S1| < 2^40,
 * (a - e)^2 < 2^32: every integer is far below 2^53.
 * planes[q * plane_stride + y * row_pitch + col(k)], q = 0 shift, 1 peak, 2 width, 3 cog, 4 flux. */
int shg_line_emission(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px, int64_t frame_stride_px,
                      const double* fit, int half_width, int shift, double min_excess, int flip_x, float* planes, int64_t plane_stride,
                      int64_t row_pitch, int64_t n_cols, int64_t k_offset, shg_stream_t stream);

/* shg_line_emission_finish: shg_line_profile_finish with a ring in place of the circle.  Each plane of every output pixel is
 * bit-identical to shg_doppler_finish on that plane with no circle; then, with ring4 (host: cx, cy, r_in, r_out; NULL: no mask),
 * dx = (double)c - cx, dy = (double)r - cy, d2 = dx * dx + dy * dy (the circle test's float64 steps), v = NaN where
 *   r_in >= 0 and d2 <= r_in * r_in   (the limb pixel itself is masked; a negative r_in: no inner mask, emission on the disk), or
 *   d2 > r_out * r_out                (r_out = +inf keeps everything).
 * SHG_E_ARG for a NaN in ring4, r_out < 0 or r_out < r_in.  crop4, pitches and limits as shg_line_profile_finish.
 * png (may be NULL): 0 where v is NaN, else clip(rint(e), 1, 65535) with e = 32768 + (double)v * (32767 / display_range) for shift and
 * cog, (double)v for peak, 1 + (double)v * (65534 / (2 H + 1)) for width, (double)v / (double)(2 H + 1) for flux. */
int shg_line_emission_finish(const float* raw, int64_t raw_plane_stride, int64_t h, int64_t w, int64_t raw_pitch, double h00,
                             double h01, double h02, int64_t out_h, int64_t out_w, const double* ring4, const int64_t* crop4,
                             float* maps, int64_t map_plane_stride, int64_t map_pitch, uint16_t* png, int64_t png_plane_stride,
                             int64_t png_pitch, int half_width, double display_range, shg_stream_t stream);

/* ---- removing a fitted plane from a finished line map (not a reference stage; tests/detrend_ref.py restates both calls in NumPy,
 * bit for bit).  The plane z = a + b c + g r (c the column, r the row of the map as the finish wrote it) is fitted on the host from
 * ten integer moments; the 3 x 3 normal equations are INTEGRATION.md's.
 * shg_map_plane_moments: pixel (r, c) with v = map[r * pitch + c] is USED iff
 *   v is finite and |v| < 64;
 *   with a circle (circle3, host: cx, cy, rad; NULL or (-1, -1, -1): none), not (c - cx)^2 + (r - cy)^2 > rad^2 -- shg_doppler_finish's
 *   float64 test step for step: dx = (double)c - cx, dy = (double)r - cy, dx * dx + dy * dy against rad * rad;
 *   with prev4 (host: a, b, g, limit; NULL: none), |(double)v - ((a + b * (double)c) + g * (double)r)| <= limit, one IEEE operation a
 *   step, no contraction, the <= inclusive (limit may be +inf).
 * q = (int64)rint((double)v * 4096), ties to even (the product is exact).  Over the used pixels, all exact int64:
 *   moments10 = { N, sum c, sum r, sum c^2, sum c r, sum r^2, sum q, sum q c, sum q r, sum q^2 }
 * moments10 is device memory; the call overwrites it (it does not add to it).  Every accumulated quantity is an integer, so the result
 * does not depend on the order of the additions.  1 <= h, w <= 8192, else SHG_E_UNSUPPORTED.  The bound: |v| < 64 gives |q| <= 2^18
 * (the largest float32 below 64 rounds up to it), c, r < 2^13 and N <= 2^26, so the largest sums are sum q^2 <= 2^36 * 2^26 = 2^62 and
 * |sum q c| < 2^18 * 2^13 * 2^26 = 2^57: every slot stays below 2^63.  SHG_E_ARG for a null map or moments10, pitch < w, a limit that
 * is negative or NaN, or a previous plane that is not finite.  On any error nothing is written. */
int shg_map_plane_moments(const float* map, int64_t h, int64_t w, int64_t pitch, const double* circle3, const double* prev4,
                          int64_t* moments10, shg_stream_t stream);

/* shg_map_detrend: out[r * out_pitch + c] = (float)((double)v - ((a + b * (double)c) + g * (double)r)), v = map[r * pitch + c],
 * plane3 (host) = (a, b, g), one IEEE operation a step: a NaN v gives NaN, an infinite one stays infinite.  out may be map when the
 * pitches are equal (in place).  png (may be NULL, row pitch png_pitch): shg_doppler_finish's display rule on the OUTPUT value o: 0
 * where o is NaN, else clip(rint(32768 + (double)o * (32767 / display_range)), 1, 65535).  Elements between w and a pitch are never
 * touched.  Limits and codes as shg_map_plane_moments; SHG_E_ARG also for a plane3 that is not finite, an output pitch < w, out == map
 * with another pitch, and (with png) a display range that is not positive. */
int shg_map_detrend(const float* map, int64_t h, int64_t w, int64_t pitch, const double* plane3, float* out, int64_t out_pitch,
                    uint16_t* png, int64_t png_pitch, double display_range, shg_stream_t stream);

/* ---- flattening the disk: the median of every one-pixel annulus around the centre, and the division by that profile (not a
 * reference stage; tests/flatten_ref.py restates both calls in NumPy, bit for bit).
 * The ring of a pixel.  circle3 (host) = (cx, cy, rad).  For the pixel in row r, column c: dx = (double)c - cx, dy = (double)r - cy,
 * d2 = dx * dx + dy * dy -- the circle test's float64 steps, one IEEE operation each, no contraction.  The pixel is ON THE DISK iff
 * not d2 > rad * rad (the test of shg_doppler_finish and shg_map_plane_moments).  Its RING is the largest integer k with
 * (double)k * (double)k <= d2: no square root is part of the definition.  There are K = floor(rad) + 1 rings, and the ring of a pixel
 * on the disk is < K.
 * shg_ring_medians_u16: with n the number of pixels of the image that are on the disk and in ring k, for every k < n_rings
 *   count[k] = n, lo[k] = the (n - 1) / 2-th smallest of their values, hi[k] = the n / 2-th smallest (0-based, integer division: the
 *   median is (lo + hi) / 2); lo[k] = hi[k] = 0 when n = 0.
 * count, lo and hi are device memory of n_rings elements; the call overwrites them.  Everything accumulated is an integer count, so
 * the result depends neither on the launch grid nor on the order of any atomic.  workspace: shg_ring_medians_u16_workspace_bytes
 * (n_rings), which is 0 for n_rings outside [1, 16384] and needs no GPU.  1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG for a
 * null pointer, pitch < w, a circle that is not finite, rad < 0, rad >= 16384, |cx| or |cy| >= 65536, n_rings != floor(rad) + 1, or a
 * workspace that is too small.  On any error nothing is written.  The call neither waits for the device nor copies from it. */
size_t shg_ring_medians_u16_workspace_bytes(int64_t n_rings);
int shg_ring_medians_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, int64_t n_rings,
                         uint32_t* count, uint16_t* lo, uint16_t* hi, void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* shg_ring_flatten_u16: gain (host) = K = n_rings doubles, gain[k] standing for the radius k + 1/2.  Off the disk
 * out[r * out_pitch + c] = v = img[r * pitch + c].  On the disk, one IEEE float64 operation a step:
 *   rho = sqrt(d2), correctly rounded;  u = rho - 0.5;
 *   g = gain[0] if u <= 0;  g = gain[K - 1] if u >= (double)(K - 1);
 *   else j = (int64)u (truncation), t = u - (double)j, g = gain[j] + (gain[j + 1] - gain[j]) * t;
 *   out = (uint16)clip(rint((double)v * g), 0, 65535), rint to nearest, ties to even.
 * out may be img when the pitches are equal (in place).  Elements between w and a pitch are never touched.  Limits and codes as
 * shg_ring_medians_u16; SHG_E_ARG also for a gain that is negative or not finite, an output pitch < w, and out == img with another
 * pitch. */
int shg_ring_flatten_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, const double* gain,
                         int64_t n_rings, uint16_t* out, int64_t out_pitch, shg_stream_t stream);

/* ---- stacking a series of scans: the resample-and-combine of N registered disks in one launch, and the exact sum of squared
 * differences over a window of integer offsets that refines a registration (not reference stages; tests/stack_ref.py restates both
 * calls in NumPy, bit for bit).
 * shg_stack_combine_u16.  host_srcs (host): n device pointers to uint16 images; host_dims3 (host) = [n][3] int64 (h_j, w_j, pitch_j);
 * host_xform4 (host) = [n][4] doubles (s_j, tx_j, ty_j, gain_j): the similarity transform from the output grid into source j and
 * the factor on its values.  Everything is float64, one IEEE operation a step, no contraction.  For the output pixel in row r,
 * column c and source j, in source order:
 *   sx = tx + s * (double)c;  sy = ty + s * (double)r;
 *   the sample is PRESENT iff sx >= 0 && sx <= (double)(w - 1) && sy >= 0 && sy <= (double)(h - 1);
 *   x0 = (int64)sx (truncation), x1 = min(x0 + 1, w - 1), fx = sx - (double)x0;  y0, y1, fy the same from sy and h;
 *   with a = src[y0][x0], b = src[y0][x1], c = src[y1][x0], d = src[y1][x1] as doubles:
 *   top = a + (b - a) * fx;  bot = c + (d - c) * fx;  val = top + (bot - top) * fy;  v_j = val * gain_j.
 * With n' the number of present samples and v the present samples in source order:
 *   n' = 0: out = 0, count = 0.
 *   SHG_STACK_MEAN: m = (((v_0 + v_1) + v_2) + ...) / (double)n';  count = n'.
 *   SHG_STACK_MEDIAN: with the v sorted, m = (v[(n' - 1) / 2] + v[n' / 2]) / 2 (integer division in the ranks);  count = n'.
 *   SHG_STACK_SIGMA: the kappa-sigma clipped mean; count = the number of samples kept.  For n' < 3 it is the mean.  Otherwise the kept
 *     set K is at first every present sample, and up to `iterations` times:
 *       m = (the sum of the kept v, in source order) / (double)|K|;  q = the sum, in source order, of (v - m) * (v - m) over K;
 *       lim = kappa * sqrt(q / (double)|K|), the square root correctly rounded;  K' = the j of K with |v_j - m| <= lim;
 *       K' empty: K stays as it was and the passes end;  K' = K: the passes end;  else K = K', and the passes end when |K| < 3.
 *     m = the in-order mean of K.
 *   out[r * out_pitch + c] = (uint16)clip(rint(m), 0, 65535), rint to nearest, ties to even;  count[r * count_pitch + c] = the count
 *   (count may be NULL).  (A v that overflows to infinity saturates the mean; under SIGMA its deviation is not a number, no sample
 *   is kept, and the rule for an empty K' applies.)
 * Elements between ow and a pitch are never touched.  1 <= n <= 32, else SHG_E_ARG.  1 <= oh, ow, h_j, w_j <= 16384, else
 * SHG_E_UNSUPPORTED.  SHG_E_ARG for a null pointer (count excepted), a pitch below its width, an s that is not finite and > 0, a tx,
 * ty or gain that is not finite, a gain < 0, an unknown mode, a kappa that is NaN or < 1, iterations outside [1, 3] (kappa and
 * iterations are checked whatever the mode), and an output or count plane that overlaps a source or the other.  On any error
 * nothing is written.  The call allocates nothing, waits for nothing and copies nothing from the device. */
#define SHG_STACK_MEAN   0
#define SHG_STACK_MEDIAN 1
#define SHG_STACK_SIGMA  2
int shg_stack_combine_u16(const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4, int n, int mode,
                          double kappa, int iterations, uint16_t* out, int64_t oh, int64_t ow, int64_t out_pitch, uint8_t* count,
                          int64_t count_pitch, shg_stream_t stream);

/* shg_shift_ssd_u16: ref and img are uint16 images of h x w on one grid (pitches ref_pitch, img_pitch).  The pixel set, the same for
 * every offset: every (r, c) with S <= c < w - S and S <= r < h - S that, given a circle3 (host; NULL or (-1, -1, -1): no circle),
 * is ON THE DISK by the test of the flatten section above (not d2 > rad * rad in its float64 steps).  For every integer offset
 * (u, v) with |u|, |v| <= S:
 *   ssd[(v + S) * (2 S + 1) + (u + S)] = the sum over the set of (ref[r][c] - img[r + v][c + u])^2, as uint64;
 *   ssd[(2 S + 1)^2] = the number of pixels in the set.
 * ssd is device memory of (2 S + 1)^2 + 1 uint64; the call overwrites it (its clearing pass is part of the call).  A term is below
 * (2^16)^2 and an image holds at most 2^28 pixels: a sum stays below 2^60 < 2^64.  All sums are integers: the result depends neither
 * on the launch grid nor on the order of any atomic.  0 <= S <= 8, else SHG_E_ARG.  1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.
 * SHG_E_ARG for a null pointer, a pitch < w, and a circle that is not finite (an empty set -- w or h < 2 S + 1, a circle off the
 * image -- is no error: every sum and the count are 0).  On any error nothing is written. */
int shg_shift_ssd_u16(const uint16_t* ref, int64_t ref_pitch, const uint16_t* img, int64_t img_pitch, int64_t h, int64_t w, int S,
                      const double* circle3, uint64_t* ssd, shg_stream_t stream);

/* ---- local alignment points: one table of sums of squared differences a patch, and the combine that bends each source by a
 * displacement field (not reference stages; tests/align_ref.py restates both calls in NumPy, bit for bit).
 * shg_patch_ssd_u16: ref and img are uint16 images of h x w on one grid (pitches ref_pitch, img_pitch); points (device) = [n][2]
 * int32 (row pr, column pc), the centres, which may lie anywhere, also outside the image.  B is the patch's half-size (the patch is
 * (2 B + 1)^2), S the search.  The pixel set of point p, the same for every offset: every (r, c) with |r - pr| <= B, |c - pc| <= B,
 * S <= c < w - S and S <= r < h - S that, given a circle3 (host; NULL or (-1, -1, -1): no circle), is ON THE DISK by the test of the
 * flatten section above.  With W = (2 S + 1)^2 + 3, out (device) = [n][W] uint64, and for every integer offset (u, v), |u|, |v| <= S:
 *   out[p][(v + S) * (2 S + 1) + (u + S)] = the sum over the set of (ref[r][c] - img[r + v][c + u])^2;
 *   out[p][(2 S + 1)^2] = the number of pixels in the set;  out[p][(2 S + 1)^2 + 1] = the sum of ref[r][c] over the set;
 *   out[p][(2 S + 1)^2 + 2] = the sum of ref[r][c]^2 over the set.
 * A term is below 2^32 and a set holds at most 65^2 = 4225 pixels: every sum stays below 2^45 < 2^64.  All sums are integers and every
 * word of out is written by one plain store: the result depends neither on the launch grid nor on any order, and the call needs no
 * clearing pass.  An empty set gives a row of zeros; two equal points give two equal rows.  1 <= n <= 2^23 = 8 388 608, 1 <= B <= 32,
 * 0 <= S <= 8, else SHG_E_ARG.  1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG for a null pointer, a pitch < w, a circle that
 * is not finite, and an out that overlaps ref, img or points.  On any error nothing is written. */
int shg_patch_ssd_u16(const uint16_t* ref, int64_t ref_pitch, const uint16_t* img, int64_t img_pitch, int64_t h, int64_t w,
                      const int32_t* points, int64_t n, int B, int S, const double* circle3, uint64_t* out, shg_stream_t stream);

/* shg_stack_combine_field_u16: shg_stack_combine_u16 with a displacement field a source.  host_srcs, host_dims3, host_xform4, n, mode,
 * kappa, iterations, out, count and their pitches are that call's.  host_fields (host): n device pointers, each NULL (no field for
 * that source) or a float64 array [gh][gw][2] that starts on 16 bytes: (dx, dy) at the lattice node (j, i), which sits at the output
 * pixel (r, c) = (j * step, i * step).  The lattice is one for all sources and must cover the grid: gh = (oh - 1 + step - 1) / step + 1
 * and gw = (ow - 1 + step - 1) / step + 1 in integer division.  Everything is float64, one IEEE operation a step, no contraction.
 * For the output pixel in row r, column c:
 *   j = r / step (integer division), j1 = min(j + 1, gh - 1), fy = (double)(r - j * step) / (double)step;
 *   i = c / step, i1 = min(i + 1, gw - 1), fx = (double)(c - i * step) / (double)step;
 * and for source s with a field F, per component k = 0 (dx), 1 (dy), with a = F[j][i][k], b = F[j][i1][k], c' = F[j1][i][k],
 * d = F[j1][i1][k]:
 *   top = a + (b - a) * fx;  bot = c' + (d - c') * fx;  d_k = top + (bot - top) * fy;
 *   sx = tx + s * ((double)c + dx);  sy = ty + s * ((double)r + dy);
 * without a field sx = tx + s * (double)c, sy = ty + s * (double)r.  Presence, the bilinear sample, the gain, the three modes, the
 * rounding and the count are then exactly shg_stack_combine_u16's.  A displacement that is not finite makes sx or sy fail the
 * presence test: the sample is absent (so are the samples of every pixel whose cell has such a node, whatever its weight: inf * 0
 * is not a number).  A NULL field and a field of zeros give shg_stack_combine_u16's result bit for bit ((double)c + 0.0 is (double)c).
 * 8 <= step <= 128, else SHG_E_ARG.  SHG_E_ARG also for a null host_fields, a gh or gw other than the above, a field that does not
 * start on 16 bytes, and an output or count plane that overlaps a field; every limit and code of shg_stack_combine_u16 holds.  On
 * any error nothing is written.  The call allocates nothing, waits for nothing and copies nothing from the device. */
int shg_stack_combine_field_u16(const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4,
                                const double* const* host_fields, int64_t gh, int64_t gw, int step, int n, int mode, double kappa,
                                int iterations, uint16_t* out, int64_t oh, int64_t ow, int64_t out_pitch, uint8_t* count,
                                int64_t count_pitch, shg_stream_t stream);

/* ---- ranking scans by sharpness: the sums a quality figure is made of, one row a patch, and the combine that weights each source by
 * a lattice of such figures (not reference stages; tests/quality_ref.py restates both calls in NumPy, bit for bit).
 * shg_patch_sharpness_u16: img is a uint16 image of h x w (pitch in elements); points (device) = [n][2] int32 (row pr, column pc), the
 * centres, which may lie anywhere, also outside the image, as for shg_patch_ssd_u16.  B is the patch's half-size, D the arm of the
 * Laplacian.  The pixel set of point p: every (r, c) with |r - pr| <= B, |c - pc| <= B, D <= r < h - D and D <= c < w - D that, given a
 * circle3 (host; NULL or (-1, -1, -1): no circle), is ON THE DISK by the test of the flatten section above, the test of
 * shg_patch_ssd_u16 in the same float64 steps.  For a pixel of the set, as int64 (the arms may read pixels that are not in the set):
 *   L = 4 * img[r][c] - img[r - D][c] - img[r + D][c] - img[r][c - D] - img[r][c + D].
 * out (device) = [n][4] uint64:
 *   out[p][0] = the number of pixels in the set;  out[p][1] = the sum of img[r][c] over the set;
 *   out[p][2] = the sum of img[r][c]^2 over the set;  out[p][3] = the sum of L^2 over the set.
 * |L| <= 4 * 65535 < 2^18, L^2 < 2^36, and a set holds at most 65^2 = 4225 pixels: every sum stays below 2^49 < 2^64.  All sums are
 * integers and every word of out is written by one plain store: the result depends neither on the launch grid nor on any order, and
 * the call needs no clearing pass.  An empty set (an image narrower or lower than 2 D + 1, a centre far outside, a circle off the
 * patch) gives a row of zeros; two equal points give two equal rows.  1 <= n <= 2^23, 1 <= B <= 32, 1 <= D <= 8, else SHG_E_ARG.
 * 1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG for a null pointer, a pitch < w, a circle that is not finite, and an out that
 * overlaps img or points.  On any error nothing is written. */
int shg_patch_sharpness_u16(const uint16_t* img, int64_t pitch, int64_t h, int64_t w, const int32_t* points, int64_t n, int B, int D,
                            const double* circle3, uint64_t* out, shg_stream_t stream);

/* shg_stack_combine_weighted_u16: shg_stack_combine_field_u16 with a weight lattice a source.  Every argument of that call is that
 * call's, except that host_fields may be NULL as a whole (no source has a field).  host_weights (host): n device pointers, each NULL
 * (weight 1 everywhere) or a float64 array [gh][gw] that starts on 8 bytes: one weight a node of the lattice the fields use (gh, gw
 * and step follow that call's rules also when there is no field).  Everything is float64, one IEEE operation a step, no contraction.
 * With the cell (j, j1, i, i1, fx, fy) of shg_stack_combine_field_u16 for the output pixel, and for source s with a lattice W,
 * a = W[j][i], b = W[j][i1], c' = W[j1][i], d = W[j1][i1]:
 *   top = a + (b - a) * fx;  bot = c' + (d - c') * fx;  w_s = top + (bot - top) * fy;
 * without a lattice w_s = 1.0.  Source s is PRESENT at the pixel iff it is present by shg_stack_combine_field_u16's rule and
 * w_s > 0.0 is true (a weight that is not a number removes the sample).  With v the present samples in source order:
 *   SHG_STACK_MEAN: the kept set K is every present sample.
 *   SHG_STACK_SIGMA: K comes from exactly shg_stack_combine_u16's clipping passes over the present samples, which do not see the
 *     weights (unweighted means and deviations); its rule for n' < 3 and its rule for an empty K' hold.
 *   SHG_STACK_MEDIAN: SHG_E_ARG (there is no weighted median).
 *   num = the sum over K, in source order from 0.0, of w_s * v_s (every product rounded, then every sum);  den = the sum over K, in
 *   source order from 0.0, of w_s;  m = num / den;  out = (uint16)clip(rint(m), 0, 65535), ties to even;  count = |K|.
 *   Nothing present: out = 0, count = 0.
 * Three exact properties follow.  (a) With every lattice NULL, or every node 1.0, the result is shg_stack_combine_field_u16's bit for
 * bit: 1.0 * v is v, and the sum of |K| ones is the exact integer |K|.  (b) A lattice of zeros for source s gives the result of the
 * call without source s, the order of the others kept, bit for bit.  (c) Multiplying every node of every lattice by one power of two
 * changes no bit, as long as the nodes stay in range: every step scales exactly.
 * The nodes are the caller's to keep finite, >= 0 and <= 2^20: the call copies nothing from the device and cannot check them.  A node
 * outside that range makes the pixels of its cells unspecified; nothing outside out and count is ever written whatever the nodes
 * hold.  SHG_E_ARG for a null host_weights, a lattice that does not start on 8 bytes, and an output or count plane that overlaps a
 * weight lattice; every limit and code of shg_stack_combine_field_u16 holds (a null host_fields excepted).  On any error nothing is
 * written.  The call allocates nothing, waits for nothing and copies nothing from the device. */
int shg_stack_combine_weighted_u16(const uint16_t* const* host_srcs, const int64_t* host_dims3, const double* host_xform4,
                                   const double* const* host_fields, const double* const* host_weights, int64_t gh, int64_t gw, int step,
                                   int n, int mode, double kappa, int iterations, uint16_t* out, int64_t oh, int64_t ow, int64_t out_pitch,
                                   uint8_t* count, int64_t count_pitch, shg_stream_t stream);

/* ---- sharpening a disk: the undecimated B3-spline ("a trous") wavelet layers of a 16-bit image, one gain a layer and a soft
 * noise gate a layer (not a reference stage; tests/sharpen_ref.py restates all of it in NumPy, bit for bit).  Everything is an
 * integer: the result depends neither on the launch grid, nor on how levels are fused, nor on the order of anything.
 * The reflection R(i, n), whole-sample symmetric and repeated (NumPy's 'reflect'): 0 when n = 1; else with p = 2 (n - 1),
 *   i <- i mod p (non-negative), and R = i when i < n, p - i otherwise.  An image narrower than twice a hole reflects more than once.
 * The decomposition into 1 <= levels = L <= 6 layers, in Q6 fixed point:
 *   c_0[r][c] = 64 * img[r][c]                                                   (below 2^22);
 *   for j = 1 .. L, with the hole d = 2^(j - 1) and K = (1, 4, 6, 4, 1):
 *     S[r][c] = sum over k, l = 0 .. 4 of K[k] * K[l] * c_(j-1)[R(r + (k - 2) d, h)][R(c + (l - 2) d, w)]
 *               (below 2^30: an image of all 65535 gives 1 073 725 440; exact however it is split into a row and a column pass,
 *               nothing is rounded between the two);
 *     c_j = (S + 128) >> 8;      w_j = c_(j-1) - c_j   (int32, |w_j| < 2^22).
 *   c_0 = w_1 + ... + w_L + c_L exactly.
 * The recombination.  host_gain_q8[j - 1] in [0, 4096] is the gain of layer j, 256 standing for 1; host_threshold_q6[j - 1] in
 * [0, 2^22] is its gate, in the units of w_j (64 a count):
 *   s_j = sign(w_j) * max(|w_j| - threshold_j, 0)                                (the soft threshold; a threshold of 0 is the identity);
 *   acc = 256 * c_L + sum over j of gain_j * s_j                                 (int64, |acc| < 2^37);
 *   out[r * out_pitch + c] = (uint16)clip((acc + 8192) >> 14, 0, 65535)          (the shift is arithmetic: a floor towards -infinity).
 *   Every gain 256 and every threshold 0 give out = img.
 * shg_wavelet_sharpen_u16: planes is NULL or device int32 memory of [L + 1][h][w] (dense): w_1 .. w_L, then c_L.  Without planes no
 *   wavelet plane reaches memory: only what the launches hand each other -- c_3 and its successors and acc, beyond three levels --
 *   goes through the workspace.  workspace: shg_wavelet_workspace_bytes(h, w, levels), which is 0 for arguments out of range and
 *   needs no GPU.
 * shg_wavelet_noise_u16: the pixel set is every pixel ON THE DISK by the test of the flatten section above (circle3 on the host, the
 *   radius already multiplied by the caller's region; NULL or (-1, -1, -1): every pixel).  With n the size of the set,
 *   out2[0] = the lower median of |w_1| over the set -- the (n - 1) / 2-th smallest, 0-based, an exact integer in Q6 --, out2[1] = n;
 *   n = 0 gives 0 and 0.  out2 is device memory of two uint64.  An exact two-level radix select over the 22-bit values (high 11
 *   bits, then low 11 bits) in the manner of shg_ring_medians_u16: integer counts only, and the call includes its own clearing pass.
 *   workspace: at least shg_wavelet_workspace_bytes(h, w, 1) (the query for any level count is enough).
 * 1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG for a null pointer (planes excepted), a pitch below the width, levels outside
 * [1, 6], a gain or threshold out of range, a circle that is not finite, a workspace that is too small, and an out or planes that
 * overlaps img or the other (a stencil cannot run in place).  On any error nothing is written.  No call allocates, waits for the
 * device or copies from it.  Elements between w and a pitch are never touched. */
size_t shg_wavelet_workspace_bytes(int64_t h, int64_t w, int levels);
int shg_wavelet_sharpen_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, int levels, const int32_t* host_gain_q8,
                            const int32_t* host_threshold_q6, uint16_t* out, int64_t out_pitch, int32_t* planes, void* workspace,
                            size_t workspace_bytes, shg_stream_t stream);
int shg_wavelet_noise_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, uint64_t* out2,
                          void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* ---- deconvolving a disk: Richardson-Lucy with a separable point-spread function (not a reference stage; tests/deconvolve_ref.py
 * restates all of it in NumPy, bit for bit).  Every value is a float32 and every product and every sum is rounded on its own (no
 * fused multiply-add, no fast-math); the division is IEEE's, correctly rounded.
 * Inputs: img uint16 [h][w] with a pitch; a radius R, 0 <= R <= 16; 2 R + 1 host float32 taps k[-R .. R] (host_taps[R + i] = k[i]),
 *   each 0 or in [2^-30, 1], their float64 sum within 2^-10 of 1; 1 <= iterations = N <= 200.
 * The blur B(a, k) of a plane a, separable, with the reflection R(i, n) of the sharpening section above (an image narrower than R
 * reflects more than once):
 *   t[r][c] = sum over i = -R .. R, in increasing i, of k[i] * a[r][R(c + i, w)]       (the row pass: the sum starts from 0, and a tap
 *                                                                                      is one rounded multiply and one rounded add);
 *   B[r][c] = sum over i = -R .. R, in increasing i, of k[i] * t[R(r + i, h)][c]       (the column pass, accumulated the same way);
 *   t is a float32 between the passes.
 * The iteration: d = (float)img, e_0 = d; for n = 1 .. N:
 *   1. b = B(e_(n-1), k);
 *   2. q = d / max(b, 2^-10);
 *   3. c = B(q, k~) with k~[i] = k[-i]                     (the adjoint: the taps reversed);
 *   4. p = e_(n-1) * c;
 *   5. e_n = 0 if p < 2^-20, else min(p, 2^20)             (the flush and the clamp).
 * out[r * out_pitch + c] = (uint16)clip(rint(e_N), 0, 65535), ties to even; estimate, if given, receives e_N unrounded, dense [h][w].
 * Four properties follow, and the tests use them:
 *   (a) everything is finite and >= 0: b < 2^21, q <= 65535 * 2^10 < 2^26, c < 2^27 and p <= 2^20 c < 2^47;
 *   (b) no operation has a subnormal result: a non-zero tap is >= 2^-30, a non-zero e >= 2^-20, a non-zero q > 1 / b > 2^-21, so the
 *       smallest non-zero product of a tap and a value is above 2^-51, of a tap and a t above 2^-81, and of e and c above 2^-102: the
 *       result does not depend on the denormal mode;
 *   (c) taps padded with zeros on both sides to a larger R give the same bits: 0 * a = +0 for a finite a >= 0, and adding +0 to a
 *       non-negative sum changes nothing;
 *   (d) every pixel's value is a fixed expression of its inputs: neither the launch grid, nor the tile, nor any fusion of steps
 *       can change a bit.
 * workspace: shg_rl_workspace_bytes(h, w) -- the float planes e and q the launches hand each other, 8 bytes a pixel, plus the
 *   round-up of its start to 256 bytes --, which is 0 for dimensions out of range and needs no GPU.
 * 1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG for a null pointer (estimate excepted), a pitch below the width, a radius
 * or an iteration count out of range, a tap that is not finite or out of range, a sum of taps off 1, a workspace that is too small,
 * and an out, estimate or workspace that overlaps img or one another.  On any error nothing is written.  The call allocates nothing,
 * waits for nothing and copies nothing from the device.  Elements between w and a pitch are never touched. */
size_t shg_rl_workspace_bytes(int64_t h, int64_t w);
int shg_rl_deconvolve_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const float* host_taps, int radius, int iterations,
                          uint16_t* out, int64_t out_pitch, float* estimate, void* workspace, size_t workspace_bytes,
                          shg_stream_t stream);

/* shg_rl_deconvolve_xy_u16: the same iteration with a tap set an axis -- kx[-Rx .. Rx] (host_taps_x) in the row pass, along the
 * columns of a row, and ky[-Ry .. Ry] (host_taps_y) in the column pass: B(a) reads t = row pass with kx, then column pass with ky; the
 * adjoint reverses each set (kx~[i] = kx[-i], ky~[i] = ky[-i]).  Everything else -- the order of the sums, the roundings, steps 1 to 5,
 * out, estimate, the workspace, the properties (a) to (d) -- is as stated above with k replaced per pass, and every limit on radius and
 * taps holds for each axis.  By (c) the shorter set is padded with zeros to the longer one's radius.  Equal sets give the bits of
 * shg_rl_deconvolve_u16.  Codes as there; a null host_taps_y is SHG_E_ARG. */
int shg_rl_deconvolve_xy_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const float* host_taps_x, int radius_x,
                             const float* host_taps_y, int radius_y, int iterations, uint16_t* out, int64_t out_pitch, float* estimate,
                             void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* ---- limb protection for the two filters above: the image split into a disk plane and a sky plane that have no step at the limb, and
 * the filtered planes put back around the untouched limb (not reference stages; tests/limbguard_ref.py restates both calls in NumPy,
 * bit for bit).  Everything is float64, one IEEE operation a step, no contraction; sqrt and / are correctly rounded.
 * circle3 (host) = (cx, cy, rad); E = rad - margin, F = rad + margin.  For the pixel in row r, column c:
 *   dx = (double)c - cx, dy = (double)r - cy, d2 = dx * dx + dy * dy, rho = sqrt(d2);
 *   ux = dx / rho, uy = dy / rho when rho > 0, else ux = 1, uy = 0                       (the pixel's ray);
 *   sample(t) = bilin(cx + ux * t, cy + uy * t)                                           (the image at the distance t on that ray);
 *   bilin(x, y): x clamped to [0, w - 1], y to [0, h - 1]; x0 = (int64)x, x1 = min(x0 + 1, w - 1), fx = x - (double)x0, and y0, y1, fy
 *     likewise; with a = img[y0][x0], b = img[y0][x1], c' = img[y1][x0], d = img[y1][x1] as doubles:
 *     top = a + (b - a) * fx, bot = c' + (d - c') * fx, bilin = top + (bot - top) * fy    (well defined for w = 1 or h = 1);
 *   Q(v) = (uint16)clip(rint(v), 0, 65535), rint to nearest, ties to even.
 * shg_limb_split_u16: one launch, one read of img, two planes; inner or outer may be NULL, not both.
 *   inner[r][c] = img[r][c] where not rho > E; elsewhere, with s = sample(E): Q((s + s) - sample(max((E + E) - rho, E - reach)));
 *   outer[r][c] = img[r][c] where not rho < F; elsewhere, with s = sample(F): Q((s + s) - sample(min((F + F) - rho, F + reach))).
 *   Each plane continues the image across the limb by a POINT REFLECTION about its value at the edge of what it keeps: continuous in
 *   value and in slope along the ray.  Beyond `reach` the continuation holds a plateau along the ray.
 * shg_limb_merge_u16: disk and sky are the filtered inner and outer planes; sky may be NULL.  With o = (double)img[r][c]:
 *   rho < E:                 wt = min((E - rho) / blend, 1), out = Q(o + wt * ((double)disk[r][c] - o));
 *   rho > F and sky given:   wt = min((rho - F) / blend, 1), out = Q(o + wt * ((double)sky[r][c] - o));
 *   otherwise                out = img[r][c].
 *   Two consequences the tests use: the band E <= rho <= F of out is img bit for bit; where wt = 1 (o + (d - o) is exact for two
 *   16-bit values) out is disk, or sky, bit for bit.
 * Every pixel's value is a fixed expression of its inputs: neither the launch grid nor any early-out of the kernels can change a bit.
 * 1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG, with nothing written, for a null pointer it does not allow, a pitch below w,
 * a circle3, margin, reach or blend that is not finite, rad <= 0, rad >= 16384, |cx| or |cy| >= 65536 (the limits of
 * shg_ring_medians_u16: every coordinate of a sample stays finite), margin < 0, E < 1, reach < 1, reach > E, blend <= 0, and an output
 * that overlaps an input or the other output.  The calls allocate nothing, wait for nothing and copy nothing from the device.
 * Elements between w and a pitch are never touched. */
int shg_limb_split_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, double margin, double reach,
                       uint16_t* inner, int64_t inner_pitch, uint16_t* outer, int64_t outer_pitch, shg_stream_t stream);
int shg_limb_merge_u16(const uint16_t* img, int64_t pitch, const uint16_t* disk, int64_t disk_pitch, const uint16_t* sky, int64_t sky_pitch,
                       int64_t h, int64_t w, const double* circle3, double margin, double blend, uint16_t* out, int64_t out_pitch,
                       shg_stream_t stream);

/* ---- measuring the blur from the limb: the edge-spread tables of the annulus around the fitted circle, one row a sector (not a
 * reference stage; tests/psf_ref.py restates the call in NumPy, bit for bit).  Everything is float64, one IEEE operation a step, no
 * contraction; sqrt and / are correctly rounded.  circle3 (host) = (cx, cy, rad); reach, sub and sectors = S are integers;
 * bins = 2 * reach * sub.  For the pixel in row r, column c, with dx, dy and d2 as in shg_ring_medians_u16:
 *   THE BIN.     rho = sqrt(d2);  v = (rho - (rad - (double)reach)) * (double)sub.  The pixel COUNTS iff 0 <= v < (double)bins, and its bin
 *                is b = floor(v): bin b spans the distances t in [b / sub - reach, (b + 1) / sub - reach) from the circle.
 *   THE SECTOR.  No transcendental function is evaluated.  ax = |dx|, ay = |dy|; swap = ay > ax; hi = swap ? ay : ax, lo = swap ? ax : ay
 *                (hi >= rho / sqrt(2) > 0 for a pixel that counts, because reach <= rad - 1);  q = lo / hi, in [0, 1];
 *                i = the number of k with thresholds[k] <= q, over the n - 1 thresholds, n = S / 8  (host doubles, strictly increasing,
 *                inside (0, 1); the caller supplies them, tan((k + 1) * pi / (4 n)) for sectors of equal angle);
 *                o = swap ? 1 : 0, rev = swap;  if dx < 0: o = 3 - o, rev = !rev;  then if dy < 0: o = 7 - o, rev = !rev;
 *                sector = o * n + (rev ? n - 1 - i : i).
 *                o is the octant of the angle theta of (dx, dy), counted from the +column axis towards the +row axis -- clockwise on a
 *                screen whose rows run downwards --, so sector s covers theta in [s, s + 1) * 2 pi / S and its middle is at
 *                (s + 1/2) * 2 pi / S.  The boundaries: dy = 0 belongs to octants 0 and 3, dx = 0 to octants 1 and 6, |dx| = |dy| to
 *                octants 0, 3, 4 and 7 (no swap), and q equal to a threshold to the index above it.
 *   count[s][b] += 1 (uint32), sum[s][b] += img (uint64), sumsq[s][b] += img * img (uint64): exact integers, dense [S][bins] device
 *   tables that the call clears itself; neither the launch grid, nor the order of an atomic, nor any early-out can change a bit.
 * 1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG, with nothing written, for a null pointer (thresholds may be NULL when S = 8),
 * pitch < w, a circle outside the limits of shg_ring_medians_u16, reach outside [1, 64] or above rad - 1, sub outside [1, 8], S not a
 * multiple of 8 from 8 to 64, a threshold that is not finite, not inside (0, 1) or not above the one before it, and a table that
 * overlaps the image or another table.  The call allocates nothing, waits for nothing and copies nothing from the device. */
int shg_limb_profile_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, int reach, int sub, int sectors,
                         const double* thresholds, uint32_t* count, uint64_t* sum, uint64_t* sumsq, shg_stream_t stream);

/* ---- scan jitter along the slit: the two limb crossings of every column of a raw disk, and every column resampled along itself by
 * its own shift (not reference stages; tests/dejitter_ref.py restates both calls in NumPy, bit for bit).  Everything on the device is
 * an integer: the result depends neither on the launch grid, nor on how a column's rows are split, nor on the order of anything.
 * shg_column_limb_u16: img is a uint16 image of h x w (pitch in elements); K = window, odd, 1 <= K <= 15; T = threshold,
 * 0 <= T <= 65535.  For column c, as uint32:
 *   s[i] = sum over k = 0 .. K - 1 of img[i + k][c]   for 0 <= i <= h - K    (below 2^20);      A[i] = (s[i] >= K * T).
 *   THE TOP CROSSING is the smallest i >= 1 with !A[i - 1] && A[i], provided A[0] is false;
 *   THE BOTTOM CROSSING is the largest i <= h - K - 1 with A[i] && !A[i + 1], provided A[h - K] is false.
 *   The column HAS A MEASUREMENT iff h >= K + 2, A[0] and A[h - K] are false and some A[i] is true (both crossings then exist).
 * out6 (device) = [w][6] int32: (i_top, s[i_top - 1], s[i_top], i_bot, s[i_bot], s[i_bot + 1]) for a column with a measurement, -1 in
 * all six otherwise.  Every word is written once, by a plain store: the call needs no clearing pass and accumulates nothing across
 * workgroups.  The sub-pixel crossings are the caller's, in float64, one IEEE operation a step:
 *   top = ((double)(i_top - 1) + (double)(K * T - s[i_top - 1]) / (double)(s[i_top] - s[i_top - 1])) + (double)(K - 1) / 2.0;
 *   bot = ((double)i_bot + (double)(s[i_bot] - K * T) / (double)(s[i_bot] - s[i_bot + 1])) + (double)(K - 1) / 2.0;
 * both denominators are > 0 by construction.  SHG_E_ARG for an even window or one outside [1, 15], a threshold outside [0, 65535]
 * and a table that overlaps the image.
 * shg_column_shift_u16: img is n planes (1 <= n <= 64) of h x w uint16, rows `pitch` and planes `plane_stride` elements apart; out
 * likewise with out_pitch and out_plane_stride.  host_offset (host) = [w] int32, |offset| <= 16384; host_weight4 (host) = [w][4]
 * int32 in Q14, each in [-4096, 20480], the four of a column summing to 16384.  For plane p, row r, column c, as int64:
 *   acc = sum over k = 0 .. 3 of weight[c][k] * img[p][clamp(r + offset[c] + k - 1, 0, h - 1)][c]      (|acc| < 2^31);
 *   out[p][r][c] = (uint16)clip((acc + 8192) >> 14, 0, 65535)            (the shift is arithmetic: a floor towards -infinity).
 *   A column with offset 0 and weights (0, 16384, 0, 0) leaves as it came, bit for bit.
 * The per-column arrays travel to the device by value, in the arguments of the launches (256 columns a launch, every launch for all
 * planes): they are read before the call returns and may be reused at once.  SHG_E_ARG for n outside [1, 64], an offset or a weight
 * out of range, weights of a column that do not sum to 16384, with n > 1 a plane stride below (h - 1) * pitch + w, a plane stride
 * outside [0, 2^40], and an out that overlaps img (a resampling cannot run in place).
 * Both calls: 1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG for a null pointer and a pitch below the width.  On any error
 * nothing is written.  The calls allocate nothing, wait for nothing and copy nothing from the device.  Elements between w and a
 * pitch are never touched. */
int shg_column_limb_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, int window, int threshold, int32_t* out6,
                        shg_stream_t stream);
int shg_column_shift_u16(const uint16_t* img, int n, int64_t h, int64_t w, int64_t pitch, int64_t plane_stride,
                         const int32_t* host_offset, const int32_t* host_weight4, uint16_t* out, int64_t out_pitch,
                         int64_t out_plane_stride, shg_stream_t stream);

/* ---- differential rotation: a finished disk carried to another time, every on-disk pixel turned back about the solar pole by the
 * angle its latitude rotates in the time difference (not a reference stage; tests/derotate_ref.py restates the call in NumPy, bit for
 * bit).  circle3 = (cx, cy, rad), matrix9 = M (row-major 3 x 3) and rate3 = (k0, k1, k2) are host arrays, read before the call
 * returns; clv is NULL or device memory of n_rings positive, finite doubles (the host cannot check them: the caller guarantees it).
 * M is orthonormal: it takes image coordinates (right, up, towards the observer) to (west, the north pole, the central meridian).
 * k0, k1, k2 are radians: the rotation law A + B sin^2(latitude) + C sin^4(latitude) times the time difference, target minus image.
 * Everything is float64, one IEEE operation a step, no contraction; sqrt and / are correctly rounded; the device calls no
 * trigonometric function.  For the output pixel in row r, column c, with v0 = img[r * pitch + c]:
 *   1  u = ((double)c - cx) / rad;  v = (cy - (double)r) / rad;  d2 = u * u + v * v.  If not d2 < 1: out = v0 (the sky, a prominence).
 *      Else z = sqrt(1 - d2).
 *   2  q_i = (M[i][0] * u + M[i][1] * v) + M[i][2] * z for i = x, y, z.
 *   3  s2 = q_y * q_y;  a = (k2 * s2 + k1) * s2 + k0.  If a == 0: out = v0 (a time difference of 0 is the identity).
 *   4  a2 = a * a;  sa = a * P(a2);  ca = Q(a2), Horner forms from the highest term down with the float64 nearest to +-1 / k!:
 *        P = ((((((S15 a2 + S13) a2 + S11) a2 + S9) a2 + S7) a2 + S5) a2 + S3) a2 + 1,
 *          S3 = -0.16666666666666666, S5 = 0.008333333333333333, S7 = -0.0001984126984126984, S9 = 2.7557319223985893e-06,
 *          S11 = -2.505210838544172e-08, S13 = 1.6059043836821613e-10, S15 = -7.647163731819816e-13;
 *        Q = (((((((C16 a2 + C14) a2 + C12) a2 + C10) a2 + C8) a2 + C6) a2 + C4) a2 + C2) a2 + 1,
 *          C2 = -0.5, C4 = 0.041666666666666664, C6 = -0.001388888888888889, C8 = 2.48015873015873e-05,
 *          C10 = -2.755731922398589e-07, C12 = 2.08767569878681e-09, C14 = -1.1470745597729725e-11, C16 = 4.779477332387385e-14.
 *      The truncation is below 2^-53 for |a| <= 0.5.
 *   5  the source point: x' = q_x * ca - q_z * sa;  z' = q_x * sa + q_z * ca;  y' = q_y;  p = M^T q':
 *      p_u = (M[0][0] * x' + M[1][0] * y') + M[2][0] * z', p_v and p_z with the columns 1 and 2.  If not p_z > 0 (the source lies
 *      behind the limb): out = v0.
 *   6  x = cx + p_u * rad;  y = cy - p_v * rad;  x0 = floor(x), tx = x - x0, y0 = floor(y), ty = y - y0.  The Keys cubic weights
 *      (a = -0.5) of t, in float64: ((-0.5 t + 1) t - 0.5) t, (1.5 t - 2.5) (t t) + 1, ((-1.5 t + 2) t + 0.5) t, (0.5 t - 0.5) (t t),
 *      each rint(. * 16384), what is missing to 16384 added to the second: wx[0..3] of tx, wy[0..3] of ty.  As int64:
 *      H_j = sum over k of wx[k] * img[clamp(y0 + j - 1, 0, h - 1)][clamp(x0 + k - 1, 0, w - 1)];  T = sum over j of wy[j] * H_j;
 *      val = (T + 2^27) >> 28 (the shift is arithmetic).
 *   7  clv NULL: out = clip(val, 0, 65535).  Else, with g(rho) the rule of shg_ring_flatten_u16 on the table (u = rho - 0.5, its two
 *      end clamps, the truncation, the linear step): rho_out = sqrt(d2) * rad, rho_src = sqrt(p_u * p_u + p_v * p_v) * rad,
 *      out = (uint16)clip(rint((double)val * (g(rho_out) / g(rho_src))), 0, 65535): limb darkening belongs to the view, not to the
 *      surface, so a pixel that moves is rescaled by the profile of its new radius over that of its old one.
 * 1 <= h, w <= 16384, else SHG_E_UNSUPPORTED.  SHG_E_ARG for a null pointer other than clv, a pitch below w, a circle outside the
 * limits of shg_ring_medians_u16, n_rings != floor(rad) + 1 (with clv NULL as well), a matrix that is not finite or whose rows'
 * products differ from the identity by more than 1e-12, a rate3 that is not finite or has |k0| + |k1| + |k2| > 0.5 (about 1.9 days at
 * the default law: the polynomials' range), and an out that overlaps img.  On any error nothing is written.  The call allocates
 * nothing, waits for nothing and copies nothing from the device.  Elements between w and a pitch are never touched. */
int shg_derotate_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* circle3, const double* matrix9,
                     const double* rate3, const double* clv, int64_t n_rings, uint16_t* out, int64_t out_pitch, shg_stream_t stream);

/* The two uses of cv2.blur on the path in fused form (the blurred image never leaves the workgroup): row means of
 * blur(img, (kw, kh)) for detect_bord (solex_util.py:166-167), and the first arg-minimum over [x0, x1) of every
 * blurred row together with the first arg-minimum of the unblurred row (solex_util.py:230-231, 242).  Identical
 * results to shg_box_blur_u16 + shg_row_mean_u16 / shg_row_argmin_u16.  shg_blur_fits_fused: whether (8 + kh - 1)
 * rows of w horizontal sums fit the LDS tile (otherwise use the separate entry points). */
int shg_blur_fits_fused(int64_t w, int kh);
int shg_blur_row_mean_u16(const uint16_t* src, int64_t h, int64_t w, int kw, int kh, double* out, shg_stream_t stream);
int shg_blur_argmin_u16(const uint16_t* src, int64_t h, int64_t w, int kw, int kh, int64_t x0, int64_t x1,
                        int32_t* out_blur, int32_t* out_sharp, shg_stream_t stream);

/* ---- pass B: per-frame column extraction ----- solex_util.py:93-144 (read_video_improved)
 * For every frame k, shift s and slit row y:
 *     v = img[y][ind_l[s][y]] * lw[y] + img[y][ind_l[s][y] + 1] * rw[y]     (float64,
 *         two rounded products and one rounded add, no FMA; solex_util.py:131-133)
 *     disks[s][y][col(k)] = (uint16) v                                        (truncation, :134)
 * with col(k) = k_offset + k, or n_cols - 1 - (k_offset + k) when flip_x != 0
 * (np.flip(axis=1), Solex_recon.py:74-76).  ind_l is [n_shifts][ih] int32, already
 * clamped to [0, iw-2] (solex_util.py:114-119); lw, rw are [ih] float64, NOT adjusted
 * for the clamp (solex_util.py:122-123).  disks: n_shifts planes of plane_stride
 * elements, rows of row_pitch elements (row_pitch >= n_cols).
 * Rotated files (width > height, the usual SER) take the band kernel (k_extract_band: a group of shifts per workgroup,
 * every sample loaded once, nontemporal stores); SHG_EXT_GENERAL=1 in the environment keeps the kernel that serves
 * un-rotated files (k_extract) for them too -- the parity tests hold one against the other. */
int shg_extract_columns(const void* stack, int64_t n_frames, int64_t height, int64_t width,
                        int bytes_per_px, int64_t frame_stride_px, const int32_t* ind_l, const double* lw, const double* rw,
                        int n_shifts, uint16_t* disks, int64_t row_pitch, int64_t plane_stride,
                        int64_t n_cols, int64_t k_offset, int flip_x, shg_stream_t stream);

/* The same, and on the way the minimum and maximum of every plane, as the warp clips to them (ellipse_to_circle.py:
 * 112-114): minmax_slots is scratch + result, uint32 [n_shifts][64][2] slots (zeroed by the call, folded by a last tiny
 * kernel) followed by the result [n_shifts][2] = {min, max} -- n_shifts * 130 words in all; pass &result[s * 2] to
 * shg_warp_rows_minmax_u16.  Only meaningful when the call covers the whole scan (a rank's share of a sharded scan
 * gives the extrema of its columns only).  minmax_slots may be NULL. */
int shg_extract_columns_minmax(const void* stack, int64_t n_frames, int64_t height, int64_t width,
                               int bytes_per_px, int64_t frame_stride_px, const int32_t* ind_l, const double* lw, const double* rw,
                               int n_shifts, uint16_t* disks, int64_t row_pitch, int64_t plane_stride,
                               int64_t n_cols, int64_t k_offset, int flip_x, uint32_t* minmax_slots, shg_stream_t stream);

/* The same for a Doppler stack whose shifts are consecutive integers in any order (-w a:b:1 with the two implicit shifts inside
 * the range; 3 <= n_shifts <= 24, shg_extract_dense_fits): a lane loads the n_shifts + 1 distinct samples of a (row, frame)
 * once instead of 2 * n_shifts (rotated files: k_extract_band in groups of up to seven shift values, the file row two groups
 * share read by neighbouring workgroups of one XCD; un-rotated files: k_extract_dense).  host_shifts [n_shifts]: the shift of every plane; base_col [ih]: the column of the smallest
 * shift before the clamps (fit[:, 0] + min shift); ind_l as above, used for the rows whose line lies within n_shifts columns
 * of the frame's edge.  Bit-identical to shg_extract_columns_minmax. */
int shg_extract_dense_fits(const int32_t* host_shifts, int n_shifts);
int shg_extract_columns_dense(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                              int64_t frame_stride_px, const int32_t* ind_l, const int32_t* base_col, const double* lw,
                              const double* rw, const int32_t* host_shifts, int n_shifts, uint16_t* disks, int64_t row_pitch,
                              int64_t plane_stride, int64_t n_cols, int64_t k_offset, int flip_x, uint32_t* minmax_slots,
                              shg_stream_t stream);

/* ---- the warp ---------------------------------- ellipse_to_circle.py:112-118
 * skimage.transform.warp(order=1, mode='constant', cval=image[0,0], clip) for a
 * transform that never moves rows: out[r][c] samples input row r at
 * x = h00*c + h01*r + h02 (float64), bilinear, then clip to [min, max] of the input
 * and (uint16)(65536 * v).  The input is the uint16 disk, interpreted as
 * value/65536 (Solex_recon.py:123, ellipse_to_circle.py:299).  minmax: 2 uint32
 * device scratch words (written by the call). */
int shg_warp_rows_u16(const uint16_t* src, int64_t h, int64_t w, int64_t src_pitch,
                      double h00, double h01, double h02,
                      uint16_t* dst, int64_t out_h, int64_t out_w, int64_t dst_pitch,
                      uint32_t* minmax, shg_stream_t stream);

/* The warp with the input's extrema already known (minmax2 = {min, max}, e.g. from shg_extract_columns_minmax): saves
 * the pass over the input that shg_warp_rows_u16 makes to find them. */
int shg_warp_rows_minmax_u16(const uint16_t* src, int64_t h, int64_t w, int64_t src_pitch,
                             double h00, double h01, double h02,
                             uint16_t* dst, int64_t out_h, int64_t out_w, int64_t dst_pitch,
                             const uint32_t* minmax2, shg_stream_t stream);

/* Which kernel the two entry points above take for this image: 1 where the eight-pixels-a-lane k_warp_rows8 serves it (both
 * pitches multiples of 8, both images 16-byte aligned, at least 8 source columns and two 8-column vectors of output, 32-bit
 * offsets, 0 <= h00 <= 1.75, h01 and h02 below 1e300), 0 where k_warp_rows does.  A pure host function: the pointers are only
 * looked at as numbers, no GPU is touched.  (SHG_WARP_WIDE=0 in the environment sends every image to k_warp_rows whatever this
 * says: the A / B switch is the launcher's.)  A stack goes wide when every one of its disks fits. */
int shg_warp_rows_wide_fits(const uint16_t* src, int64_t h, int64_t w, int64_t src_pitch,
                            double h00, double h01, double h02,
                            const uint16_t* dst, int64_t out_h, int64_t out_w, int64_t dst_pitch);

/* ---- transversalium ---------------------------- solex_util.py:383-395, 76-86
 * Per row y in (y1, y2): the mean of the 2-MAD inliers of log(img[y][a:b] / img[y-1][a:b])
 * with a, b the chord of `circle` clipped to `borders` (float64).  out[y2 - y1]
 * (out[0] = 0 as solex_util.py:386).  xa, xb: int32 [y2-y1] column bounds computed on the
 * host (solex_util.py:389-391).  Images wider than SHG_TRANSV_MAX_COLS
 * (19456 columns: the row's keys must fit the CU's 160 KiB of LDS) are rejected.
 * row_factor (may be NULL): float64 [h]; when given the image is the float64 frame
 * img[y][x] * row_factor[y] that removeVignette returns (solex_util.py:654). */
#define SHG_TRANSV_MAX_COLS 19456
int shg_rowpair_logratio_stats(const uint16_t* img, int64_t h, int64_t w, int64_t pitch,
                               int64_t y1, int64_t y2, const int32_t* xa, const int32_t* xb,
                               const double* row_factor, double* out, shg_stream_t stream);
/* The same, also storing the statistics at out_mirror (may be NULL): a second, GPU-mapped host buffer for the control
 * plane, so that no copy has to follow (shg_stage_process_frames). */
int shg_rowpair_logratio_stats_mirrored(const uint16_t* img, int64_t h, int64_t w, int64_t pitch,
                                        int64_t y1, int64_t y2, const int32_t* xa, const int32_t* xb,
                                        const double* row_factor, double* out, double* out_mirror, shg_stream_t stream);

/* scipy.ndimage.correlate1d(src, weights, axis=-1, mode='constant', cval=0) for k rows of n float64
 * samples with 2*radius+1 float64 weights (device memory), in NI_Correlate1D's order of operations:
 * the interior of scipy.signal.savgol_filter(y_ratios_r, window, 3) (solex_util.py:400).  `symmetric`
 * > 0 selects SciPy's symmetric-filter form (pairs summed first, left half of the weights used), which
 * SciPy takes when |w[R+i] - w[R-i]| <= DBL_EPSILON for every i; < 0 its antisymmetric form (pairs
 * subtracted; |w[R+i] + w[R-i]| <= DBL_EPSILON); 0 the general form. */
int shg_correlate1d_rows_f64(const double* src, int64_t k, int64_t n, const double* weights, int radius,
                             int symmetric, double* dst, shg_stream_t stream);

/* ret = min(img * c[y], 65535) truncated to uint16 (solex_util.py:489, 515-516). */
int shg_scale_rows_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const double* c,
                       const double* row_factor, uint16_t* dst, int64_t dst_pitch, shg_stream_t stream);
/* 1 where shg_scale_rows_u16 takes k_scale_rows8 for this image (16-byte loads and stores: both images 16-byte aligned, both
 * pitches multiples of 8), 0 where it takes k_scale_rows.  A pure host function, as shg_warp_rows_wide_fits. */
int shg_scale_rows_vec_fits(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const uint16_t* dst, int64_t dst_pitch);

/* ---- f4: "stubborn" transversalium, the line filter of apply_lin_filter + fix_edge_effect ----
 * Replaces the three cv2.filter2D calls on log(img) (solex_util.py:277-353) and the limb clean-up
 * (:356-375).  Exact BORDER_REFLECT_101 correlation: float64 sums in a fixed order, rounded once to
 * float32 for a uint16 image (np.log(uint16) is float32) or kept in float64 for the float64 image
 * img * row_factor[y] (row_factor non-NULL).
 *
 * shg_lin_filter_row_sums: hl[h][w] = sum of the `linlen` logs centred on x along row y; hf the same
 * for the image whose flagged rows are replaced by (nearest unflagged row above)/2 + (… below)/2
 * (up/dn: int32 [h], -1 = none; only read where flagged[y] != 0).  log_lut: float32 [65536], the
 * log of every uint16 value as the caller's NumPy computes it (ignored when row_factor is given).
 *
 * shg_lin_filter_apply: delta = hl/linlen - (sum of hf over rows y-half_width..y+half_width except y)
 * /(2*half_width*linlen); kept on columns [xa[y], xb[y]), copied from column xa+edge_half into
 * [xa, xa+edge_half) when edge[y] & 1, from xb-edge_half-1 into [xb-edge_half, xb) when edge[y] & 2,
 * zero elsewhere; dst = min(img * exp(-delta * taper[y]), 65535) truncated (solex_util.py:352, 423).
 * Each edge zone must lie inside [xa, xb) and the two must not overlap (xb - xa >= 2*edge_half + 1 where
 * both bits are set): the kernel takes the left zone first and writes nothing outside [xa, xb), the
 * reference's two slice assignments let the right zone win, so an overlap is resolved differently. */
int shg_lin_filter_row_sums(const uint16_t* img, int64_t h, int64_t w, int64_t pitch,
                            const double* row_factor, const float* log_lut, const uint8_t* flagged,
                            const int32_t* up, const int32_t* dn, int linlen, double* hl, double* hf,
                            shg_stream_t stream);
int shg_lin_filter_apply(const uint16_t* img, int64_t h, int64_t w, int64_t pitch,
                         const double* row_factor, const double* hl, const double* hf, int linlen,
                         int half_width, const double* taper, const int32_t* xa, const int32_t* xb,
                         const uint8_t* edge, int edge_half, uint16_t* dst, int64_t dst_pitch,
                         shg_stream_t stream);

/* np.percentile(img, q, axis) building block (removeVignette, solex_util.py:591-592): for every
 * column (axis 0) or row (axis 1) the rank_lo-th and rank_hi-th smallest values (0-based). */
int shg_line_order_stats_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, int axis,
                             int64_t rank_lo, int64_t rank_hi, uint16_t* out_lo, uint16_t* out_hi,
                             shg_stream_t stream);

/* ---- crop / pad -------------------------------- Solex_recon.py:155-171
 * dst[h][nw] = fill everywhere, then dst[:, dx0:dx0+n] = src[:, sx0:sx0+n].
 * fill: 0..65535, or negative = src[0][0] read on the device (np.full(.., img[0, 0]), :161). */
int shg_crop_pad_u16(const uint16_t* src, int64_t h, int64_t w, int64_t pitch,
                     uint16_t* dst, int64_t nw, int64_t dst_pitch,
                     int64_t sx0, int64_t dx0, int64_t n, int32_t fill, shg_stream_t stream);

/* ---- CLAHE -------------------------------------- solex_util.py:532-533, clahe_apply.py:247
 * cv2.createCLAHE(clipLimit, (tiles, tiles)).apply(img) for uint16 (hist_size 65536)
 * or uint8 (hist_size 256) images.  workspace: tiles*tiles*hist_size uint32 histograms
 * followed by tiles*tiles*hist_size LUT entries (uint16); query the size first. */
size_t shg_clahe_workspace_bytes(int tiles, int bytes_per_px);
/* The size that lets a 16-bit call build its tile histograms without global atomics (slice histograms stored whole
 * and reduced once, the LUT by 32 workgroups per tile): shg_clahe takes that path whenever workspace_bytes allows. */
size_t shg_clahe_workspace_bytes_for(int64_t h, int64_t w, int tiles, int bytes_per_px);
int shg_clahe(const void* img, int64_t h, int64_t w, int64_t pitch, int bytes_per_px,
              double clip_limit, int tiles, void* dst, int64_t dst_pitch,
              void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* 65536-bin (or 256-bin) histogram of an image; hist is zeroed by the call.  Feeds
 * np.percentile / np.max on the host (solex_util.py:535-537). */
int shg_hist(const void* img, int64_t h, int64_t w, int64_t pitch, int bytes_per_px,
             uint32_t* hist, shg_stream_t stream);

/* Exact order statistics of a uint16 image: out[i] (as double) = the host_ranks[i]-th smallest pixel
 * (0-based; rank h*w-1 = np.max).  Feeds np.percentile without moving a histogram to the host. */
size_t shg_select_u16_workspace_bytes(int n_ranks);
int shg_select_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, const int64_t* host_ranks,
                   int n_ranks, double* out, void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* rescale_brightness: trunc(clamp((sat*alpha)*(v-lo)/(hi-lo), 0, sat)), float64, sat = 65535
 * (solex_util.py:519-525). */
int shg_rescale_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch,
                    double lo, double hi, double alpha, uint16_t* dst, int64_t dst_pitch,
                    shg_stream_t stream);
/* The same for 8-bit images (sat = 255): clahe_apply.py:251 stretches 8-bit PNGs too. */
int shg_rescale_u8(const uint8_t* img, int64_t h, int64_t w, int64_t pitch, double lo, double hi,
                   double alpha, uint8_t* dst, int64_t dst_pitch, shg_stream_t stream);

/* cv2.circle(img, (x0, y0), r, value, -1): filled integer midpoint circle, clipped to the
 * image (solex_util.py:542-547).  scratch: unused (may be NULL); kept for ABI stability. */
int shg_fill_disc_u16(uint16_t* img, int64_t h, int64_t w, int64_t pitch,
                      int64_t x0, int64_t y0, int64_t r, uint16_t value, int32_t* scratch,
                      shg_stream_t stream);

/* skimage.transform.downscale_local_mean(img/65536, (f, f)) (ellipse_to_circle.py:299-302):
 * zero-padded block mean, float64 out [ceil(h/f)][ceil(w/f)]. */
int shg_downscale_mean_u16(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, int factor,
                           double* dst, shg_stream_t stream);

/* ---- limb detection on the block-mean image ------ ellipse_to_circle.py:148-250
 * cv2.blur(float64 image, (k, k)) (ellipse_to_circle.py:163, 241): box sums accumulated left to
 * right then top to bottom, times 1/(k*k), BORDER_REFLECT_101, anchor k/2.  tmp: h*w doubles. */
int shg_box_blur_f64(const double* src, int64_t h, int64_t w, int k, double* dst, double* tmp,
                     shg_stream_t stream);

/* cv2.blur for an image whose values are whole numbers of 2^-20 below 1 (the 4x4 block mean of uint16 / 65536,
 * ellipse_to_circle.py:299-301), k <= 63: also keys[i] = the k x k window sum in units of 2^-20 (exact, < 2^32), so that
 * np.median / np.percentile of the blurred image can be selected on 32-bit integers: shg_select_keys_u32, out[i] = the
 * host_ranks[i]-th smallest of host_keys[i][n] turned back into the blurred value, (key * 2^-20) * (1 / (k_i * k_i)) --
 * three 11-bit radix passes instead of the eight 8-bit passes float64 keys take. */
int shg_box_blur_key_f64(const double* src, int64_t h, int64_t w, int k, double* dst, uint32_t* keys, double* tmp,
                         shg_stream_t stream);
size_t shg_select_keys_workspace_bytes(int n_pairs);
int shg_select_keys_u32(const uint32_t* const* host_keys, int64_t n, const int64_t* host_ranks, const int* host_k,
                        int n_pairs, double* out, void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* Exact order statistics: out[i] = the host_ranks[i]-th smallest value (0-based) of values[n]
 * (MSB-first radix select; feeds np.median / np.percentile, ellipse_to_circle.py:165, 241).
 * host_ranks is a HOST array of n_ranks <= 8 entries. */
size_t shg_select_workspace_bytes(int n_ranks);
int shg_select_f64(const double* values, int64_t n, const int64_t* host_ranks, int n_ranks, double* out,
                   void* workspace, size_t workspace_bytes, shg_stream_t stream);
/* the same for several arrays of one length in one launch sequence: out[i] = the host_ranks[i]-th smallest value of
 * host_arrays[i] (HOST array of device pointers). */
int shg_select_multi_f64(const double* const* host_arrays, int64_t n, const int64_t* host_ranks, int n_ranks,
                         double* out, void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* get_flood_image's statistics (ellipse_to_circle.py:159-169): stats[0] = np.sum(image) (image
 * values are multiples of 2^-20, as the 4x4 block mean of uint16/65536 is), and over
 * data = blurred[blurred < very_bright]: stats[1] = min, stats[2] = max,
 * counts[20] = np.histogram(data, bins=20)[0].  workspace: 256 bytes. */
int shg_flood_stats_f64(const double* image, const double* blurred, int64_t n, double very_bright,
                        double* stats, uint32_t* counts, void* workspace, shg_stream_t stream);
/* The same with very_bright = np.percentile(blurred, 99) formed on the device from the two order
 * statistics order_stats[0..1] (device memory, e.g. shg_select_multi_f64's output) by NumPy's _lerp
 * with weight gamma: b - (b-a)*(1-gamma) if gamma >= 0.5 else a + (b-a)*gamma. */
int shg_flood_stats_lerp_f64(const double* image, const double* blurred, int64_t n,
                             const double* order_stats, double gamma, double* stats, uint32_t* counts,
                             void* workspace, shg_stream_t stream);

/* skimage.feature.canny(flooded, sigma, low, high) up to its two hysteresis masks
 * (ellipse_to_circle.py:245-250), where flooded = (blurred < flood_thresh ? 0 : 65000)
 * (ellipse_to_circle.py:226-227).  host_gauss_weights: the 2*radius+1 normalised Gaussian taps
 * (HOST pointer, copied into the launch).  low_mask / high_mask: uint8 [h][w] =
 * local_maxima & (magnitude >= low / high).  The 8-connected hysteresis is a labelling step
 * the caller does on those masks. */
size_t shg_canny_workspace_bytes(int64_t h, int64_t w);
int shg_canny_masks_f64(const double* blurred, int64_t h, int64_t w, double flood_thresh,
                        const double* host_gauss_weights, int radius, double low, double high,
                        uint8_t* low_mask, uint8_t* high_mask, void* workspace, size_t workspace_bytes,
                        shg_stream_t stream);

/* canny's hysteresis and the labelling of its result (ellipse_to_circle.py:245-252): the pixels of
 * the 8-connected components of low_mask that contain a high_mask pixel, in raster order:
 * out_idx[i] = y*w + x, out_root[i] = smallest linear index of the pixel's component (sorting the
 * distinct roots gives scipy.ndimage.label's numbering), out_count[0] = number of pixels.
 * out_idx / out_root: h*w int32 each. */
size_t shg_edge_components_workspace_bytes(int64_t h, int64_t w);
int shg_edge_components(const uint8_t* low_mask, const uint8_t* high_mask, int64_t h, int64_t w,
                        int32_t* out_idx, int32_t* out_root, int32_t* out_count,
                        void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* ---- image_process in two calls --------------------------------- solex_util.py:527-547
 * shg_contrast_stats_u16: cl1 = CLAHE(frame, clip_limit, tiles), then the order statistics np.percentile and np.max
 * need: out5[0..1] = frame's ranks_frame2[0..1]-th smallest pixels, out5[2..4] = cl1's ranks_cl13[0..2]-th (host
 * rank arrays).  shg_contrast_products_u16: high_contrast = rescale(frame, lo_hi6[0], lo_hi6[1]), protus =
 * rescale(frame, lo_hi6[2], lo_hi6[3]), cc = rescale(cl1, lo_hi6[4], lo_hi6[5]) (host doubles), then the filled disc
 * of value 80 on protus when disc_r > 0 (:542-547).  Same kernels and order as the separate entry points. */
size_t shg_contrast_stats_workspace_bytes(int tiles);
size_t shg_contrast_stats_workspace_bytes_for(int64_t h, int64_t w, int tiles);   /* with shg_clahe_workspace_bytes_for's room */
int shg_contrast_stats_u16(const uint16_t* frame, int64_t h, int64_t w, int64_t pitch, double clip_limit,
                           int tiles, uint16_t* cl1, int64_t cl1_pitch, const int64_t* ranks_frame2,
                           const int64_t* ranks_cl13, double* out5, void* workspace, size_t workspace_bytes,
                           shg_stream_t stream);
int shg_contrast_products_u16(const uint16_t* frame, int64_t frame_pitch, const uint16_t* cl1, int64_t cl1_pitch,
                              int64_t h, int64_t w, const double* lo_hi6, uint16_t* high_contrast,
                              uint16_t* protus, uint16_t* cc, int64_t dst_pitch, int64_t disc_x0,
                              int64_t disc_y0, int64_t disc_r, shg_stream_t stream);
/* 1 where shg_contrast_products_u16 takes k_products8 for these five images (all 16-byte aligned, the three pitches multiples
 * of 8, at least 9 columns -- two vectors a row --, 32-bit offsets), 0 where it takes k_products.  A pure host function, as
 * shg_warp_rows_wide_fits. */
int shg_contrast_products_vec_fits(const uint16_t* frame, int64_t frame_pitch, const uint16_t* cl1, int64_t cl1_pitch,
                                   int64_t h, int64_t w, const uint16_t* high_contrast, const uint16_t* protus,
                                   const uint16_t* cc, int64_t dst_pitch);

/* What the contrast stage of shg_stage_process_frames would do with k disks [h][w] (rows `pitch` apart, the CLAHE images rows
 * `dst_pitch` apart; ptr_bits: the OR of the low four bits of every image pointer, 0 for 16-byte aligned images) at this clip limit
 * and tile grid: the plan of its first launch (the first 32 disks), as plan_clahe makes it -- the same function, the same
 * environment knobs, nothing decided differently for being asked.  fused != 0: the images are still to be formed by the histogram
 * kernel (taken only where the stage batches); want_ranks != 0: np.percentile(frame, 99.9999)'s two order statistics ride on the
 * LUT kernel (the batched route always asks for them); want_window: 0 / 1, or negative for what the stage asks for at this many
 * disks.  A pure host function, as shg_warp_rows_wide_fits: no pointer is followed, no GPU touched, the workspace taken as roomy.
 * out[SHG_PLAN_FIELDS]:
 *   [0] 1 = all disks through one launch per kernel, 0 = disk by disk (shg_contrast_stats_u16)      [1] disks in that launch
 *   [2] route: 0 / 1 = 8- / 16-bit atomics, 2 / 3 / 4 = slices with u16 / byte / nibble counters     [3] counter bits (0: atomics)
 *   [4] clip (pixels a bin; 0 = no clipping)   [5] rows a slice   [6] slices a tile   [7] rows between two clamps (a chunk)
 *   [8], [9] the frame's ranks as the LUT kernel takes them (0 where none ride along)   [10] 1 = they count from the top
 *   [11] pixels a lane of the blend   [12] 1 = its lanes dealt in tiles   [13] 1 = a LUT workgroup builds every tile's entries
 *   [14] 1 = the percentile window is counted   [15] 1 = the histogram kernel forms the images
 * Returns 0, or the code the launch would fail with (shg_last_error has the text). */
#define SHG_PLAN_FIELDS 16
int shg_contrast_plan_query(int64_t k, int64_t h, int64_t w, int64_t pitch, int64_t dst_pitch, int ptr_bits, double clip_limit,
                            int tiles, int fused, int want_ranks, int want_window, int64_t* out);

/* ---- the limb stage's kernels fused through LDS tiles ------ ellipse_to_circle.py:148-291, 299-302 (csrc/limb_fused.hip)
 * The same arithmetic as shg_downscale_mean_u16 / shg_box_blur_key_f64 / shg_select_keys_u32 / shg_flood_stats_lerp_f64 and
 * shg_canny_masks_f64 / shg_edge_components, bit for bit, in 5 + 3 launches instead of 12 + 11.
 * shg_limb_fused_fits: whether the k x k blur window (k = int(0.01 * sh)) fits the tile (k <= 16).
 * shg_limb_prepare: for the uint16 disk [h][w] and its 4x4 block mean [sh = ceil(h/4)][sw = ceil(w/4)]: cv2.blur with windows k
 *   and 5 (as 32-bit window sums in units of 2^-20), host_ranks4 = the two order statistics of np.median(blur 5) and the two
 *   of np.percentile(blur k, 99), very_bright = NumPy's _lerp of the latter with weight gamma99, and np.sum(image), min, max,
 *   np.histogram(., 20) of blur k below very_bright.  packed (device or GPU-mapped host memory, 32 doubles): [0..3] order
 *   statistics, [4] sum, [5] min, [6] max, 20 uint32 counts at packed + 8.  *keys_out: the window sums of blur k, inside the
 *   workspace, for shg_limb_edges.
 * shg_limb_edges: canny (flooded = blurred < flood_thresh ? 0 : 65000; Gaussian taps as shg_canny_masks_f64) and the
 *   8-connected labelling of its LOW mask: comp (device or GPU-mapped host memory, 2 * sh * sw + 1 int32) = [m | idx[n] |
 *   root[n]]: the m low-mask pixels in raster order, root = smallest linear index of the pixel's component, bit 30 of root set
 *   where the pixel is in the HIGH mask (hysteresis = keep the components holding such a pixel: one pass for the caller). */
int shg_limb_fused_fits(int64_t sh, int64_t sw, int k);
size_t shg_limb_prepare_workspace_bytes(int64_t sh, int64_t sw, int k);
int shg_limb_prepare(const uint16_t* img, int64_t h, int64_t w, int64_t pitch, int k, const int64_t* host_ranks4, double gamma99,
                     double* packed, const uint32_t** keys_out, void* workspace, size_t workspace_bytes, shg_stream_t stream);
size_t shg_limb_edges_workspace_bytes(int64_t sh, int64_t sw);
int shg_limb_edges(const uint32_t* keys, int64_t sh, int64_t sw, int k, double flood_thresh, const double* host_gauss_weights,
                   int radius, double low, double high, int32_t* comp, void* workspace, size_t workspace_bytes, shg_stream_t stream);

/* ==== stage composites ============================================================================
 * Each stage function of the reference as one call: the same kernels in the same order as the entry points
 * above, the scalars / 1-D vectors in between brought to the host through PINNED memory and handled by the
 * host control plane below -- no interpreter (and no interpreter lock) between the kernels, so several
 * scans run side by side in one process.  Device `workspace` and pinned `host_pinned` staging areas are
 * sized by the *_bytes queries; a stage synchronises `stream` where the control plane needs a result. */

/* compute_mean_return_fit (solex_util.py:191-259): pass A (or the given, e.g. all-reduced, sum_in / max_in),
 * mean / max images [ih][iw] (dense), detect_bord, the two argmin traces, the cubic fit.
 * host_y12 = clipped (y1, y2); host_p4 lowest power first; host_fit [ih][4]; host_trace_sharp [ih] and
 * host_mask_good [y2-y1 <= ih] (both may be NULL) feed the reference's diagnostic plot. */
size_t shg_stage_mean_fit_workspace_bytes(int64_t n_frames, int64_t height, int64_t width, int bytes_per_px);
size_t shg_stage_mean_fit_host_bytes(int64_t height, int64_t width);
int shg_stage_mean_fit(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                       int64_t frame_stride_px, const uint64_t* sum_in, const uint16_t* max_in, int64_t n_total,
                       uint16_t* mean_out, uint16_t* max_out, int64_t* host_y12, double* host_p4, double* host_fit,
                       int32_t* host_trace_sharp, uint8_t* host_mask_good, void* workspace, size_t workspace_bytes,
                       void* host_pinned, size_t host_pinned_bytes, shg_stream_t stream);

/* read_video_improved (solex_util.py:93-144) from the host `fit` and shift list: sample columns and weights
 * (shg_host_column_plan), upload, shg_extract_columns_minmax -- or shg_extract_columns_dense for consecutive shifts
 * (minmax_slots may be NULL).  Asynchronous: host_pinned is read by the GPU after the call has returned and must stay untouched
 * until the work queued on `stream` up to here has run. */
size_t shg_stage_extract_workspace_bytes(int64_t height, int64_t width, int n_shifts);   /* device and pinned */
int shg_stage_extract(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                      int64_t frame_stride_px, const double* host_fit, const int32_t* host_shifts, int n_shifts,
                      uint16_t* disks, int64_t row_pitch, int64_t plane_stride, int64_t n_cols, int64_t k_offset,
                      int flip_x, uint32_t* minmax_slots, void* workspace, size_t workspace_bytes, void* host_pinned,
                      size_t host_pinned_bytes, shg_stream_t stream);

/* get_edge_list on the 4x4 block mean of the disk (ellipse_to_circle.py:231-291, 299-302): flood image, canny ladder
 * (sigma 2, 1.5, 1, 0.5; host_gauss_taps = scipy's taps for those, 17 + 13 + 9 + 5 values), hysteresis + labelling,
 * region choice, convex-hull filter, row crop.  host_points [points_cap][2]: edge pixels (row, col) of the quarter-size
 * image in raster order; host_flags [points_cap]: 1 = limb point; host_counts2 = edge pixels, limb points.  The
 * ellipse fit on the limb points stays with the caller (NumPy, see csrc/hostmath.hip). */
size_t shg_stage_limb_points_workspace_bytes(int64_t h, int64_t w);
size_t shg_stage_limb_points_host_bytes(int64_t h, int64_t w);
int shg_stage_limb_points(const uint16_t* disk, int64_t h, int64_t w, int64_t pitch, const double* host_gauss_taps,
                          int32_t* host_points, uint8_t* host_flags, int64_t points_cap, int64_t* host_counts2,
                          void* workspace, size_t workspace_bytes, void* host_pinned, size_t host_pinned_bytes,
                          shg_stream_t stream);

/* ellipse_to_circle without its warp (ellipse_to_circle.py:294-314): shg_stage_limb_points, then two_step, correct_image's
 * geometry and the borders (shg_host_limb_geometry).  Flag bit 1 = kept by two_step; host_counts3 = edge pixels, limb
 * points, kept points. */
int shg_stage_limb_fit(const uint16_t* disk, int64_t h, int64_t w, int64_t pitch, const double* host_gauss_taps,
                       int32_t* host_points, uint8_t* host_flags, int64_t points_cap, int64_t* host_counts3,
                       double* host_geom16, int64_t* host_dims2, double* host_outline200, void* workspace,
                       size_t workspace_bytes, void* host_pinned, size_t host_pinned_bytes, shg_stream_t stream);

/* single_image_process for the k requested disks of a file (Solex_recon.py:136-174; solex_util.py:383-516,
 * 527-547): transversalium, crop / pad, CLAHE + order statistics, the three rescales + protuberance disc.
 * See csrc/stages.hip for the argument list. */
size_t shg_stage_process_workspace_bytes(int64_t k, int64_t h, int64_t w, int64_t crop_w, int tiles);
size_t shg_stage_process_host_bytes(int64_t k, int64_t h);
int shg_stage_process_frames(const uint16_t* const* host_frames, int64_t k, int64_t h, int64_t w, int64_t pitch,
                             int transversalium, const double* host_circle3, const double* host_borders4,
                             const double* host_taps, int64_t window, double* host_factors, int64_t crop_w,
                             int64_t sx0, int64_t dx0, int64_t ncopy, double clip_limit, int tiles, int64_t disc_x0,
                             int64_t disc_y0, int64_t disc_r, uint16_t* const* host_detrans, int64_t detrans_pitch,
                             uint16_t* const* host_final, uint16_t* const* host_cl1, uint16_t* const* host_hc,
                             uint16_t* const* host_protus, uint16_t* const* host_cc, int64_t out_pitch, void* workspace,
                             size_t workspace_bytes, void* host_pinned, size_t host_pinned_bytes, shg_stream_t stream);

/* ==== one scan, one call =========================================================================
 * The whole per-file flow of solex_do_work's loop body (Solex_recon.py:33-42: solex_read :50-83, solex_process :94-134,
 * single_image_process :136-174) as ONE call, so that nothing of a scan in flight waits for the caller's interpreter:
 * shg_stage_mean_fit -> shg_stage_extract -> (limb fit of the first disk, or the fixed ratio / slant of the options) ->
 * the warp of every requested disk -> shg_stage_process_frames.  Same kernels and host control plane as the stage
 * composites; what the caller's language would have done between them (shift bookkeeping, phi through degrees and back
 * as options['slant_fix'] stores it, the crop plan, the protuberance disc, the Savitzky-Golay window) is restated here.
 * Image sizes after the warp are only known once the limb is fitted, so the images go into two ARENAS the caller sizes by
 * guess: when one (or the workspace) turns out too small the call returns SHG_E_WORKSPACE with needed_* filled in and
 * phase_done = 3; the caller grows the buffers and calls again with start_phase = 3 and the same result struct (the raw
 * disks and the geometry are kept; nothing is computed twice). */
typedef struct shg_scan_request {
    uint32_t struct_bytes;            /* sizeof(shg_scan_request) of the caller */
    int32_t  start_phase;             /* 0: whole scan; 3: resume at the warp after SHG_E_WORKSPACE */
    /* the frame stack, file layout */
    const void* stack;
    int64_t  n_frames, height, width, frame_stride_px;
    int32_t  bytes_per_px;
    int32_t  flip_x;                  /* options['flip_x'] (Solex_recon.py:74-76) */
    /* options['shift'] after solex_read's de-duplication (:55): [ellipse_fit_shift, 0, requested...] */
    const int32_t* host_shifts;
    const uint8_t* host_requested;    /* [n_shifts]: shift in options['shift_requested'] */
    int32_t  n_shifts;
    int32_t  want_fit_image;          /* warp the first disk even when it is not requested (diagnostic plot) */
    double   ratio_fixe, slant_fix_deg;   /* options['ratio_fixe'] / ['slant_fix']; NaN = None (both NaN: fit the limb) */
    int32_t  transversalium, keep_detrans;
    int64_t  trans_strength;
    const double* host_taps;          /* savgol_coeffs(taps_window, 3) for the window the caller expects (may be NULL); */
    int64_t  taps_window;             /* another window is asked from shg_host_set_savgol_taps's callback */
    int32_t  crop_square, has_fixed_width;
    int64_t  fixed_width;
    int32_t  disk_display, tiles;
    int64_t  delta_radius;
    double   clip_limit;
    const double* host_gauss_taps;    /* as shg_stage_limb_points */
    /* device buffers of the caller */
    uint16_t* mean_out;               /* [ih][iw] dense */
    uint16_t* max_out;
    uint16_t* disks;                  /* [n_shifts] planes, rows of disk_pitch elements */
    int64_t  disk_pitch, disk_plane_stride;
    uint32_t* minmax_slots;           /* n_shifts * 130 words (shg_extract_columns_minmax) */
    void*    arena;                   /* images the caller may drop early: corrected frames, final / CLAHE / high-contrast */
    size_t   arena_bytes;
    void*    results;                 /* the images solex_process returns: protus and cc of every requested disk */
    size_t   results_bytes;
    void*    workspace;
    size_t   workspace_bytes;
    void*    host_pinned;             /* page-locked, GPU-mapped; read by the GPU until the call's last kernel has run */
    size_t   host_pinned_bytes;
    /* host outputs */
    double*  host_fit;                /* [ih][4] */
    int32_t* host_trace_sharp;        /* [ih] or NULL */
    uint8_t* host_mask_good;          /* [ih] or NULL */
    int32_t* host_points;             /* [points_cap][2] */
    uint8_t* host_flags;              /* [points_cap] */
    int64_t  points_cap;              /* ceil(ih/4) * ceil(n_frames/4) always suffices */
    double*  host_outline200;         /* or NULL */
    double*  host_factors;            /* [n_out][ih] transversalium row factors, or NULL */
} shg_scan_request;

typedef struct shg_scan_result {
    int32_t phase_done;               /* 0 nothing | 1 line fit | 2 raw disks | 3 geometry | 4 products */
    int32_t limb_fitted;              /* this call fitted the limb (options['ratio_fixe'] / ['slant_fix'] are to be set) */
    int64_t y1, y2;                   /* backup bounds */
    double  p4[4];
    int64_t counts3[3];               /* edge pixels, limb points, kept points */
    double  geom16[16];               /* shg_host_limb_geometry (when limb_fitted) */
    double  phi, ratio;               /* limb fit: its phi and ratio; else radians(slant_fix) or 0, ratio_fixe or 1 */
    double  h_first[3], h_rest[3];    /* warp row (h00, h01, h02) of the first disk / of the others (phi through degrees) */
    double  theta_first, theta_rest;
    double  circle3[3], borders4[4];  /* cercle0 ((-1,-1,-1) without a limb fit), borders */
    double  circle_out3[3];           /* the circle after the crop block */
    int64_t out_h, out_w, frame_pitch;        /* circularised frames: [out_h][out_w], rows frame_pitch elements apart */
    int64_t n_out, prod_w, prod_pitch;        /* requested disks; products [out_h][prod_w] */
    int64_t window;                   /* Savitzky-Golay window used (0: transversalium off) */
    int64_t crop4[4];                 /* crop plan (new width, source x0, destination x0, columns copied); new width 0 = none */
    int64_t disc3[3];                 /* protuberance disc x0, y0, r (r = 0: none) */
    /* byte offsets into the arena; -1 = absent */
    int64_t fit_image_off;            /* the corrected first disk when it is not a requested one */
    int64_t frames_off;               /* [n_out][out_h][frame_pitch] */
    int64_t detrans_off;              /* [n_out][out_h][frame_pitch] */
    int64_t products_off;             /* [n_out][3][out_h][prod_pitch]: final, cl1, high contrast */
    int64_t results_off;              /* into `results`: [n_out][2][out_h][prod_pitch]: protus, cc */
    size_t  needed_arena_bytes, needed_results_bytes, needed_workspace_bytes;
} shg_scan_result;

size_t shg_scan_workspace_bytes(const shg_scan_request* req);      /* phases 0-2; the rest is reported by needed_workspace_bytes */
size_t shg_scan_host_bytes(const shg_scan_request* req);           /* the whole call */
int shg_scan_file(const shg_scan_request* req, shg_scan_result* res, shg_stream_t stream);
/* savgol_coeffs(window, 3) for a window other than request.taps_window: fn(window, out[window]) returns 0, or an SHG_E_*
 * code (SHG_E_VALUE where SciPy raises ValueError). */
typedef int (*shg_savgol_taps_fn)(int64_t window, double* out);
int shg_host_set_savgol_taps(shg_savgol_taps_fn fn);

/* ==== scan pool ===================================================================================
 * The reference's Pool(4) (Solex_recon.py:30-42) as native threads: n_workers threads of the current device, thread k
 * with streams[k], run the submitted shg_scan_file requests in submission order; host_cpus (may be NULL) is where the
 * threads should run.  The request, its buffers and the result must stay alive until shg_pool_wait has returned for the
 * ticket; by then the scan's last kernel has run (the worker synchronises its stream).  shg_pool_wait: blocks until the
 * ticket is done, -> *scan_status = what shg_scan_file returned, error_buf = its message.  shg_pool_poll: 1 done, 0 not yet.
 * shg_pool_destroy runs what is queued, then joins the threads. */
typedef struct shg_pool shg_pool;
int shg_pool_create(const shg_stream_t* streams, int n_workers, const int32_t* host_cpus, int n_cpus, shg_pool** out);
int shg_pool_submit(shg_pool* pool, const shg_scan_request* req, shg_scan_result* res, int64_t* ticket);
/* The same, naming the stream the stack was produced on (0 = the null stream).  With a frame-pass lane set, the scan's pass A
 * (solex_util.py:174-188) is launched on the lane right here, behind what that stream holds now, and the worker that later runs
 * the scan finds it there: the lane does not idle while every worker is still in the chain of an earlier scan. */
int shg_pool_submit_after(shg_pool* pool, const shg_scan_request* req, shg_scan_result* res, shg_stream_t after, int64_t* ticket);
/* The pieces shg_pool_submit_after is made of (a caller with a queue of its own): start pass A of a request / of a stack ahead
 * of shg_scan_file / shg_accumulate_mean_max with the same arguments (*launched = 0: no lane, nothing done), and wait for and
 * drop a pass that nobody came to use. */
int shg_scan_prelaunch(const shg_scan_request* req, shg_stream_t after, int* launched);
int shg_pass_a_prelaunch(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                         int64_t frame_stride_px, void* workspace, size_t workspace_bytes, shg_stream_t after, int* launched);
int shg_pass_a_forget(const void* workspace);
/* Measurement aid (tools/lane_packets.py): `launches` passes A back to back on `stream`, all into `workspace`, with between two
 * launches  mode 0: three event records (two timed, one not),  1: one,  2: nothing,  3: nothing, an event bound to every launch
 * as the lane binds it (and, while the profiler is enabled for "accumulate", a sample per launch).  -> milliseconds per launch. */
int shg_lane_packets_probe(const void* stack, int64_t n_frames, int64_t height, int64_t width, int bytes_per_px,
                           int64_t frame_stride_px, void* workspace, size_t workspace_bytes, int mode, int launches,
                           shg_stream_t stream, double* ms_per_launch);
int shg_pool_poll(shg_pool* pool, int64_t ticket);
int shg_pool_wait(shg_pool* pool, int64_t ticket, int* scan_status, char* error_buf, size_t error_cap);
int shg_pool_destroy(shg_pool* pool);

/* ==== streams of a scan worker pool ==============================================================
 * The reference post-processes up to four files at once (Pool(4), Solex_recon.py:30-42).  Scans in flight share one
 * device: shg_frame_pass_lane_set names ONE stream of the current device through which pass A of every scan runs
 * (shg_accumulate_mean_max, and with it shg_stage_mean_fit / shg_scan_file) -- HBM-bound passes side by side only halve
 * each other's bandwidth; the caller's stream waits for its pass through an event.  NULL switches the lane off.
 * shg_stream_create: priority < 0 high, 0 normal, > 0 low; host_cu_mask (n_mask_words 32-bit words, bit i = CU i, may be
 * NULL) confines the stream's kernels to those CUs (hipExtStreamCreateWithCUMask; priority is ignored then). */
int shg_device_cu_count(int* out);
int shg_stream_create(int priority, const uint32_t* host_cu_mask, int n_mask_words, shg_stream_t* out);
int shg_stream_destroy(shg_stream_t stream);
int shg_frame_pass_lane_set(shg_stream_t lane);
shg_stream_t shg_frame_pass_lane_get(void);

/* ==== host control plane =======================================================================
 * The 1-D / scalar arithmetic between the kernels, restated from the reference's NumPy / SciPy calls so
 * that a pipeline stage is one call that holds no interpreter lock (several scans in flight per process).
 * Every pointer here is a HOST pointer; no GPU is needed.  The line fit follows NumPy operation by
 * operation and solves its least-squares systems with the very LAPACK routine NumPy loaded
 * (shg_host_bind_lapack: address of the ILP64 Fortran dgelsd, scipy_dgelsd_64_ in NumPy 2.x wheels), so
 * `fit` -- and with it the raw disks -- is bit-identical to the reference's on the same host. */
int shg_host_bind_lapack(void* dgelsd_ilp64);          /* NULL: fall back to a built-in Householder QR */
int shg_host_lapack_bound(void);
/* The mode of the rounded line residuals is `values[np.argpartition(-counts, kth=2)[:2][0]]` (solex_util.py:245-247):
 * one of the two most frequent values, which one being up to NumPy's selection kernel on this CPU.  A binding that
 * wants NumPy's very choice registers a picker (called with -counts, returns the index); NULL = the first most
 * frequent value (the scalar introselect's answer). */
typedef int64_t (*shg_mode_pick_fn)(const int64_t* neg_counts, int64_t n);
int shg_host_set_mode_pick(shg_mode_pick_fn pick);
/* np.polyfit(x, y, 3): coefficients, highest power first (solex_util.py:233, 238, 255; scipy _fit_edge) */
int shg_host_polyfit3(const double* host_x, const double* host_y, int64_t n, double* host_coef4);
/* detect_bord's decision on the row means of the blurred image (solex_util.py:167-172) */
int shg_host_detect_bord(const double* host_row_means, int64_t n, int64_t* lb, int64_t* ub);
/* compute_mean_return_fit from the two argmin traces on (solex_util.py:231-259): trace_blur relative to column
 * blur_offset (= 12), rows [y1, y2) fitted; p4 lowest power first, fit[ih][4] = [floor(c), c - floor(c), y, c],
 * mask_good[y2 - y1] (may be NULL).  SHG_E_VALUE when fewer than 3 distinct residuals (:246), SHG_E_TYPE on an
 * empty fit, SHG_E_LINALG when the SVD fails. */
int shg_host_line_fit(const int32_t* host_trace_blur, const int32_t* host_trace_sharp, int64_t ih, int64_t y1,
                      int64_t y2, int32_t blur_offset, double* host_p4, double* host_fit, uint8_t* host_mask_good);
/* read_video_improved's per-shift sample columns and weights (solex_util.py:113-123) */
int shg_host_column_plan(const double* host_fit, int64_t ih, int64_t iw, const int32_t* host_shifts, int n_shifts,
                         int32_t* host_ind_l, double* host_lw, double* host_rw);
/* get_flood_image's threshold from the reduced image statistics (ellipse_to_circle.py:159-225).  Empty data (a constant image:
 * the kernels leave mn / mx as NaN and 20 zero counts): SHG_E_VALUE, never a threshold. */
int shg_host_flood_threshold(double total, int64_t h, int64_t w, double mn, double mx, const int64_t* host_counts20,
                             double* thresh_out);
/* get_edge_list after canny (ellipse_to_circle.py:251-291): region choice, convex-hull filter, row crop on the
 * labelled edge pixels (shg_edge_components' output); out_sel[m] = 1 for limb points */
int shg_host_limb_points(const int32_t* host_idx, const int32_t* host_root, int64_t m, int64_t h, int64_t w,
                         uint8_t* host_out_sel, int64_t* n_selected);
/* The limb geometry with NumPy's own BLAS / LAPACK: phi and ratio steer every sample position of the warp, so the
 * scatter matrices, 3x3 inverses and the eigen-decomposition of the ellipse fit come out of the routines NumPy calls,
 * called the way its matmul / inv / eig call them (csrc/hostmath.hip).  shg_host_bind_blas takes the ILP64 entry
 * points cblas_dgemm, cblas_dsyrk, cblas_dgemv, dgesv, dgeev of the OpenBLAS NumPy loaded; without them the
 * functions below return SHG_E_UNSUPPORTED and the caller keeps the geometry in NumPy. */
int shg_host_bind_blas(void* cblas_dgemm_ilp64, void* cblas_dsyrk_ilp64, void* cblas_dgemv_ilp64, void* dgesv_ilp64,
                       void* dgeev_ilp64);
int shg_host_blas_bound(void);
/* LsqEllipse().fit(points).as_parameters() (ellipse_to_circle.py:57-59), Halir & Flusser */
int shg_host_fit_ellipse(const double* host_points, int64_t n, double* host_center2, double* width, double* height,
                         double* phi);
/* get_correction_matrix (ellipse_to_circle.py:39-50): inverse matrix (row major) and theta */
int shg_host_correction_matrix(double phi, double r, double* host_inv4, double* theta_out);
/* two_step (ellipse_to_circle.py:62-91); host_kept[n] and outline200 = return_fit(n_points=100) may be NULL */
int shg_host_two_step(const double* host_points, int64_t n, double* host_center2, double* height_out, double* phi_out,
                      double* ratio_out, uint8_t* host_kept, int64_t* n_kept, double* host_outline200);
/* correct_image's geometry (ellipse_to_circle.py:100-122) */
int shg_host_warp_geometry(double phi, double ratio, int64_t h, int64_t w, double* host_mat3_9, double* host_inv4,
                           double* host_origin2, double* det_out, double* theta_out, int64_t* out_h, int64_t* out_w);
/* ellipse_to_circle after get_edge_list (ellipse_to_circle.py:303-314): two_step on the limb points (row, col), the geometry
 * of the corrected h x w disk, its circle and the borders of the kept points.  host_geom16 = ellipse centre x, y, height,
 * phi, ratio | circle cx, cy, r | borders[4] | mat3 row 0 (h00, h01, h02 for shg_warp_rows_u16) | theta; host_dims2 = out_h,
 * out_w; host_kept [n] and host_outline200 may be NULL. */
int shg_host_limb_geometry(const double* host_points, int64_t n, int64_t h, int64_t w, double* host_geom16,
                           int64_t* host_dims2, uint8_t* host_kept, int64_t* n_kept, double* host_outline200);
/* correct_transversalium2's chord slices (solex_util.py:384-391); xa, xb: max(y2-y1, 1) entries */
int shg_host_chord_bounds(double cx, double cy, double r, double b0, double b2, int64_t y1, int64_t y2, int64_t w,
                          int32_t* host_xa, int32_t* host_xb);
/* correction factors from the row-pair statistics (solex_util.py:400-404, 456-472); taps = savgol_coeffs(window, 3) */
int shg_host_transversalium_factors(const double* host_ratios, const double* host_interior, int64_t k, int64_t n,
                                    const double* host_taps, int64_t window, int tapered, double* host_out);
/* np.percentile's two order statistics and lerp weight; NumPy's _lerp */
int shg_host_percentile_plan(int64_t n, double q, int64_t* rank_lo, int64_t* rank_hi, double* gamma);
double shg_host_lerp(double a, double b, double gamma);

#ifdef __cplusplus
}
#endif
#endif /* SHG_HIP_H */
