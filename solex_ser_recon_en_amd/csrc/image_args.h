// What the host code of the disk products' entry points (rings.hip, stack.hip, wavelet.hip, deconvolve.hip), of the patch kernels (patch_args.h) and of the map detrend
// (detrend.hip) share: the checks of an image argument, byte spans and their overlap, row alignment, the workspace's round-up, the optional disk
// mask and the cleared table.  Host only: no kernel and no kernel argument struct is declared here.
#pragma once

#include "shg_common.h"

#include <math.h>

namespace shg {

constexpr int kMaxImageDim = 16384;

inline bool image_dims_ok(int64_t h, int64_t w) { return h >= 1 && h <= kMaxImageDim && w >= 1 && w <= kMaxImageDim; }

// `pointers`: none of the entry point's pointers is null; `images`: "an image", or "images" of one shape with `pitch` the smallest.
inline int check_images(const char* fn, bool pointers, const char* images, int64_t h, int64_t w, int64_t pitch) {
    SHG_REQUIRE(pointers, SHG_E_ARG, "%s: null pointer", fn);
    SHG_REQUIRE(image_dims_ok(h, w), SHG_E_UNSUPPORTED, "%s: %s of %lld x %lld (1 to %d either way)", fn, images, (long long)h, (long long)w,
                kMaxImageDim);
    SHG_REQUIRE(pitch >= w, SHG_E_ARG, "%s: pitch < w", fn);
    return 0;
}
inline int check_image(const char* fn, const void* img, int64_t h, int64_t w, int64_t pitch) {
    return check_images(fn, img != nullptr, "an image", h, w, pitch);
}

// [p, p + ((h - 1) pitch + w) item) of an image
struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const void* p, int64_t h, int64_t w, int64_t pitch, size_t item) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + (uintptr_t)((h - 1) * pitch + w) * item};
}
inline bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

// every row of the image starts on a multiple of `align` bytes
inline bool rows_aligned(const void* p, int64_t pitch_elements, size_t element_bytes, size_t align) {
    return reinterpret_cast<uintptr_t>(p) % align == 0 && (pitch_elements * (int64_t)element_bytes) % (int64_t)align == 0;
}

// A workspace is used from its first multiple of kWorkspaceAlign bytes on: an entry point asks for that many bytes more.
constexpr size_t kWorkspaceAlign = 256;
inline uint8_t* align_up(void* workspace, size_t align) {
    return reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(workspace) + align - 1) / align * align);
}

// The optional disk of a pixel set: circle3 NULL or (-1, -1, -1) is no mask (*masked = 0, the rest untouched), else cx, cy, rad^2.
inline int parse_disk_mask(const char* fn, const double* circle3, int* masked, double* cx, double* cy, double* rad2) {
    *masked = circle3 && !(circle3[0] == -1.0 && circle3[1] == -1.0 && circle3[2] == -1.0);
    if (*masked) {
        SHG_REQUIRE(isfinite(circle3[0]) && isfinite(circle3[1]) && isfinite(circle3[2]), SHG_E_ARG, "%s: the circle (%g, %g, %g) is not finite",
                    fn, circle3[0], circle3[1], circle3[2]);
        *cx = circle3[0], *cy = circle3[1], *rad2 = circle3[2] * circle3[2];
    }
    return 0;
}

inline int zero_async(const char* fn, void* p, size_t bytes, hipStream_t st) {
    if (hipError_t e = hipMemsetAsync(p, 0, bytes, st)) {
        set_error("%s: %s", fn, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

}  // namespace shg
