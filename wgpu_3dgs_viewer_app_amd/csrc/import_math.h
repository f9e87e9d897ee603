// import_math.h — the arithmetic of gsx_model_import_ply (spec/RENDER_SPEC.md §15, "PLY import") that the kernel
// (kernels_import.hip) and the sanitized host driver tests/import_driver.cpp share, written once:
//   * the checks of a caller's gsx_ply_header before a row is read;
//   * the property fetch of one binary row: by name through the header's offsets, 4 bytes little-endian each, assembled from bytes
//     (any offset) or taken as whole words (a row whose stride and offsets are multiples of 4);
//   * the row -> gsx_gaussian step: rot normalised in float32 as gsx_ply_read_gaussians does, the colour bytes in float32, scale and
//     alpha through the float64 exponential rounded once — defined without reference to any libm's float32 expf.
// The library is built with -ffp-contract=off.  No HIP include (the functions are __host__ __device__ under hipcc).
#pragma once
#include <math.h>
#include <stdint.h>

#include "edit_math.h"

namespace gsx {

#if defined(__HIPCC__)
#define GSX_IM_UNROLL _Pragma("unroll")
#else
#define GSX_IM_UNROLL
#endif

constexpr int kImportProps = 62;              // the INRIA properties, in gsx_ply_header::offsets order
constexpr uint32_t kImportMaxStride = 1024;   // the largest vertex_bytes the device path takes
constexpr uint32_t kImportCanonicalStride = 248;
constexpr float kImportShC0 = 0.28209479177387814f;
// property indices of a row (gsx_ply.cpp: kProps)
enum { IMP_X = 0, IMP_FDC = 6, IMP_REST = 9, IMP_OPACITY = 54, IMP_SCALE = 55, IMP_ROT = 58 };
constexpr int kImportRequired[14] = {0, 1, 2, 6, 7, 8, 54, 55, 56, 57, 58, 59, 60, 61};

// what a kernel needs of a gsx_ply_header, passed by value
struct ImportLayout {
    uint32_t stride;
    int32_t off[kImportProps];  // byte offset inside a row, -1: absent (reads as 0.0f)
};

// the verdict on a caller's header: 0 fine, 1 unsupported (ascii, or a stride above kImportMaxStride), 2 invalid (a zero stride, an
// offset that is neither -1 nor inside the row, a required property absent).  *bad: the property that fails (or -1)
GSX_HD inline int im_check_header(const gsx_ply_header& h, int* bad) {
    *bad = -1;
    if (h.is_ascii) return 1;
    if (h.vertex_bytes > kImportMaxStride) return 1;
    if (h.vertex_bytes == 0) return 2;
    for (int k = 0; k < kImportProps; ++k) {
        const int32_t o = h.offsets[k];
        if (o == -1) continue;
        if (o < 0 || (uint32_t)o > h.vertex_bytes || (uint32_t)o + 4u > h.vertex_bytes) {
            *bad = k;
            return 2;
        }
    }
    for (int r = 0; r < 14; ++r)
        if (h.offsets[kImportRequired[r]] < 0) {
            *bad = kImportRequired[r];
            return 2;
        }
    return 0;
}

GSX_HD inline ImportLayout im_layout(const gsx_ply_header& h) {
    ImportLayout l;
    l.stride = h.vertex_bytes;
    for (int k = 0; k < kImportProps; ++k) l.off[k] = h.offsets[k];
    return l;
}

// stride 248 and property k at byte 4 k: what the INRIA trainer, gsx_ply_write and gsx_model_export_ply write
GSX_HD inline bool im_is_canonical(const ImportLayout& l) {
    if (l.stride != kImportCanonicalStride) return false;
    for (int k = 0; k < kImportProps; ++k)
        if (l.off[k] != 4 * k) return false;
    return true;
}

// may every property be fetched as one aligned word (from a 4-byte aligned first row)?
GSX_HD inline bool im_is_word_aligned(const ImportLayout& l) {
    if (l.stride & 3u) return false;
    for (int k = 0; k < kImportProps; ++k)
        if (l.off[k] >= 0 && (l.off[k] & 3)) return false;
    return true;
}

GSX_HD inline float im_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// the 62 properties of one row, from its bytes
GSX_HD inline void im_fetch_bytes(const uint8_t* row, const ImportLayout& l, float v[kImportProps]) {
    GSX_IM_UNROLL
    for (int k = 0; k < kImportProps; ++k) {
        const int32_t o = l.off[k];
        uint32_t u = 0u;
        if (o >= 0) u = (uint32_t)row[o] | ((uint32_t)row[o + 1] << 8) | ((uint32_t)row[o + 2] << 16) | ((uint32_t)row[o + 3] << 24);
        v[k] = im_float(u);
    }
}

// ... from its words (im_is_word_aligned; row is 4-byte aligned)
GSX_HD inline void im_fetch_words(const uint32_t* row, const ImportLayout& l, float v[kImportProps]) {
    GSX_IM_UNROLL
    for (int k = 0; k < kImportProps; ++k) {
        const int32_t o = l.off[k];
        v[k] = im_float(o >= 0 ? row[o >> 2] : 0u);
    }
}

// floor(clamp(t, 0, 1) * 255 + 0.5): a NaN gives 0 (fmaxf returns the other operand)
GSX_HD inline uint8_t im_unorm8(float t) { return (uint8_t)floorf(fminf(fmaxf(t, 0.0f), 1.0f) * 255.0f + 0.5f); }

// the float64 exponential of a float32, rounded once: +inf -> inf, -inf -> 0, NaN -> NaN
GSX_HD inline float im_exp(float v) { return (float)exp((double)v); }

// sigmoid in float64, then the byte: a NaN gives 0
GSX_HD inline uint8_t im_alpha(float o) {
    const double a = 1.0 / (1.0 + exp(-(double)o));
    return (uint8_t)floor(fmin(fmax(a, 0.0), 1.0) * 255.0 + 0.5);
}

// gs::Gaussian::from(PlyGaussianPod), with §15's roundings: v holds the 62 properties in header order
GSX_HD inline void im_row_to_gaussian(const float v[kImportProps], gsx_gaussian* g) {
    float w = v[IMP_ROT], x = v[IMP_ROT + 1], y = v[IMP_ROT + 2], z = v[IMP_ROT + 3];
    const float len = sqrtf(((w * w + x * x) + y * y) + z * z);
    if (!(len > 0.0f)) {
        g->rot[0] = 0.0f; g->rot[1] = 0.0f; g->rot[2] = 0.0f; g->rot[3] = 1.0f;
    } else {
        g->rot[0] = x / len; g->rot[1] = y / len; g->rot[2] = z / len; g->rot[3] = w / len;
    }
    for (int k = 0; k < 3; ++k) {
        g->pos[k] = v[IMP_X + k];
        g->scale[k] = im_exp(v[IMP_SCALE + k]);
        g->color[k] = im_unorm8(0.5f + kImportShC0 * v[IMP_FDC + k]);
    }
    g->color[3] = im_alpha(v[IMP_OPACITY]);
    GSX_IM_UNROLL
    for (int c = 0; c < 15; ++c)
        GSX_IM_UNROLL
        for (int ch = 0; ch < 3; ++ch) g->sh[c][ch] = v[IMP_REST + ch * 15 + c];  // channel-major on disk
}

}  // namespace gsx
