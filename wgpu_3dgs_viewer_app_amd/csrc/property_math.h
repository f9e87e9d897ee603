// property_math.h — the arithmetic of the model properties (spec/RENDER_SPEC.md §17, "Model properties"), written once: the kernels
// of kernels_property.hip and the host restatement of tests/property_driver.cpp both include it, so the two cannot drift.
// It holds the value of a property from the stored words of a Gaussian (position and colour word; the dequantised covariance), the
// histogram's geometry for a run-time bin count (bounds_math.h's recipe restated: the bin of a value, the edge of a bin), the class
// of a value under a range (non-finite, below, above, a bin), the hit test of gsx_model_select_range, and the order-preserving
// integer key min / max are reduced in.  (The selection op on a word, prop_apply_op, is edit_math.h's: k_selection_op applies it too.)
// Plain float32 / integer arithmetic, <math.h> only besides export_math.h (ex_solve) and edit_math.h (em_rgb_to_hsv); no HIP
// include (the functions are __host__ __device__ under hipcc).  Built with -ffp-contract=off wherever it is included.
#pragma once
#include <math.h>
#include <stdint.h>

#include "export_math.h"

namespace gsx {

constexpr uint32_t kPropMaxBins = GSX_HIST_MAX_BINS;

GSX_HD inline bool prop_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN and +-inf
GSX_HD inline bool prop_is_position(uint32_t property) { return property <= (uint32_t)GSX_PROP_POS_Z; }
GSX_HD inline bool prop_is_scale(uint32_t property) { return property >= (uint32_t)GSX_PROP_SCALE_MAX && property < (uint32_t)GSX_PROP_COUNT; }

GSX_HD inline float prop_from_bits(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// The model transform of a GSX_PROP_WORLD position: gsx_model_merge's bake (kernels_merge.hip), p' = R (s * p) + t, each row
// ((R0 a0 + R1 a1) + R2 a2) + t in float32.  R: row-major, the float32 matrix the frame uses (quat_to_rows).
struct PropTransform {
    float R[9], s[3], t[3];
};
GSX_HD inline float prop_world_axis(const PropTransform& x, int axis, float px, float py, float pz) {
    const float sx = x.s[0] * px, sy = x.s[1] * py, sz = x.s[2] * pz;
    // (all three rows with constant indices, the result picked by compares: the transform stays in registers on the device)
    const float wx = ((x.R[0] * sx + x.R[1] * sy) + x.R[2] * sz) + x.t[0];
    const float wy = ((x.R[3] * sx + x.R[4] * sy) + x.R[5] * sz) + x.t[1];
    const float wz = ((x.R[6] * sx + x.R[7] * sy) + x.R[8] * sz) + x.t[2];
    return axis == 0 ? wx : (axis == 1 ? wy : wz);
}

// Properties 0..9 from the position + colour element (x, y, z bits and the rgba8 word).  world: apply `x` (never set for an
// identity transform: that gives the stored bits).
GSX_HD inline float prop_value_pc(uint32_t property, uint32_t wx, uint32_t wy, uint32_t wz, uint32_t color, bool world, const PropTransform& x) {
    if (property <= (uint32_t)GSX_PROP_POS_Z) {
        if (!world) return prop_from_bits(property == 0u ? wx : (property == 1u ? wy : wz));
        return prop_world_axis(x, (int)property, prop_from_bits(wx), prop_from_bits(wy), prop_from_bits(wz));
    }
    // the bytes of the colour word as ex_edited_color unpacks them
    const float r = (float)(color & 0xFFu) / 255.0f, g = (float)((color >> 8) & 0xFFu) / 255.0f, b = (float)((color >> 16) & 0xFFu) / 255.0f;
    switch (property) {
        case GSX_PROP_RED: return r;
        case GSX_PROP_GREEN: return g;
        case GSX_PROP_BLUE: return b;
        case GSX_PROP_OPACITY: return (float)(color >> 24) / 255.0f;
        default: break;
    }
    float h, s, v;
    em_rgb_to_hsv(r, g, b, h, s, v);
    return property == (uint32_t)GSX_PROP_HUE ? h : (property == (uint32_t)GSX_PROP_SATURATION ? s : v);
}

// Properties 10..12 from the exactly dequantised covariance (xx, xy, xz, yy, yz, zz): the scale gsx_model_export writes.
GSX_HD inline float prop_value_scale(uint32_t property, const float c[6]) {
    float rot[4], scale[3];
    ex_solve<ExportReal>(c, rot, scale);
    return property == (uint32_t)GSX_PROP_SCALE_MAX ? scale[0] : (property == (uint32_t)GSX_PROP_SCALE_MID ? scale[1] : scale[2]);
}

// ---- min / max ------------------------------------------------------------------------------------------------------------------------
// A float32 as an unsigned key of the same order (-inf < ... < -0 < +0 < ... < +inf): integer min / max of keys are exact and give
// the same bits in any order of combination.
GSX_HD inline uint32_t prop_key(float v) {
    const uint32_t u = ex_bits(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
GSX_HD inline float prop_unkey(uint32_t k) { return prop_from_bits((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
constexpr uint32_t kPropKeyMinIdentity = 0xFFFFFFFFu, kPropKeyMaxIdentity = 0u;

// ---- bins -----------------------------------------------------------------------------------------------------------------------------
// `bins` equal bins over [lo, hi]: bounds_math.h's BoundsAxis with the bin count a run-time value.  `live` is false for a range
// that has no usable bins — zero or not a finite float32, or so small that range / bins is 0 or bins / range is not finite — and
// every in-range value then lies in bin 0.
struct PropRange {
    float lo, hi, width, scale;
    uint32_t bins;
    bool live;
};
GSX_HD inline PropRange prop_range(float lo, float hi, uint32_t bins) {
    PropRange a;
    a.lo = lo;
    a.hi = hi;
    a.bins = bins ? bins : 1u;
    const float range = hi - lo, fb = (float)a.bins;
    a.live = range > 0.0f && prop_finite(range) && range / fb > 0.0f && prop_finite(fb / range);
    a.width = a.live ? range / fb : 0.0f;
    a.scale = a.live ? fb / range : 0.0f;
    return a;
}
// Lower edge of bin b; edge(0) = lo and edge(bins) = hi exactly, never decreasing in b.
GSX_HD inline float prop_edge(const PropRange& a, uint32_t b) {
    if (b == 0) return a.lo;
    if (b >= a.bins) return a.hi;
    return fminf(a.hi, a.lo + (float)b * a.width);
}
// The bin of a value lo <= v <= hi: the b with edge(b) <= v <= edge(b + 1), the estimate floor((v - lo) * scale) moved until both
// hold; 0 when the range is not live.
GSX_HD inline uint32_t prop_bin(const PropRange& a, float v) {
    if (!a.live) return 0u;
    const float t = (v - a.lo) * a.scale;
    uint32_t b = t >= (float)(a.bins - 1u) ? a.bins - 1u : (t > 0.0f ? (uint32_t)t : 0u);
    while (b > 0 && v < prop_edge(a, b)) --b;
    while (b + 1 < a.bins && v > prop_edge(a, b + 1)) ++b;
    return b;
}

// The class of a value under a range: a bin, or one of three codes above every bin.
constexpr uint32_t kPropNonfinite = 0xFFFFFFFFu, kPropBelow = 0xFFFFFFFEu, kPropAbove = 0xFFFFFFFDu;
GSX_HD inline uint32_t prop_classify(const PropRange& a, float v) {
    if (!prop_finite(v)) return kPropNonfinite;
    if (v < a.lo) return kPropBelow;
    if (v > a.hi) return kPropAbove;
    return prop_bin(a, v);
}
// gsx_model_select_range: is a value that passed the filter hit?  use_bins: the bin must lie in [bin_lo, bin_hi] as well.
GSX_HD inline bool prop_hit(const PropRange& a, float v, bool use_bins, uint32_t bin_lo, uint32_t bin_hi) {
    const uint32_t c = prop_classify(a, v);
    if (c >= kPropAbove) return false;
    return !use_bins || (c >= bin_lo && c <= bin_hi);
}

}  // namespace gsx
