// bounds_math.h — the arithmetic of gsx_model_bounds' trimmed box (spec/RENDER_SPEC.md §11, "Model bounds"), written once: the
// kernels of kernels_bounds.hip and the host restatement of tests/bounds_driver.cpp both include it, so the two cannot drift.
// It holds the histogram's geometry per axis (the bin of a value, the edge of a bin), the scan of a histogram for the bin where
// the cumulative count first exceeds k, and the result of a call that counted nothing.
// Plain float32 / integer arithmetic, <math.h> only; no HIP include (the functions are __host__ __device__ under hipcc).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GSX_BD_HD __host__ __device__
#else
#define GSX_BD_HD
#endif

namespace gsx {

constexpr uint32_t kBoundsBins = 2048;  // per axis, over [min, max] of the counted positions

GSX_BD_HD inline bool bounds_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN and +-inf

// One axis of the histogram: kBoundsBins equal bins over [lo, hi].  `live` is false for an axis that has no histogram — its range
// is zero or not a finite float32, or so small that range / bins is 0 or bins / range is not finite — and whose trimmed box is
// [lo, hi] itself.
struct BoundsAxis {
    float lo, hi, width, scale;  // width = (hi - lo) / bins; scale = bins / (hi - lo)
    bool live;
};
GSX_BD_HD inline BoundsAxis bounds_axis(float lo, float hi) {
    BoundsAxis a;
    a.lo = lo;
    a.hi = hi;
    const float range = hi - lo;
    // (a range so small that a bin's width underflows to 0, or the scale overflows, has no usable bins either)
    a.live = range > 0.0f && bounds_finite(range) && range / (float)kBoundsBins > 0.0f && bounds_finite((float)kBoundsBins / range);
    a.width = a.live ? range / (float)kBoundsBins : 0.0f;
    a.scale = a.live ? (float)kBoundsBins / range : 0.0f;
    return a;
}

// Lower edge of bin b; edge(0) = lo and edge(bins) = hi exactly, never decreasing in b.
GSX_BD_HD inline float bounds_edge(const BoundsAxis& a, uint32_t b) {
    if (b == 0) return a.lo;
    if (b >= kBoundsBins) return a.hi;
    return fminf(a.hi, a.lo + (float)b * a.width);
}

// The bin of a value lo <= v <= hi of a live axis: the b with edge(b) <= v <= edge(b + 1), decided against the edges as
// bounds_edge computes them — the estimate floor((v - lo) * scale) is moved until both hold (not at all, or by one bin, unless
// the range is a few thousand ulps of its ends).  So a value is never below the lower edge of its bin nor above the upper one,
// whatever the rounding, and that is all the trimmed box's guarantees rest on.
GSX_BD_HD inline uint32_t bounds_bin(const BoundsAxis& a, float v) {
    const float t = (v - a.lo) * a.scale;
    uint32_t b = t >= (float)(kBoundsBins - 1) ? kBoundsBins - 1 : (t > 0.0f ? (uint32_t)t : 0u);
    while (b > 0 && v < bounds_edge(a, b)) --b;
    while (b + 1 < kBoundsBins && v > bounds_edge(a, b + 1)) ++b;
    return b;
}

// Scan of n bins for the first whose cumulative count exceeds k: in ascending order of index (reverse = false) or descending
// (reverse = true).  Returns its position in scan order and, in *before, the count in front of it; n when the whole histogram
// holds no more than k.
GSX_BD_HD inline uint32_t bounds_scan(const uint32_t* hist, uint32_t n, bool reverse, uint64_t k, uint64_t* before) {
    uint64_t cum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = hist[reverse ? n - 1 - i : i];
        if (cum + c > k) {
            *before = cum;
            return i;
        }
        cum += c;
    }
    *before = cum;
    return n;
}

// k of spec §11: how many counted Gaussians the trimmed box may leave below it, and above it, per axis
GSX_BD_HD inline uint64_t bounds_trim_k(uint64_t count, uint32_t trim_permille) { return count * trim_permille / 1000u; }

// The trimmed ends of one axis from the scan positions of bounds_scan (kBoundsBins: nothing found): the lower edge of the bin the
// ascending scan stopped in, the upper edge of the bin the descending scan stopped in.  At most k counted values lie below the
// one and at most k above the other (bounds_bin), and each end is within one bin width of the k-th value from its side.
GSX_BD_HD inline float bounds_trim_lo(const BoundsAxis& a, uint32_t pos) { return a.live && pos < kBoundsBins ? bounds_edge(a, pos) : a.lo; }
GSX_BD_HD inline float bounds_trim_hi(const BoundsAxis& a, uint32_t pos) { return a.live && pos < kBoundsBins ? bounds_edge(a, kBoundsBins - pos) : a.hi; }

// What a call returns that counted nothing: every float field 0.0f (the two counts are the caller's).  `f` = the 18 floats of
// gsx_model_bounds_t from `min` on.
GSX_BD_HD inline void bounds_empty(float* f) {
    for (int i = 0; i < 18; ++i) f[i] = 0.0f;
}

}  // namespace gsx
