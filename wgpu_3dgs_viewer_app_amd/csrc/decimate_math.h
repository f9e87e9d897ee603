// decimate_math.h — the arithmetic of gsx_model_decimate (spec/RENDER_SPEC.md §22, "Model decimate"), written once: the kernels of
// kernels_decimate.hip, the host side of gsx_api_decimate.cpp and the host restatement of tests/decimate_driver.cpp all include it, so
// they cannot drift.  It holds the grid of an edge (the cell function itself is neighbors_math.h's nb_cell: the ONLY copy), the key a
// cell's members are ordered by, what one member contributes to its cell's sums (dec_member), the one accumulation step (dec_acc) and
// the moment-matched Gaussian of the finished sums (dec_finish, dec_sh).
// float32 throughout, every operation rounded (built with -ffp-contract=off wherever it is included); the divide and the square root
// are the correctly rounded ones gsx_model_export's scale solve relies on (export_math.h).  <math.h> only; no HIP include (the
// functions are __host__ __device__ under hipcc).
//
// The columns of a cell's sums, one lane each in k_dec_merge: 0 W | 1..3 S1 | 4..9 S2 (xx xy xz yy yz zz) | 10..12 C (r g b) |
// 13..57 H (the 45 SH floats).  A member's value in column 0 is 1, so W is the sum of the weights like every other column; with mass
// weights W IS M, the same additions in the same order.
#pragma once
#include <math.h>
#include <stdint.h>

#include "neighbors_math.h"

namespace gsx {

constexpr uint32_t kDecGeo = 13u;          // the columns in front of the SH floats
constexpr uint32_t kDecColumns = 58u;      // all of them: they fit the 64 lanes of a wave
constexpr uint32_t kDecRankBucket = 64u;   // a bucket of at most this many records is ordered by counting, one lane a record
constexpr uint32_t kDecLdsBucket = 2048u;  // ... of at most this many in LDS by one workgroup; a larger one in global memory
constexpr uint32_t kDecNoCell = 0xFFFFFFFFu;  // out_map of a Gaussian that does not participate
constexpr uint32_t kDecEdgeSteps = 20u;    // gsx_model_decimate_edge's bisection

// Is the edge one a call accepts?  finite, above 0, its float32 reciprocal finite and above 0
inline bool dec_cell_ok(float cell) {
    const float inv_h = 1.0f / cell;
    return nb_finite(cell) && cell > 0.0f && nb_finite(inv_h) && inv_h > 0.0f;
}
// The grid of an edge: nb_grid's counterpart, the edge given instead of a radius.
struct DecGrid {
    float h, inv_h;
};
inline DecGrid dec_grid(float cell) {
    DecGrid g;
    g.h = cell;
    g.inv_h = 1.0f / cell;
    return g;
}
// The probes of gsx_model_decimate_edge: the ends of the bracket for an extent, and the midpoint in log2(edge) of two edges (the
// square root of their product, in double: correctly rounded, so every restatement lands on the same float32).
inline double dec_edge_lo(float extent) { return (double)extent / 32767.0; }
inline double dec_edge_hi(float extent) { return (double)extent * (1.0 + 1.0 / 32.0); }
inline double dec_edge_mid(double lo, double hi) { return sqrt(lo * hi); }
// The bisection itself: kDecEdgeSteps count-only probes.  count(edge, &cells) returns 0 or a status, which ends the search.  The
// high end of the bracket gives one cell by construction (every u is below 1) and counts as probed.  An extent of 0, or one whose
// bracket holds no edge a call accepts, gives edge 1 and one cell; a probe that is no such edge counts as too fine.
template <class Count>
inline int dec_find_edge(float extent, uint64_t target, Count&& count, float* out_cell, uint64_t* out_cells) {
    *out_cell = 1.0f;
    *out_cells = 1;
    double lo = dec_edge_lo(extent), hi = dec_edge_hi(extent);
    if (!(extent > 0.0f) || !dec_cell_ok((float)hi)) return 0;
    *out_cell = (float)hi;
    for (uint32_t step = 0; step < kDecEdgeSteps; ++step) {
        const double mid = dec_edge_mid(lo, hi);
        const float edge = (float)mid;
        uint64_t cells = 0;
        bool fits = false;
        if (dec_cell_ok(edge)) {
            const int st = count(edge, &cells);
            if (st) return st;
            fits = cells <= target;
        }
        if (fits) {
            hi = mid;
            *out_cell = edge;
            *out_cells = cells;
        } else {
            lo = mid;
        }
    }
    return 0;
}

// the 45 bits a cell's members share: cells are at most kNbMaxCell = 2^15 - 1 per axis
GSX_NB_HD inline uint64_t dec_cell_key(uint32_t cx, uint32_t cy, uint32_t cz) { return (uint64_t)cx | ((uint64_t)cy << 15) | ((uint64_t)cz << 30); }

// det of the symmetric c = (xx, xy, xz, yy, yz, zz)
GSX_NB_HD inline float dec_det(const float c[6]) {
    const float xx = c[0], xy = c[1], xz = c[2], yy = c[3], yz = c[4], zz = c[5];
    return (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz);
}

// One member: position p, covariance c and colour word (r | g << 8 | b << 16 | a << 24) exactly dequantised, p_r its cell's
// representative.  v[0 .. 12] are its values in the columns in front of the SH floats; returns its mass m = alpha * sqrt(det), *a its
// opacity byte.
GSX_NB_HD inline float dec_member(const float p[3], const float pr[3], const float c[6], uint32_t color, float v[13], uint32_t* a) {
    *a = color >> 24;
    const float alpha = (float)*a / 255.0f;
    const float det = dec_det(c);
    const float vol = (det > 0.0f && nb_finite(det)) ? sqrtf(det) : 0.0f;
    const float d0 = p[0] - pr[0], d1 = p[1] - pr[1], d2 = p[2] - pr[2];
    v[0] = 1.0f;
    v[1] = d0; v[2] = d1; v[3] = d2;
    v[4] = c[0] + d0 * d0; v[5] = c[1] + d0 * d1; v[6] = c[2] + d0 * d2;
    v[7] = c[3] + d1 * d1; v[8] = c[4] + d1 * d2; v[9] = c[5] + d2 * d2;
    v[10] = (float)(color & 0xFFu); v[11] = (float)((color >> 8) & 0xFFu); v[12] = (float)((color >> 16) & 0xFFu);
    return alpha * vol;
}

// One step of a column's sum, members in ascending index: the weight times the value, rounded, then the addition, rounded.  The
// uniform fallback passes w = 1 (the product is then the value itself).
GSX_NB_HD inline float dec_acc(float acc, float w, float v) { return acc + w * v; }

// Are the mass weights in use?  Otherwise every member weighs 1.
GSX_NB_HD inline bool dec_mass(float M) { return M > 0.0f && nb_finite(M); }

GSX_NB_HD inline uint32_t dec_byte(float x) {  // clamp(x, 0, 255) of an integral or non-finite x (NaN: 0)
    return (uint32_t)fminf(fmaxf(x, 0.0f), 255.0f);
}

// The merged Gaussian from the sums g[0 .. 12] of the weights in use (g[0] = W): mean, covariance (unquantised) and colour word;
// M is the mass sum, max_a the largest opacity byte of the members.  *inv_out = 1 / W, for dec_sh.
GSX_NB_HD inline void dec_finish(const float g[13], bool mass, float M, uint32_t max_a, const float pr[3], float mu[3], float cov[6], uint32_t* color,
                                 float* inv_out, float* alpha_out = nullptr) {
    const float inv = 1.0f / g[0];
    const float e0 = g[1] * inv, e1 = g[2] * inv, e2 = g[3] * inv;
    mu[0] = pr[0] + e0; mu[1] = pr[1] + e1; mu[2] = pr[2] + e2;
    cov[0] = g[4] * inv - e0 * e0; cov[1] = g[5] * inv - e0 * e1; cov[2] = g[6] * inv - e0 * e2;
    cov[3] = g[7] * inv - e1 * e1; cov[4] = g[8] * inv - e1 * e2; cov[5] = g[9] * inv - e2 * e2;
    const uint32_t r = dec_byte(floorf(g[10] * inv + 0.5f)), gg = dec_byte(floorf(g[11] * inv + 0.5f)), b = dec_byte(floorf(g[12] * inv + 0.5f));
    const float det = dec_det(cov);
    const float alpha = (mass && det > 0.0f && nb_finite(det)) ? fminf(1.0f, M / sqrtf(det)) : (float)max_a / 255.0f;
    const uint32_t a = dec_byte(floorf(alpha * 255.0f + 0.5f));
    *color = r | (gg << 8) | (b << 16) | (a << 24);
    *inv_out = inv;
    if (alpha_out) *alpha_out = alpha;  // (before the byte: the tests' tolerance is on it)
}
GSX_NB_HD inline float dec_sh(float H, float inv) { return H * inv; }

}  // namespace gsx
