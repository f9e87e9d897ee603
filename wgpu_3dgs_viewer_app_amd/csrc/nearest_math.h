// nearest_math.h — the rules of the nearest search across models (spec/RENDER_SPEC.md §23, "Model nearest (across models)"), written
// once: the kernels of kernels_nearest.hip, the host side of gsx_api_nearest.cpp, radius_search.h (the order in which the cap, the
// round's radius and the final round are applied: the library's loop, which tests/nearest_driver.cpp runs too) and the driver's host
// version of the work all include it, so they cannot drift.  It holds the mapping of a query into the targets' space, the order among candidates (d2,
// then the smaller target index), the cap that max_distance puts on d2, the radius of a round under that cap, and the matrix between
// two model transforms.  The distance, the cells (nb_cell_signed) and the grid are neighbors_math.h's, the radii and the rule that
// goes to the exact fallback knn_math.h's, the unit quaternion merge_math.h's; nothing of them is restated here.
// Plain float32 / double arithmetic, <math.h> only; no HIP include.  Built with -ffp-contract=off wherever it is included.
//
// Why a round is exact.  A query q walks the 27 cells around its own signed cell (neighbors_grid.h proves, also below the origin,
// that every target with d2(q, t) <= r2 lies in them) and sees each such target once (the own-cell test).  It keeps the least (d2,
// index) among the candidates with d2 <= e2 = min(r2, cap2).  If that best d2 is <= e2, every target with a d2 at or below it — every
// tie included — is among the candidates it saw: the pair is the answer.  If it kept nothing, no target lies within e2: where r2 >=
// cap2 (the round is final) that is the answer "none", otherwise the query stays unresolved.
#pragma once
#include <math.h>
#include <stdint.h>

#include "knn_math.h"
#include "merge_math.h"
#include "neighbors_math.h"

namespace gsx {

constexpr uint32_t kNearestNone = 0xFFFFFFFFu;        // GSX_NEAREST_NONE
constexpr uint32_t kNearestModelTransforms = 1u;      // GSX_NEAREST_MODEL_TRANSFORMS
constexpr uint32_t kNearestSelectRange = 0u;          // GSX_NEAREST_SELECT_RANGE
constexpr uint32_t kNearestSelectTransfer = 1u;       // GSX_NEAREST_SELECT_TRANSFER
constexpr float kNearestUnlimited = 3.402823466e+38f;  // the cap on d2 without a max_distance: a d2 that overflowed is out of reach

// One row of the 3x4 matrix applied to a stored position: ((m0 x + m1 y) + m2 z) + m3, every operation rounded to float32.
GSX_NB_HD inline float nearest_map_row(const float* m, float x, float y, float z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }

// Does the candidate (d2, index) come before the best so far?  The smaller d2, among equal d2 the smaller target index.
GSX_NB_HD inline bool nearest_better(float d2, uint32_t index, float best_d2, uint32_t best_index) {
    return d2 < best_d2 || (d2 == best_d2 && index < best_index);
}

// The cap on d2: fl(max * max), or the largest float32 where max_distance is 0 (unlimited).
inline float nearest_cap2(float max_distance) { return max_distance > 0.0f ? max_distance * max_distance : kNearestUnlimited; }
// Is max_distance one a call accepts?  0, or a radius gsx_model_neighbors accepts.
inline bool nearest_max_ok(float max_distance) { return max_distance == 0.0f || nb_radius_ok(max_distance); }
// What a round at r2 under the cap admits, and whether that round leaves nothing to a later one.
GSX_NB_HD inline float nearest_reach2(float r2, float cap2) { return r2 < cap2 ? r2 : cap2; }
inline bool nearest_final(float r2, float cap2) { return r2 >= cap2; }
// The radius of the round to come: `r` (the clamped first radius, or knn_next_radius of the last), but exactly max_distance where r
// is beyond it and the grid may run there (not below the floor, inside the radii a search uses).  A round at a radius at or beyond
// max_distance is final either way.
inline float nearest_round_radius(float r, float floor_, float max_distance) {
    if (max_distance > 0.0f && r > max_distance && max_distance >= floor_ && max_distance >= kKnnMinRadius && max_distance <= kKnnMaxRadius) return max_distance;
    return r;
}

// The rotation matrix of a unit quaternion (x, y, z, w), row-major, in double.
inline void nearest_quat_rows(const double q[4], double r[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    r[0] = 1.0 - 2.0 * (y * y + z * z); r[1] = 2.0 * (x * y - w * z); r[2] = 2.0 * (x * z + w * y);
    r[3] = 2.0 * (x * y + w * z); r[4] = 1.0 - 2.0 * (x * x + z * z); r[5] = 2.0 * (y * z - w * x);
    r[6] = 2.0 * (x * z - w * y); r[7] = 2.0 * (y * z + w * x); r[8] = 1.0 - 2.0 * (x * x + y * y);
}
// inv(M_dst) M_src with M = T R S (spec section 13), in double, rounded to float32 once: A = S_d^-1 R_d^T R_s S_s, b = S_d^-1 R_d^T
// (t_s - t_d).  The destination's scale components are not 0 and both quaternions not zero (the caller checks).
inline void nearest_model_matrix(const float pos_s[3], const float quat_s[4], const float scale_s[3], const float pos_d[3], const float quat_d[4],
                                 const float scale_d[3], float out[12]) {
    double qs[4], qd[4], Rs[9], Rd[9];
    merge_unit_quat(quat_s, qs);
    merge_unit_quat(quat_d, qd);
    nearest_quat_rows(qs, Rs);
    nearest_quat_rows(qd, Rd);
    for (int r = 0; r < 3; ++r) {
        const double inv = 1.0 / (double)scale_d[r];
        for (int c = 0; c < 3; ++c) {
            double a = 0.0;
            for (int k = 0; k < 3; ++k) a += Rd[3 * k + r] * Rs[3 * k + c];
            out[4 * r + c] = (float)(inv * a * (double)scale_s[c]);
        }
        double b = 0.0;
        for (int k = 0; k < 3; ++k) b += Rd[3 * k + r] * ((double)pos_s[k] - (double)pos_d[k]);
        out[4 * r + 3] = (float)(inv * b);
    }
}

}  // namespace gsx
