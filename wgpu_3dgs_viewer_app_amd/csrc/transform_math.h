// transform_math.h — the arithmetic of gsx_model_apply_transform (spec/RENDER_SPEC.md §21, "Model transform") that the host, the
// kernel (kernels_transform.hip) and the sanitized host driver tests/transform_driver.cpp share, written once:
//   * the mode of a transform: which planes a call has to rewrite (a plane that is not rewritten keeps its stored bits);
//   * the position formula with its pivot rule;
//   * the validity test (merge_is_valid, extended to the pivot).
// The SH matrices are merge_math.h's (merge_sh_matrices); the float32 rotation matrix is quat_to_rows of the quaternion as given.
// No HIP include (the position formula is __host__ __device__ under hipcc).  Compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "merge_math.h"

namespace gsx {

// ---- mode -----------------------------------------------------------------------------------------------------------------------
// What a transform asks of the planes, from the float32 VALUES of its components (so -0 is 0):
//   identity     merge_is_identity: nothing is written, whatever the pivot;
//   translate    quat (0, 0, 0, +-1) and scale (1, 1, 1): positions only (pc.xyz and the record's position word);
//   no rotation  quat (0, 0, 0, +-1), another scale: positions and the covariance; the SH planes keep their bits;
//   full         every other quaternion — one that is the identity only after normalisation, (0, 0, 0, 2) say, among them: every
//                plane is rewritten, positions and covariances by the quat_to_rows matrix of the quaternion as given (which is no
//                rotation for a quaternion that is not of unit length), the SH by the matrices of the normalised quaternion.
enum : int { kTransformIdentity = 0, kTransformTranslate = 1, kTransformNoRotation = 2, kTransformFull = 3 };

inline bool transform_rotation_is_identity(const float quat[4]) {
    return quat[0] == 0.0f && quat[1] == 0.0f && quat[2] == 0.0f && (quat[3] == 1.0f || quat[3] == -1.0f);
}
inline int transform_mode(const float pos[3], const float quat[4], const float scale[3]) {
    if (merge_is_identity(pos, quat, scale)) return kTransformIdentity;
    if (!transform_rotation_is_identity(quat)) return kTransformFull;
    return (scale[0] == 1.0f && scale[1] == 1.0f && scale[2] == 1.0f) ? kTransformTranslate : kTransformNoRotation;
}

// ---- validity -------------------------------------------------------------------------------------------------------------------
inline bool transform_is_valid(const float pos[3], const float quat[4], const float scale[3], const float pivot[3]) {
    for (int k = 0; k < 3; ++k)
        if (!isfinite(pivot[k])) return false;
    return merge_is_valid(pos, quat, scale);
}
// exactly (0, 0, 0) as float32 values: the subtraction and the final addition of the position formula are then not performed
inline bool transform_pivot_is_zero(const float pivot[3]) { return pivot[0] == 0.0f && pivot[1] == 0.0f && pivot[2] == 0.0f; }

// ---- position -------------------------------------------------------------------------------------------------------------------
// p' = R (s * (p - c)) + t + c, every operation rounded to float32: q = p - c per axis, a = s * q, each row
// (((R_r0 a0 + R_r1 a1) + R_r2 a2) + t_r) + c_r.  Without a pivot (use_pivot false) q = p and the last addition is left out: §13's
// position bit for bit, signed zeros included.  A non-finite coordinate goes through the same operations.
GSX_EX_HD inline void transform_position(const float R[9], const float s[3], const float t[3], const float c[3], bool use_pivot, const float p[3],
                                         float out[3]) {
    float q0 = p[0], q1 = p[1], q2 = p[2];
    if (use_pivot) {
        q0 = p[0] - c[0];
        q1 = p[1] - c[1];
        q2 = p[2] - c[2];
    }
    const float a0 = s[0] * q0, a1 = s[1] * q1, a2 = s[2] * q2;
    for (int r = 0; r < 3; ++r) {
        float o = ((R[3 * r] * a0 + R[3 * r + 1] * a1) + R[3 * r + 2] * a2) + t[r];
        if (use_pivot) o = o + c[r];
        out[r] = o;
    }
}

}  // namespace gsx
