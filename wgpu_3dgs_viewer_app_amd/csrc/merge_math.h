// merge_math.h — the arithmetic of gsx_model_merge (spec/RENDER_SPEC.md §13, "Model merge") that the host, the kernels and the
// sanitized host driver tests/merge_driver.cpp share, written once:
//   * the identity test of a model transform (an identity source travels as stored bits);
//   * the bit address of a destination Gaussian in the `edited` plane when a source lands at an offset that is no multiple of 32
//     (two sources then share the word at their joint);
//   * the float64 construction of the three SH rotation matrices (3x3, 5x5, 7x7) of a unit quaternion — host only.
// No HIP include (the integer functions are __host__ __device__ under hipcc).
#pragma once
#include <math.h>
#include <stdint.h>

#include "extract_math.h"

namespace gsx {

constexpr uint32_t kMergeMaxSources = 64;  // GSX_MERGE_MAX_SOURCES (gsx.h)
// the matrices of bands 1, 2, 3, row-major, one behind the other: 9 + 25 + 49 floats
constexpr int kMergeShFloats = 83;
constexpr int kMergeBandCoeff[3] = {0, 3, 8};   // first SH coefficient of band l (coefficient 0 = the first of degree 1)
constexpr int kMergeBandSize[3] = {3, 5, 7};
constexpr int kMergeBandMatrix[3] = {0, 9, 34};  // where band l's matrix starts

// ---- identity -------------------------------------------------------------------------------------------------------------------
// pos 0, scale 1 and quat (0, 0, 0, 1) or (0, 0, 0, -1), compared as float32 values (so -0 is 0): exactly the transforms under which
// p' = R(s * p) + t, the covariance and the SH rotation are the identity in float32 AND for which nothing needs computing.
inline bool merge_is_identity(const float pos[3], const float quat[4], const float scale[3]) {
    for (int k = 0; k < 3; ++k)
        if (pos[k] != 0.0f || scale[k] != 1.0f || quat[k] != 0.0f) return false;
    return quat[3] == 1.0f || quat[3] == -1.0f;
}
// every component finite and the quaternion not zero (its float64 norm can be taken and divided by)
inline bool merge_is_valid(const float pos[3], const float quat[4], const float scale[3]) {
    for (int k = 0; k < 3; ++k)
        if (!isfinite(pos[k]) || !isfinite(scale[k])) return false;
    double nn = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (!isfinite(quat[k])) return false;
        nn += (double)quat[k] * (double)quat[k];
    }
    return nn > 0.0;
}

// ---- the joint word ---------------------------------------------------------------------------------------------------------------
// Gaussian j of a source whose kept Gaussians start at dst index `off`: the word and the bit of dst's `edited` plane.  The plane
// cannot be addressed through a pointer offset as the 16-byte planes are: off is generally no multiple of 32.
GSX_EX_HD inline uint64_t merge_bit_word(uint64_t off, uint64_t j) { return (off + j) >> 5; }
GSX_EX_HD inline uint32_t merge_bit_mask(uint64_t off, uint64_t j) { return 1u << (uint32_t)((off + j) & 31u); }
// does the source that starts at `off` share its first word with the source before it?
GSX_EX_HD inline bool merge_joint_shared(uint64_t off) { return (off & 31u) != 0u; }

// ---- SH rotation (host, float64) --------------------------------------------------------------------------------------------------
// the 15 basis functions of degrees 1..3 at a unit direction, with spec §4.9's constants and signs (project_math.h: pm_color)
inline void merge_sh_basis(const double d[3], double Y[15]) {
    const double C1 = 0.4886025119029199;
    const double C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
    const double C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                          1.445305721320277, -0.5900435899266435};
    const double x = d[0], y = d[1], z = d[2], xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    Y[0] = -C1 * y;
    Y[1] = C1 * z;
    Y[2] = -C1 * x;
    Y[3] = C2[0] * xy;
    Y[4] = C2[1] * yz;
    Y[5] = C2[2] * (2.0 * zz - xx - yy);
    Y[6] = C2[3] * xz;
    Y[7] = C2[4] * (xx - yy);
    Y[8] = C3[0] * y * (3.0 * xx - yy);
    Y[9] = C3[1] * xy * z;
    Y[10] = C3[2] * y * (4.0 * zz - xx - yy);
    Y[11] = C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
    Y[12] = C3[4] * x * (4.0 * zz - xx - yy);
    Y[13] = C3[5] * z * (xx - yy);
    Y[14] = C3[6] * x * (xx - 3.0 * yy);
}

// rotation matrix (row-major) of a UNIT quaternion x, y, z, w
inline void merge_quat_matrix(const double q[4], double R[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// The matrices M_l with c' = M_l c per band and channel such that  sum_k c'_k Y_k(R d) = sum_k c_k Y_k(d)  for every unit d.
// With y_i = Y(d_i) and z_i = Y(R d_i) over kMergeFitDirs fixed directions (a Fibonacci spiral: the normal matrix is close to a
// multiple of the identity), the property reads M^T z_i = y_i, so  (sum_i z_i z_i^T) M = sum_i z_i y_i^T,  solved per band by
// Gaussian elimination with partial pivoting.  Nothing is assumed about the basis (orthonormality, signs) beyond its closure under
// rotation.  q: unit quaternion.
constexpr int kMergeFitDirs = 48;
inline void merge_sh_matrices_f64(const double q[4], double out[kMergeShFloats]) {
    double R[9];
    merge_quat_matrix(q, R);
    double y[kMergeFitDirs][15], z[kMergeFitDirs][15];
    for (int i = 0; i < kMergeFitDirs; ++i) {
        const double h = 1.0 - (2.0 * i + 1.0) / kMergeFitDirs, r = sqrt(1.0 - h * h), phi = 2.399963229728653 * i;  // the golden angle
        const double d[3] = {r * cos(phi), r * sin(phi), h};
        const double rd[3] = {R[0] * d[0] + R[1] * d[1] + R[2] * d[2], R[3] * d[0] + R[4] * d[1] + R[5] * d[2],
                              R[6] * d[0] + R[7] * d[1] + R[8] * d[2]};
        merge_sh_basis(d, y[i]);
        merge_sh_basis(rd, z[i]);
    }
    for (int l = 0; l < 3; ++l) {
        const int m = kMergeBandSize[l], c0 = kMergeBandCoeff[l];
        double A[7][14];  // [ sum z z^T | sum z y^T ]
        for (int r = 0; r < m; ++r)
            for (int c = 0; c < m; ++c) {
                double g = 0.0, k = 0.0;
                for (int i = 0; i < kMergeFitDirs; ++i) {
                    g += z[i][c0 + r] * z[i][c0 + c];
                    k += z[i][c0 + r] * y[i][c0 + c];
                }
                A[r][c] = g;
                A[r][m + c] = k;
            }
        for (int p = 0; p < m; ++p) {
            int best = p;
            for (int r = p + 1; r < m; ++r)
                if (fabs(A[r][p]) > fabs(A[best][p])) best = r;
            for (int c = 0; c < 2 * m; ++c) {
                const double tmp = A[p][c];
                A[p][c] = A[best][c];
                A[best][c] = tmp;
            }
            for (int r = 0; r < m; ++r) {
                if (r == p) continue;
                const double f = A[r][p] / A[p][p];
                for (int c = p; c < 2 * m; ++c) A[r][c] -= f * A[p][c];
            }
        }
        for (int r = 0; r < m; ++r)
            for (int c = 0; c < m; ++c) out[kMergeBandMatrix[l] + r * m + c] = A[r][m + c] / A[r][r];
    }
}

// a model quaternion (merge_is_valid) normalised in float64
inline void merge_unit_quat(const float quat[4], double q[4]) {
    double nn = 0.0;
    for (int k = 0; k < 4; ++k) nn += (double)quat[k] * (double)quat[k];
    const double inv = 1.0 / sqrt(nn);
    for (int k = 0; k < 4; ++k) q[k] = (double)quat[k] * inv;
}

// what the host hands the kernel: the quaternion normalised in float64, the matrices rounded to float32
inline void merge_sh_matrices(const float quat[4], float out[kMergeShFloats]) {
    double q[4], M[kMergeShFloats];
    merge_unit_quat(quat, q);
    merge_sh_matrices_f64(q, M);
    for (int k = 0; k < kMergeShFloats; ++k) out[k] = (float)M[k];
}

}  // namespace gsx
