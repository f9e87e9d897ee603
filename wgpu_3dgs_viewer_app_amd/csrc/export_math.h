// export_math.h — the arithmetic of gsx_model_export (spec/RENDER_SPEC.md §14, "Model export") that the kernel
// (kernels_export.hip) and the sanitized host driver tests/export_driver.cpp share, written once:
//   * rotation and scale from a stored covariance: a cyclic Jacobi eigen-solve of the symmetric 3x3 with a FIXED number of sweeps
//     in a fixed pair order, the descending sort, the determinant fix, matrix -> quaternion, the canonical sign, the special cases;
//   * the colour of a row: the stored colour word, or spec §7 Export's arithmetic (edit_math.h: em_apply_edit) when edits are baked;
//   * the assembly of a gsx_gaussian record (56 words) and of an INRIA PLY row (62 words, gsx_ply.cpp: gaussian_to_vertex).
// float32 throughout (the library is built with -ffp-contract=off); the solve is a template over its scalar so that the float64
// variant of §14 exists next to it.  No HIP include (the functions are __host__ __device__ under hipcc).
#pragma once
#include <math.h>
#include <stdint.h>

#include "edit_math.h"

namespace gsx {

constexpr uint32_t kExportGaussianWords = 56;  // sizeof(gsx_gaussian) / 4
constexpr uint32_t kExportPlyWords = 62;       // the 62 float32 properties of gsx_ply_write
// Jacobi sweeps, each over the pairs (0,1), (0,2), (1,2).  Four give the errors of six, bit for bit in the worst case, on all four
// fixture families of tests/test_export_cpu.py (three do not: 29 x 2^-24 on the bench generator's scales); five leaves one in hand.
constexpr int kExportSweeps = 5;
constexpr float kExportShC0 = 0.28209479177387814f;
// word offsets of a gsx_gaussian record and of a PLY row
enum { EXG_ROT = 0, EXG_POS = 4, EXG_COLOR = 7, EXG_SH = 8, EXG_SCALE = 53 };
enum { EXP_X = 0, EXP_FDC = 6, EXP_REST = 9, EXP_OPACITY = 54, EXP_SCALE = 55, EXP_ROT = 58 };

#if defined(__HIPCC__)
#define GSX_EX_UNROLL _Pragma("unroll")
#else
#define GSX_EX_UNROLL
#endif

GSX_HD inline uint32_t ex_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

GSX_HD inline float ex_sqrt(float x) { return sqrtf(x); }
GSX_HD inline double ex_sqrt(double x) { return sqrt(x); }
GSX_HD inline float ex_abs(float x) { return fabsf(x); }
GSX_HD inline double ex_abs(double x) { return fabs(x); }

// One Jacobi rotation in the plane (P, Q) of the symmetric a, accumulated into the columns P and Q of v.  Skipped when a[P][Q] is
// zero, or so small beside a[Q][Q] - a[P][P] that theta^2 is not finite (the angle is then below every rounding that follows).
template <class T, int P, int Q>
GSX_HD inline void ex_rotate(T (&a)[3][3], T (&v)[3][3]) {
    constexpr int R = 3 - P - Q;
    const T apq = a[P][Q];
    const T theta = (a[Q][Q] - a[P][P]) / (apq + apq);
    const T th2 = theta * theta;
    if (!(apq != T(0) && th2 < T(INFINITY))) return;
    const T tt = T(1) / (ex_abs(theta) + ex_sqrt(th2 + T(1)));
    const T t = theta < T(0) ? -tt : tt;
    const T c = T(1) / ex_sqrt(t * t + T(1)), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = T(0);
    const T arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
    for (int k = 0; k < 3; ++k) {
        const T vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

template <class T, int P, int Q>
GSX_HD inline void ex_sort_pair(T (&l)[3], T (&v)[3][3]) {  // the larger eigenvalue first; equal ones keep their order
    if (l[P] < l[Q]) {
        const T tl = l[P];
        l[P] = l[Q];
        l[Q] = tl;
        for (int k = 0; k < 3; ++k) {
            const T tv = v[k][P];
            v[k][P] = v[k][Q];
            v[k][Q] = tv;
        }
    }
}

// a proper rotation matrix -> unit quaternion x, y, z, w with w >= 0 (w == 0: the first non-zero of x, y, z positive)
template <class T>
GSX_HD inline void ex_matrix_quat(const T (&m)[3][3], float rot[4]) {
    const T tr = m[0][0] + m[1][1] + m[2][2];
    T x, y, z, w;
    if (tr >= m[0][0] && tr >= m[1][1] && tr >= m[2][2]) {
        const T s = ex_sqrt(tr + T(1)) * T(2);
        w = s * T(0.25);
        x = (m[2][1] - m[1][2]) / s;
        y = (m[0][2] - m[2][0]) / s;
        z = (m[1][0] - m[0][1]) / s;
    } else if (m[0][0] >= m[1][1] && m[0][0] >= m[2][2]) {
        const T s = ex_sqrt(((T(1) + m[0][0]) - m[1][1]) - m[2][2]) * T(2);
        w = (m[2][1] - m[1][2]) / s;
        x = s * T(0.25);
        y = (m[0][1] + m[1][0]) / s;
        z = (m[0][2] + m[2][0]) / s;
    } else if (m[1][1] >= m[2][2]) {
        const T s = ex_sqrt(((T(1) + m[1][1]) - m[0][0]) - m[2][2]) * T(2);
        w = (m[0][2] - m[2][0]) / s;
        x = (m[0][1] + m[1][0]) / s;
        y = s * T(0.25);
        z = (m[1][2] + m[2][1]) / s;
    } else {
        const T s = ex_sqrt(((T(1) + m[2][2]) - m[0][0]) - m[1][1]) * T(2);
        w = (m[1][0] - m[0][1]) / s;
        x = (m[0][2] + m[2][0]) / s;
        y = (m[1][2] + m[2][1]) / s;
        z = s * T(0.25);
    }
    const T len = ex_sqrt(((x * x + y * y) + z * z) + w * w);
    x = x / len;
    y = y / len;
    z = z / len;
    w = w / len;
    const bool flip = w < T(0) || (w == T(0) && (x < T(0) || (x == T(0) && (y < T(0) || (y == T(0) && z < T(0))))));
    const T sg = flip ? T(-1) : T(1);
    rot[0] = (float)(sg * x);
    rot[1] = (float)(sg * y);
    rot[2] = (float)(sg * z);
    rot[3] = (float)(sg * w) + 0.0f;  // (-0 -> +0)
}

// rotation (x, y, z, w) and linear scales, scale[0] >= scale[1] >= scale[2], of the covariance c = (xx, xy, xz, yy, yz, zz), so
// that S = R diag(scale^2) R^T.  A non-finite entry: no solve, the identity rotation and the diagonal's roots.
template <class T>
GSX_HD inline void ex_solve(const float c[6], float rot[4], float scale[3]) {
    bool finite = true;
    for (int k = 0; k < 6; ++k) finite = finite && ex_abs(c[k]) < INFINITY;  // (false for NaN too)
    if (!finite) {
        rot[0] = rot[1] = rot[2] = 0.0f;
        rot[3] = 1.0f;
        scale[0] = sqrtf(fmaxf(c[0], 0.0f));
        scale[1] = sqrtf(fmaxf(c[3], 0.0f));
        scale[2] = sqrtf(fmaxf(c[5], 0.0f));
        return;
    }
    T a[3][3] = {{(T)c[0], (T)c[1], (T)c[2]}, {(T)c[1], (T)c[3], (T)c[4]}, {(T)c[2], (T)c[4], (T)c[5]}};
    T v[3][3] = {{T(1), T(0), T(0)}, {T(0), T(1), T(0)}, {T(0), T(0), T(1)}};
    for (int sweep = 0; sweep < kExportSweeps; ++sweep) {
        ex_rotate<T, 0, 1>(a, v);
        ex_rotate<T, 0, 2>(a, v);
        ex_rotate<T, 1, 2>(a, v);
    }
    T l[3] = {a[0][0], a[1][1], a[2][2]};
    ex_sort_pair<T, 0, 1>(l, v);
    ex_sort_pair<T, 1, 2>(l, v);
    ex_sort_pair<T, 0, 1>(l, v);
    const T det = (v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0])) +
                  v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    if (det < T(0))
        for (int k = 0; k < 3; ++k) v[k][2] = -v[k][2];
    ex_matrix_quat<T>(v, rot);
    for (int k = 0; k < 3; ++k) scale[k] = sqrtf(fmaxf((float)l[k], 0.0f));  // (an indefinite covariance: scale 0)
}

// the scalar the library solves in (§14: float32 meets the covariance bound)
typedef float ExportReal;

// ---- colour -------------------------------------------------------------------------------------------------------------------------
GSX_HD inline uint32_t ex_unorm8(float x) { return (uint32_t)floorf(em_clamp(x, 0.0f, 1.0f) * 255.0f + 0.5f); }
GSX_HD inline float ex_logit(float a) {
    a = fminf(fmaxf(a, 1e-6f), 1.0f - 1e-6f);
    return logf(a / (1.0f - a));
}
// the float colour of a stored colour word, edited by e (e.flag has ENABLED): spec §7 Export
GSX_HD inline void ex_edited_color(uint32_t word, const gsx_gaussian_edit& e, float& r, float& g, float& b, float& a) {
    r = (float)(word & 0xFFu) / 255.0f;
    g = (float)((word >> 8) & 0xFFu) / 255.0f;
    b = (float)((word >> 16) & 0xFFu) / 255.0f;
    a = (float)(word >> 24) / 255.0f;
    em_apply_edit(e, r, g, b, a);
}

// ---- rows ---------------------------------------------------------------------------------------------------------------------------
// pos: the stored bits; sh(f): the bits of dequantised SH float f = 3 * coefficient + channel (ExportShZero: an Sh None model);
// bake: e is the edit record to bake (its flag has ENABLED); otherwise e is not read
struct ExportShZero {
    GSX_HD uint32_t operator()(int) const { return 0u; }
};
struct ExportShWords {  // 45 words in memory order
    const uint32_t* w;
    GSX_HD uint32_t operator()(int f) const { return w[f]; }
};

template <class Sh>
GSX_HD inline void ex_row_gaussian(uint32_t* row, const uint32_t pos[3], uint32_t color, const Sh& sh, const float rot[4], const float scale[3],
                                   bool bake, const gsx_gaussian_edit& e) {
    for (int k = 0; k < 4; ++k) row[EXG_ROT + k] = ex_bits(rot[k]);
    for (int k = 0; k < 3; ++k) row[EXG_POS + k] = pos[k];
    if (bake) {
        float r, g, b, a;
        ex_edited_color(color, e, r, g, b, a);
        color = ex_unorm8(r) | (ex_unorm8(g) << 8) | (ex_unorm8(b) << 16) | (ex_unorm8(a) << 24);
    }
    row[EXG_COLOR] = color;
    GSX_EX_UNROLL
    for (int f = 0; f < 45; ++f) row[EXG_SH + f] = sh(f);
    for (int k = 0; k < 3; ++k) row[EXG_SCALE + k] = ex_bits(scale[k]);
}

template <class Sh>
GSX_HD inline void ex_row_ply(uint32_t* row, const uint32_t pos[3], uint32_t color, const Sh& sh, const float rot[4], const float scale[3],
                              bool bake, const gsx_gaussian_edit& e) {
    for (int k = 0; k < 3; ++k) {
        row[EXP_X + k] = pos[k];
        row[3 + k] = 0u;  // normals
    }
    float r, g, b, a;
    if (bake) {
        ex_edited_color(color, e, r, g, b, a);
    } else {
        r = (float)(color & 0xFFu) / 255.0f;
        g = (float)((color >> 8) & 0xFFu) / 255.0f;
        b = (float)((color >> 16) & 0xFFu) / 255.0f;
        a = (float)(color >> 24) / 255.0f;
    }
    row[EXP_FDC] = ex_bits((r - 0.5f) / kExportShC0);
    row[EXP_FDC + 1] = ex_bits((g - 0.5f) / kExportShC0);
    row[EXP_FDC + 2] = ex_bits((b - 0.5f) / kExportShC0);
    GSX_EX_UNROLL
    for (int c = 0; c < 15; ++c)
        GSX_EX_UNROLL
        for (int ch = 0; ch < 3; ++ch) row[EXP_REST + ch * 15 + c] = sh(3 * c + ch);  // channel-major on disk
    row[EXP_OPACITY] = ex_bits(ex_logit(a));
    for (int k = 0; k < 3; ++k) row[EXP_SCALE + k] = ex_bits(logf(scale[k]));  // (a zero scale: -inf, as gsx_ply_write)
    row[EXP_ROT] = ex_bits(rot[3]);
    for (int k = 0; k < 3; ++k) row[EXP_ROT + 1 + k] = ex_bits(rot[k]);
}

}  // namespace gsx
