// normals_math.h — the rules of the model normals (spec/RENDER_SPEC.md §26, "Model normals"), written once: the kernels of
// kernels_normals.hip, the host side of gsx_api_normals.cpp and the host replay tests/normals_driver.cpp all include it, so they cannot
// drift.  It holds the neighbour list's key and the chain that keeps a lane's K smallest keys, the rule that proves a list, the rule
// that says whether a list can be fitted, the plane fit (offsets, mean, scatter, eigen-solve, normal, variation), the sign of the
// normal, and the select's two tests.  The distance, the cell and the grid are neighbors_math.h's (nb_d2: the ONLY copy); the radii and
// the fallback rule are knn_math.h's, applied by radius_search.h; the Jacobi rotation and the sort are export_math.h's templates,
// called here with double.  Plain float32 / double / integer arithmetic, <math.h> only; no HIP include.  Built with -ffp-contract=off
// wherever it is included.
//
// The key.  A neighbour is the pair (d2, j).  Every d2 is +0 or above and never NaN, so its bits order as its value does, and
// (bits(d2) << 32) | j orders by d2, then by index: keys of different j are different, and ties cannot make a list ambiguous.
//
// Why a round is exact.  knn_math.h's proof, with keys: a lane that walks the 27 cells sees every j with d2(i, j) <= r2.  If the
// d2 of its k-th smallest key is <= r2, a j it did not see has d2 > r2, a larger key than all k it kept: they are the k smallest
// keys of all.  Unlike the search by values, a lane cannot stop once its k-th d2 is 0: a smaller index at d2 = 0 may still come.
//
// Why the fit needs no rescaling.  The offsets are float32, their products and the sums of up to 17 of them are far inside double's
// range (|q| < 2^128, q * q < 2^256), and a product of two float32 values is exact in double.
#pragma once
#include <math.h>
#include <stdint.h>

#include "export_math.h"
#include "neighbors_math.h"

#if defined(__clang__)
#define GSX_NM_UNROLL _Pragma("unroll")  // the K registers stay registers only where the loops over them are unrolled
#else
#define GSX_NM_UNROLL
#endif

namespace gsx {

constexpr uint32_t kNormalsMinK = 3u;             // GSX_NORMALS_MIN_K
constexpr uint32_t kNormalsMaxK = 16u;            // GSX_NORMALS_MAX_K
constexpr uint32_t kNormalsOrientCanonical = 0u;  // GSX_NORMALS_ORIENT_CANONICAL
constexpr uint32_t kNormalsOrientToward = 1u;     // GSX_NORMALS_ORIENT_TOWARD
constexpr uint32_t kNormalsSelectVariation = 0u;  // GSX_NORMALS_SELECT_VARIATION
constexpr uint32_t kNormalsSelectFacing = 1u;     // GSX_NORMALS_SELECT_FACING
constexpr uint32_t kNormalsAbs = 1u;              // GSX_NORMALS_ABS
constexpr uint32_t kNormalsNone = 0xFFFFFFFFu;    // GSX_NORMALS_NONE: no such neighbour
constexpr uint32_t kNormalsBruteLanes = 256u;     // the lanes of one workgroup of the exact fallback
constexpr uint64_t kNormalsEmpty = (uint64_t(0x7F800000u) << 32) | kNormalsNone;  // (+inf, none): above every key of a neighbour

GSX_NB_HD inline uint32_t nm_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
GSX_NB_HD inline uint64_t nm_key(float d2, uint32_t j) { return ((uint64_t)nm_bits(d2) << 32) | j; }
GSX_NB_HD inline float nm_key_d2(uint64_t key) { return nb_from_bits((uint32_t)(key >> 32)); }
// the index a list entry reports: none where the distance is +inf (an empty slot, or a difference that overflowed)
GSX_NB_HD inline uint32_t nm_key_index(uint64_t key) { return nb_finite(nm_key_d2(key)) ? (uint32_t)key : kNormalsNone; }

// The lane's k smallest keys in K registers, k <= K, as knn_math.h keeps its values: b[K - k .. K - 1] hold them ascending,
// kNormalsEmpty where fewer were offered, and b[0 .. K - k - 1] are pinned at 0, which no offer displaces (min(0, key) is 0).  So
// the k-th smallest is always b[K - 1], a constant index.  nm_offer takes one more key: a compare-exchange chain over constant
// indices.  A key is offered at most once (a walk gives a record once), so equal keys never meet but at the pinned 0.
template <int K>
GSX_NB_HD inline void nm_reset(uint64_t (&b)[K], uint32_t k) {
GSX_NM_UNROLL
    for (int q = 0; q < K; ++q) b[q] = (uint32_t)q + k < (uint32_t)K ? 0u : kNormalsEmpty;
}
template <int K>
GSX_NB_HD inline void nm_offer(uint64_t (&b)[K], uint64_t key) {
GSX_NM_UNROLL
    for (int q = 0; q < K; ++q) {
        const uint64_t lo = b[q] < key ? b[q] : key;
        key = b[q] < key ? key : b[q];
        b[q] = lo;
    }
}
template <int K>
GSX_NB_HD inline uint64_t nm_last(const uint64_t (&b)[K]) {
    return b[K - 1];
}
// Is the list of a lane that kept only candidates with d2 <= r2 out of its 27 cells the true list?
GSX_NB_HD inline bool nm_list_proven(uint64_t last, float r2) { return nm_key_d2(last) <= r2; }
// Can a plane be fitted to the list?  All k entries finite (the list ascends: the k-th is) and not all k coincident with i.
GSX_NB_HD inline bool nm_list_fitted(uint64_t last) {
    const float d2 = nm_key_d2(last);
    return nb_finite(d2) && d2 > 0.0f;
}
// The list's k indices to out[0 .. k - 1].
template <int K>
GSX_NB_HD inline void nm_store_indices(const uint64_t (&b)[K], uint32_t k, uint32_t* out) {
GSX_NM_UNROLL
    for (int q = 0; q < K; ++q)
        if ((uint32_t)q + k >= (uint32_t)K) out[(uint32_t)q + k - (uint32_t)K] = nm_key_index(b[q]);
}

// What a Gaussian keeps of its fit.  Unfitted (and a Gaussian that does not participate): normal (0, 0, 0), variation +inf.
struct NormalFit {
    float n[3];
    float variation;
    bool fitted;
};
GSX_NB_HD inline NormalFit nm_unfitted() { return NormalFit{{0.0f, 0.0f, 0.0f}, INFINITY, false}; }

// The sign.  CANONICAL: the first non-zero component is positive.  TOWARD: the normal looks at the point `toward`; a dot product of
// exactly 0 falls back to the canonical rule.  The dot product takes the float32 normal, in double, in axis order.
GSX_NB_HD inline bool nm_flip_canonical(const float n[3]) { return n[0] < 0.0f || (n[0] == 0.0f && (n[1] < 0.0f || (n[1] == 0.0f && n[2] < 0.0f))); }
GSX_NB_HD inline bool nm_flip(const float n[3], const float p[3], uint32_t orient, const float toward[3]) {
    if (orient == kNormalsOrientToward) {
        double dot = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double t = (double)toward[a] - (double)p[a];
            const double prod = (double)n[a] * t;
            dot = dot + prod;
        }
        if (dot != 0.0) return dot < 0.0;
    }
    return nm_flip_canonical(n);
}

// The plane fit of Gaussian i at p to its list b (nm_list_fitted or not).  fetch(j, out): the stored position of neighbour j.
// Offsets q_0 = 0 (i itself) and q_m = fl32(p_j - p) per axis in list order; the mean of the k + 1 and the scatter about it in
// double, both sums in ascending m; kExportSweeps sweeps of export_math.h's rotation in its pair order, its descending sort; the
// eigenvalues clamped at 0; the normal is the last column over its length, rounded to float32; variation = l2 / ((l0 + l1) + l2).
template <int K, class Fetch>
GSX_NB_HD inline NormalFit nm_plane_fit(const uint64_t (&b)[K], uint32_t k, const float p[3], Fetch fetch, uint32_t orient, const float toward[3]) {
    if (!nm_list_fitted(nm_last(b))) return nm_unfitted();
    float off[K][3];
    double sum[3] = {0.0, 0.0, 0.0};  // (q_0 = 0 is the first term)
GSX_NM_UNROLL
    for (int q = 0; q < K; ++q) {
        if ((uint32_t)q + k < (uint32_t)K) {
            off[q][0] = off[q][1] = off[q][2] = 0.0f;
            continue;
        }
        float pj[3];
        fetch((uint32_t)b[q], pj);
        for (int a = 0; a < 3; ++a) {
            off[q][a] = pj[a] - p[a];
            sum[a] = sum[a] + (double)off[q][a];
        }
    }
    const double count = (double)(k + 1u);
    const double mu[3] = {sum[0] / count, sum[1] / count, sum[2] / count};
    // the scatter's upper triangle xx, xy, xz, yy, yz, zz; the first term is i's own offset, 0
    const double s0[3] = {0.0 - mu[0], 0.0 - mu[1], 0.0 - mu[2]};
    double c[6] = {s0[0] * s0[0], s0[0] * s0[1], s0[0] * s0[2], s0[1] * s0[1], s0[1] * s0[2], s0[2] * s0[2]};
GSX_NM_UNROLL
    for (int q = 0; q < K; ++q) {
        if ((uint32_t)q + k < (uint32_t)K) continue;
        const double x = (double)off[q][0] - mu[0], y = (double)off[q][1] - mu[1], z = (double)off[q][2] - mu[2];
        c[0] = c[0] + x * x;
        c[1] = c[1] + x * y;
        c[2] = c[2] + x * z;
        c[3] = c[3] + y * y;
        c[4] = c[4] + y * z;
        c[5] = c[5] + z * z;
    }
    double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kExportSweeps; ++sweep) {
        ex_rotate<double, 0, 1>(a, v);
        ex_rotate<double, 0, 2>(a, v);
        ex_rotate<double, 1, 2>(a, v);
    }
    double l[3] = {a[0][0], a[1][1], a[2][2]};
    ex_sort_pair<double, 0, 1>(l, v);
    ex_sort_pair<double, 1, 2>(l, v);
    ex_sort_pair<double, 0, 1>(l, v);
    for (int e = 0; e < 3; ++e) l[e] = l[e] > 0.0 ? l[e] : 0.0;  // (a NaN becomes 0 too)
    const double trace = (l[0] + l[1]) + l[2];
    if (!(trace > 0.0 && trace < (double)INFINITY)) return nm_unfitted();
    const double len = sqrt((v[0][2] * v[0][2] + v[1][2] * v[1][2]) + v[2][2] * v[2][2]);
    NormalFit f;
    f.n[0] = (float)(v[0][2] / len);
    f.n[1] = (float)(v[1][2] / len);
    f.n[2] = (float)(v[2][2] / len);
    const float sign = nm_flip(f.n, p, orient, toward) ? -1.0f : 1.0f;
    for (int e = 0; e < 3; ++e) f.n[e] = sign * f.n[e] + 0.0f;  // (-0 -> +0)
    f.variation = (float)(l[2] / trace);
    f.fitted = true;
    return f;
}

// A Gaussian is fitted iff its stored variation is finite (an unfitted one and one that does not participate keep +inf).
GSX_NB_HD inline bool nm_is_fitted(float variation) { return nb_finite(variation); }

// The select's direction: dir normalised in double, rounded to float32.  false where dir is not finite or its length is 0.
inline bool nm_direction(const float dir[3], float out[3]) {
    if (!(nb_finite(dir[0]) && nb_finite(dir[1]) && nb_finite(dir[2]))) return false;
    const double x = (double)dir[0], y = (double)dir[1], z = (double)dir[2];
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0)) return false;
    out[0] = (float)(x / len);
    out[1] = (float)(y / len);
    out[2] = (float)(z / len);
    return true;
}
// The select's test: hit iff fitted and lo <= the measure <= hi.  VARIATION: the variation.  FACING: c = (nx dx + ny dy) + nz dz in
// float32, every operation rounded; |c| with kNormalsAbs.
GSX_NB_HD inline bool nm_select_hit(uint32_t mode, uint32_t flags, const float n[3], float variation, const float d[3], float lo, float hi) {
    if (!nm_is_fitted(variation)) return false;
    float c = variation;
    if (mode == kNormalsSelectFacing) {
        c = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
        if (flags & kNormalsAbs) c = fabsf(c);
    }
    return c >= lo && c <= hi;
}

}  // namespace gsx
