// plane_math.h — the rules of the model plane (spec/RENDER_SPEC.md §28, "Model plane"), written once: the kernels of kernels_plane.hip,
// the host side of gsx_api_plane.cpp and the host replay tests/plane_driver.cpp all include it, so they cannot drift.  It holds the
// counter-based hash that samples the candidates and the probe that turns it into a participant's index, the two candidate
// constructions, the residual and the inlier rule (pl_residual, pl_inlier, pl_in_range, pl_facing: the ONLY copies — the score, the
// moments and the select call them), the winner, the least-squares plane of the moments (the host solve) and gsx_plane_level.  The
// Jacobi rotation and the sort are export_math.h's templates, the sign of a normal and "fitted" normals_math.h's.  Plain float32 /
// double / integer arithmetic, <math.h> only; no HIP include.  Built with -ffp-contract=off wherever it is included.
#pragma once
#include <math.h>
#include <stdint.h>

#include "normals_math.h"

namespace gsx {

constexpr uint32_t kPlaneMaxCandidates = 1024u;  // GSX_PLANE_MAX_CANDIDATES
constexpr uint32_t kPlaneSampleTriples = 0u;     // GSX_PLANE_SAMPLE_TRIPLES
constexpr uint32_t kPlaneSampleNormals = 1u;     // GSX_PLANE_SAMPLE_NORMALS
constexpr uint32_t kPlaneSampleCaller = 2u;      // GSX_PLANE_SAMPLE_CALLER
constexpr uint32_t kPlaneProbes = 64u;           // the indices a slot tries before it gives up
constexpr uint32_t kPlaneMaxRefine = 8u;         // GSX_PLANE_MAX_REFINE
constexpr uint32_t kPlaneNone = 0xFFFFFFFFu;     // GSX_PLANE_NONE: no index, no winner
constexpr uint32_t kPlaneMinInliers = 3u;        // a winner with fewer inliers is no plane

// The plane as the kernels carry it: the points p with (nx px + ny py) + nz pz = offset.
struct Plane {
    float n[3];
    float offset;
};

// ---- the sampling -------------------------------------------------------------------------------------------------------------------
// mix(seed, h, s, t): output number k = (h << 16) | (s << 8) | t of the splitmix64 stream seeded with `seed`: the state seed + (k + 1) *
// golden through splitmix64's finaliser.  h < 2^16 (at most 1024), s < 3, t < 64: the counters of different (h, s, t) differ.
GSX_NB_HD inline uint64_t pl_mix(uint64_t seed, uint32_t h, uint32_t s, uint32_t t) {
    const uint64_t k = ((uint64_t)h << 16) | ((uint64_t)s << 8) | (uint64_t)t;
    uint64_t z = seed + (k + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// Slot s of candidate h: the first of the indices mix(seed, h, s, t) mod n, t = 0 .. 63, that ok(index) accepts; kPlaneNone if none
// does (or n is 0).
template <class Ok>
GSX_NB_HD inline uint32_t pl_probe(uint64_t seed, uint32_t h, uint32_t s, uint64_t n, Ok ok) {
    if (n == 0) return kPlaneNone;
    for (uint32_t t = 0; t < kPlaneProbes; ++t) {
        const uint32_t i = (uint32_t)(pl_mix(seed, h, s, t) % n);
        if (ok(i)) return i;
    }
    return kPlaneNone;
}

// ---- the residual and the inlier rule ---------------------------------------------------------------------------------------------------
// r = ((nx px + ny py) + nz pz) - offset in float32, every operation rounded
GSX_NB_HD inline float pl_dot(const Plane& pl, float px, float py, float pz) { return (pl.n[0] * px + pl.n[1] * py) + pl.n[2] * pz; }
GSX_NB_HD inline float pl_residual(const Plane& pl, float px, float py, float pz) { return pl_dot(pl, px, py, pz) - pl.offset; }
// the fit's distance test: inclusive.  A NaN residual (an invalid candidate carries a NaN offset) is no inlier.
GSX_NB_HD inline bool pl_inlier(float r, float tolerance) { return fabsf(r) <= tolerance; }
// the select's: signed, a bound may be infinite
GSX_NB_HD inline bool pl_in_range(float r, float lo, float hi) { return r >= lo && r <= hi; }
// With min_cos > 0: the Gaussian is fitted (normals_math.h: a finite variation) and |c| >= min_cos, c = section 26's FACING cosine of
// its kept normal k against the plane's normal, (kx nx + ky ny) + kz nz in float32.  The score tests the first half once a Gaussian
// and the second (pl_cos_ok) once a plane.
GSX_NB_HD inline bool pl_cos_ok(const Plane& pl, float kx, float ky, float kz, float min_cos) { return fabsf(pl_dot(pl, kx, ky, kz)) >= min_cos; }
GSX_NB_HD inline bool pl_facing(const Plane& pl, float kx, float ky, float kz, float variation, float min_cos) {
    return nm_is_fitted(variation) && pl_cos_ok(pl, kx, ky, kz, min_cos);
}
// three finite stored coordinates
GSX_NB_HD inline bool pl_finite3(float x, float y, float z) { return nb_finite(x) && nb_finite(y) && nb_finite(z); }

// ---- the candidates ---------------------------------------------------------------------------------------------------------------------
// What an invalid candidate is scored with: every residual is NaN, so it has no inlier.  It is REPORTED as normal 0, offset 0.
GSX_NB_HD inline Plane pl_invalid() { return Plane{{0.0f, 0.0f, 0.0f}, nb_from_bits(0x7FC00000u)}; }
// NORMALS: a participant a and its kept normal k
GSX_NB_HD inline Plane pl_from_normal(const float a[3], const float k[3]) {
    Plane pl{{k[0], k[1], k[2]}, 0.0f};
    pl.offset = pl_dot(pl, a[0], a[1], a[2]);
    return pl;
}
// TRIPLES: u = b - a, v = c - a per axis in float32; u x v in double, each component the difference of two exact products; its
// length in double; the quotient rounded to float32; the offset from a.  false: the length is zero or not finite.
GSX_NB_HD inline bool pl_from_triple(const float a[3], const float b[3], const float c[3], Plane* out) {
    const float uf[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, vf[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double u[3] = {(double)uf[0], (double)uf[1], (double)uf[2]}, v[3] = {(double)vf[0], (double)vf[1], (double)vf[2]};
    const double x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0 && len < (double)INFINITY)) return false;
    Plane pl{{(float)(x / len), (float)(y / len), (float)(z / len)}, 0.0f};
    pl.offset = pl_dot(pl, a[0], a[1], a[2]);
    *out = pl;
    return true;
}
// CALLER: used as given (not normalised); every component finite and the normal not zero
GSX_NB_HD inline bool pl_caller_ok(const Plane& pl) {
    return pl_finite3(pl.n[0], pl.n[1], pl.n[2]) && nb_finite(pl.offset) && (pl.n[0] != 0.0f || pl.n[1] != 0.0f || pl.n[2] != 0.0f);
}

// ---- the winner -------------------------------------------------------------------------------------------------------------------------
// The valid candidate with the largest count, ties to the smaller h; kPlaneNone without a valid candidate.
inline uint32_t pl_winner(const uint32_t* counts, const uint32_t* valid, uint32_t n_candidates) {
    uint32_t best = kPlaneNone;
    for (uint32_t h = 0; h < n_candidates; ++h)
        if (valid[h] && (best == kPlaneNone || counts[h] > counts[best])) best = h;
    return best;
}

// ---- the least-squares plane --------------------------------------------------------------------------------------------------------------
// What the device sums over a plane's inliers, in double: pass 0 the count, sum p and sum r^2 (r the float32 residual against that
// plane, squared exactly in double); pass 1, about c = fl32(sum p / count) per axis, d = p - c in float32 and the upper triangle of
// sum d d^T (xx, xy, xz, yy, yz, zz) as sums of exact products.
struct PlaneSums {
    double count = 0.0;
    double sum_p[3] = {0, 0, 0};
    double sum_r2 = 0.0;
    double scatter[6] = {0, 0, 0, 0, 0, 0};
};
// one axis of the centre (the kernel's pass 1 rounds the same quotient)
GSX_NB_HD inline float pl_centre(double sum_p, double count) { return count > 0.0 ? (float)(sum_p / count) : 0.0f; }

struct PlaneFit {
    Plane plane{{0.0f, 0.0f, 0.0f}, 0.0f};
    float centre[3] = {0.0f, 0.0f, 0.0f};
    double eigenvalues[3] = {0, 0, 0};  // descending, clamped at 0
    bool ok = false;                    // false: fewer than kPlaneMinInliers points, or their scatter is zero or not finite
};
// kExportSweeps sweeps of export_math.h's rotation in its pair order and its descending sort, as the normals' fit calls them; the
// normal is the eigenvector of the smallest eigenvalue over its length, in double, rounded to float32; its sign section 26's rule at
// the centre; offset = (float)((nx cx + ny cy) + nz cz), the float32 normal and centre taken in double.
inline PlaneFit pl_solve(const PlaneSums& s, uint32_t orient, const float toward[3]) {
    PlaneFit f;
    if (!(s.count >= (double)kPlaneMinInliers)) return f;
    for (int a = 0; a < 3; ++a) f.centre[a] = pl_centre(s.sum_p[a], s.count);
    const double* c = s.scatter;
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
    if (!(trace > 0.0 && trace < (double)INFINITY)) return f;
    const double len = sqrt((v[0][2] * v[0][2] + v[1][2] * v[1][2]) + v[2][2] * v[2][2]);
    float n[3] = {(float)(v[0][2] / len), (float)(v[1][2] / len), (float)(v[2][2] / len)};
    const float sign = nm_flip(n, f.centre, orient, toward) ? -1.0f : 1.0f;
    for (int e = 0; e < 3; ++e) f.plane.n[e] = sign * n[e] + 0.0f;  // (-0 -> +0)
    f.plane.offset = (float)(((double)f.plane.n[0] * (double)f.centre[0] + (double)f.plane.n[1] * (double)f.centre[1]) + (double)f.plane.n[2] * (double)f.centre[2]);
    for (int e = 0; e < 3; ++e) f.eigenvalues[e] = l[e];
    f.ok = true;
    return f;
}

// ---- gsx_plane_level ------------------------------------------------------------------------------------------------------------------------
// The rigid motion that stands a plane level, in double: quat (x, y, z, w), w >= 0, is the shortest-arc rotation that takes the plane's
// unit normal a = n / |n| to b = up / |up|: (a x b, 1 + a . b) over its length.  Antiparallel (1 + a . b <= 2^-40: the arc's axis is no
// longer determined): the half turn about the fixed perpendicular e x a over its length, e the coordinate axis along which |a| is
// smallest (the first of equals), w = 0.  pos = -(offset / |n|) b: the rotated plane passes through the origin's height.  false:
// a normal or an up that is zero or not finite, or an offset that is not finite.
inline bool pl_level(const Plane& pl, const float up[3], double quat[4], double pos[3]) {
    if (!pl_caller_ok(pl) || !pl_finite3(up[0], up[1], up[2])) return false;
    const double n[3] = {(double)pl.n[0], (double)pl.n[1], (double)pl.n[2]}, u[3] = {(double)up[0], (double)up[1], (double)up[2]};
    const double nl = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]), ul = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    if (!(nl > 0.0) || !(ul > 0.0)) return false;
    const double a[3] = {n[0] / nl, n[1] / nl, n[2] / nl}, b[3] = {u[0] / ul, u[1] / ul, u[2] / ul};
    const double w = 1.0 + ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
    double q[4];
    if (w > 0x1p-40) {
        q[0] = a[1] * b[2] - a[2] * b[1];
        q[1] = a[2] * b[0] - a[0] * b[2];
        q[2] = a[0] * b[1] - a[1] * b[0];
        q[3] = w;
    } else {
        int e = 0;
        if (fabs(a[1]) < fabs(a[e])) e = 1;
        if (fabs(a[2]) < fabs(a[e])) e = 2;
        const double ax[3] = {e == 0 ? 1.0 : 0.0, e == 1 ? 1.0 : 0.0, e == 2 ? 1.0 : 0.0};
        q[0] = ax[1] * a[2] - ax[2] * a[1];
        q[1] = ax[2] * a[0] - ax[0] * a[2];
        q[2] = ax[0] * a[1] - ax[1] * a[0];
        q[3] = 0.0;
    }
    const double ql = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) quat[k] = q[k] / ql + 0.0;
    const double h = (double)pl.offset / nl;
    for (int k = 0; k < 3; ++k) pos[k] = -(h * b[k]) + 0.0;
    return true;
}

}  // namespace gsx
