// align_plane_math.h — the host solve of one point-to-plane registration step (spec/RENDER_SPEC.md §27, gsx_model_align_plane_step),
// written once: gsx_api_nearest.cpp and tests/align_plane_driver.cpp include it.  Over the used pairs (q, t, n) — a mapped source
// position, its nearest target and that target's kept unit normal — the device sums, about the centre c = fl32(mean q),
//   J = ((q - c) x n, n),  e = (q - t) . n,  A = sum J J^T (6x6, symmetric),  b = sum J e,
// and the small motion x = (omega, tau) about c that minimises sum (e + J . x)^2 solves A x = -b.  A is rarely of full rank (a floor
// against a floor determines the lift and two tilts only), so the solve is spectral: A's eigenvalues and eigenvectors by align_math.h's
// cyclic Jacobi, the eigenvalues above kAlignPlaneRank x the largest kept, x = -sum v (v . b) / lambda over the kept ones: the
// minimum-norm solution, exactly 0 along every direction the pairs do not determine.  Nothing depends on the sign of n.
// Plain double arithmetic, <math.h> only; no HIP.  Built with -ffp-contract=off wherever it is included.
#pragma once
#include "align_math.h"

namespace gsx {

constexpr uint32_t kAlignPlaneTri = 21;  // the upper triangle of a symmetric 6x6 matrix, row-major: (0,0) .. (0,5), (1,1) .. (5,5)
// What the device accumulates over the used pairs, in double: the count and, from the sum of q, the centre (pass 0), and about the
// centre the upper triangle of A, b, sum e^2 and sum d2 (pass 1).
struct AlignPlaneSums {
    double n = 0.0;
    double centre[3] = {0, 0, 0};
    double A[kAlignPlaneTri] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double b[6] = {0, 0, 0, 0, 0, 0};
    double sum_e2 = 0.0, sum_d2 = 0.0;
};
struct AlignPlaneDelta {
    AlignDelta delta;                           // quat (x, y, z, w), w >= 0; scale 1; pos; degenerate: fewer than 3 pairs or rank 0
    double centre[3] = {0, 0, 0};               // c
    double eigenvalues[6] = {0, 0, 0, 0, 0, 0};  // descending
    double x[6] = {0, 0, 0, 0, 0, 0};           // (omega, tau)
    uint32_t rank = 0;
};

constexpr double kAlignPlaneRank = kAlignGap;  // an eigenvalue at or below this share of the largest: its direction is not determined

// one axis of the centre: the mean of q rounded to float32, 0 without pairs (the kernel's pass 1 rounds the same quotient)
inline double align_plane_centre(double sum_q, double pairs) { return pairs > 0.0 ? (double)(float)(sum_q / pairs) : 0.0; }

inline AlignPlaneDelta align_plane_solve(const AlignPlaneSums& s) {
    AlignPlaneDelta d;
    for (int a = 0; a < 3; ++a) d.centre[a] = s.centre[a];
    double M[36], w[6], V[36];
    for (int r = 0, k = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c, ++k) M[6 * r + c] = M[6 * c + r] = s.A[k];
    align_jacobi<6>(M, w, V);
    int order[6] = {0, 1, 2, 3, 4, 5};  // descending eigenvalues, equal ones by column: an insertion sort
    for (int i = 1; i < 6; ++i)
        for (int j = i; j > 0 && w[order[j]] > w[order[j - 1]]; --j) {
            const int o = order[j];
            order[j] = order[j - 1];
            order[j - 1] = o;
        }
    for (int i = 0; i < 6; ++i) d.eigenvalues[i] = w[order[i]];
    const double largest = d.eigenvalues[0];
    if (largest > 0.0)
        for (int i = 0; i < 6; ++i)
            if (d.eigenvalues[i] > kAlignPlaneRank * largest) d.rank += 1u;
    if (s.n < 3.0 || d.rank == 0u) {
        d.delta.degenerate = true;
        return d;
    }
    for (uint32_t i = 0; i < d.rank; ++i) {
        const int col = order[i];
        double vb = 0.0;
        for (int r = 0; r < 6; ++r) vb += V[6 * r + col] * s.b[r];
        const double f = vb / w[col];
        for (int r = 0; r < 6; ++r) d.x[r] -= V[6 * r + col] * f;
    }
    const double angle = sqrt((d.x[0] * d.x[0] + d.x[1] * d.x[1]) + d.x[2] * d.x[2]);
    if (angle > 0.0) {
        const double half = 0.5 * angle, sn = sin(half) / angle, cs = cos(half), sign = cs < 0.0 ? -1.0 : 1.0;
        for (int a = 0; a < 3; ++a) d.delta.quat[a] = sign * (d.x[a] * sn);
        d.delta.quat[3] = sign * cs;
    }
    double R[9];
    align_quat_rows(d.delta.quat, R);
    for (int r = 0; r < 3; ++r) {
        double rc = 0.0;
        for (int c = 0; c < 3; ++c) rc += R[3 * r + c] * d.centre[c];
        d.delta.pos[r] = (d.centre[r] + d.x[3 + r]) - rc;
    }
    return d;
}

}  // namespace gsx
