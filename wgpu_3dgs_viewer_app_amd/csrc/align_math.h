// align_math.h — the host solve of one point-to-point registration step (spec/RENDER_SPEC.md §23, gsx_model_align_step), written
// once: gsx_api_nearest.cpp and tests/nearest_driver.cpp include it.  From the sums over the found pairs (q, t) — the means, the
// centred cross-covariance H = sum (q - qm)(t - tm)^T, sum |q - qm|^2 — it gives the similarity t ~ s R q + p that minimises the
// squared residual: Horn's closed form (J. Opt. Soc. Am. A 4, 1987).  The unit quaternion of R is the eigenvector of the largest
// eigenvalue of the symmetric 4x4 matrix N(H), found by cyclic Jacobi rotations to convergence; s = sum (t - tm) . R (q - qm) /
// sum |q - qm|^2 where a scale is asked for, 1 otherwise; p = tm - s R qm.
// Plain double arithmetic, <math.h> only; no HIP.  Built with -ffp-contract=off wherever it is included.
#pragma once
#include <math.h>
#include <stdint.h>

namespace gsx {

// What the device accumulates over the found pairs, in double: the count, the sums of q and t (pass 0), and about the means rounded
// to float32 the cross-covariance (row: q's axis, column: t's), the two spreads and the sum of d2 (pass 1).
struct AlignSums {
    double n = 0.0;
    double sum_q[3] = {0, 0, 0}, sum_t[3] = {0, 0, 0};
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double spread_q = 0.0, spread_t = 0.0, sum_d2 = 0.0;
};
struct AlignDelta {
    double quat[4] = {0, 0, 0, 1};  // (x, y, z, w), w >= 0
    double scale = 1.0;
    double pos[3] = {0, 0, 0};
    bool degenerate = false;         // fewer than 3 pairs, no spread, or no single best rotation: the identity above
    double eigenvalue = 0.0, gap = 0.0;  // N's largest eigenvalue and its distance to the next one
};

constexpr double kAlignGap = 1e-9;   // a gap below this share of N's Frobenius norm: the rotation is not determined (collinear pairs)
constexpr int kAlignSweeps = 64;     // cyclic Jacobi converges quadratically: a 4x4 or 6x6 matrix needs fewer than ten sweeps

// Horn's N(H), symmetric, row-major, over the quaternion (w, x, y, z).
inline void align_horn_matrix(const double H[9], double N[16]) {
    const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
    const double M[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                          Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                          Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                          Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
    for (int k = 0; k < 16; ++k) N[k] = M[k];
}

// The eigenvalues (w[N]) and eigenvectors (the columns of V, row-major) of the symmetric N x N matrix A, by cyclic Jacobi: sweeps over
// the pairs (p, q), p < q, until every off-diagonal element is exactly 0 or a sweep changes nothing any more.  The one copy of the
// rotation: the 4x4 matrix of Horn's solve below and the 6x6 normal matrix of align_plane_math.h both run it.
template <int N>
inline void align_jacobi(const double* A_in, double* w, double* V) {
    double A[N * N];
    for (int k = 0; k < N * N; ++k) {
        A[k] = A_in[k];
        V[k] = (k % (N + 1) == 0) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < kAlignSweeps; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < N; ++p)
            for (int q = 0; q < N; ++q) (p == q ? diag : off) += A[N * p + q] * A[N * p + q];
        if (off == 0.0 || off <= 1e-60 * diag) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[N * p + q];
                if (apq == 0.0) continue;
                const double theta = (A[N * q + q] - A[N * p + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) {  // A <- A J
                    const double akp = A[N * k + p], akq = A[N * k + q];
                    A[N * k + p] = c * akp - s * akq;
                    A[N * k + q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; ++k) {  // A <- J^T A
                    const double apk = A[N * p + k], aqk = A[N * q + k];
                    A[N * p + k] = c * apk - s * aqk;
                    A[N * q + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < N; ++k) {  // V <- V J
                    const double vkp = V[N * k + p], vkq = V[N * k + q];
                    V[N * k + p] = c * vkp - s * vkq;
                    V[N * k + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int k = 0; k < N; ++k) w[k] = A[(N + 1) * k];
}
inline void align_jacobi4(const double A_in[16], double w[4], double V[16]) { align_jacobi<4>(A_in, w, V); }

// The rotation matrix of a unit quaternion (x, y, z, w), row-major.
inline void align_quat_rows(const double q[4], double r[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    r[0] = 1.0 - 2.0 * (y * y + z * z); r[1] = 2.0 * (x * y - w * z); r[2] = 2.0 * (x * z + w * y);
    r[3] = 2.0 * (x * y + w * z); r[4] = 1.0 - 2.0 * (x * x + z * z); r[5] = 2.0 * (y * z - w * x);
    r[6] = 2.0 * (x * z - w * y); r[7] = 2.0 * (y * z + w * x); r[8] = 1.0 - 2.0 * (x * x + y * y);
}

inline AlignDelta align_solve(const AlignSums& s, bool with_scale) {
    AlignDelta d;
    if (s.n < 3.0 || !(s.spread_q > 0.0)) {
        d.degenerate = true;
        return d;
    }
    double N[16], w[4], V[16];
    align_horn_matrix(s.H, N);
    align_jacobi4(N, w, V);
    int best = 0;
    for (int k = 1; k < 4; ++k)
        if (w[k] > w[best]) best = k;
    double second = -INFINITY, norm2 = 0.0;
    for (int k = 0; k < 4; ++k)
        if (k != best && w[k] > second) second = w[k];
    for (int k = 0; k < 16; ++k) norm2 += N[k] * N[k];
    d.eigenvalue = w[best];
    d.gap = w[best] - second;
    if (!(d.gap > kAlignGap * sqrt(norm2))) {
        d.degenerate = true;
        return d;
    }
    double q[4] = {V[4 * 0 + best], V[4 * 1 + best], V[4 * 2 + best], V[4 * 3 + best]};  // (w, x, y, z)
    const double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sign = q[0] < 0.0 ? -1.0 : 1.0;
    d.quat[0] = sign * q[1] / len; d.quat[1] = sign * q[2] / len; d.quat[2] = sign * q[3] / len; d.quat[3] = sign * q[0] / len;
    double R[9];
    align_quat_rows(d.quat, R);
    if (with_scale) {
        double num = 0.0;  // sum (t - tm) . R (q - qm) = sum over (r, c) of R[r][c] H[c][r]
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) num += R[3 * r + c] * s.H[3 * c + r];
        d.scale = num / s.spread_q;
    }
    for (int r = 0; r < 3; ++r) {
        double rq = 0.0;
        for (int c = 0; c < 3; ++c) rq += R[3 * r + c] * (s.sum_q[c] / s.n);
        d.pos[r] = s.sum_t[r] / s.n - d.scale * rq;
    }
    return d;
}

// delta o xform: the 3x4 float32 matrix of x -> s R (A x + b) + p, composed in double and rounded once.
inline void align_compose(const AlignDelta& d, const float xform[12], float out[12]) {
    double R[9];
    align_quat_rows(d.quat, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 4; ++c) {
            double a = 0.0;
            for (int k = 0; k < 3; ++k) a += R[3 * r + k] * (double)xform[4 * k + c];
            out[4 * r + c] = (float)(d.scale * a + (c == 3 ? d.pos[r] : 0.0));
        }
    }
}

}  // namespace gsx
