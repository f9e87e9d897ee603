// merge_driver.cpp — csrc/merge_math.h played on the host, for tests/test_merge_cpu.py.  A stand-alone program: built with the
// address and undefined-behaviour sanitizers and run as a child process.  It reads commands from stdin, one a line, floats as the
// eight hex digits of their bit pattern:
//   quat x y z w                         -> "M" + the 83 float64 matrix entries of the normalised quaternion, "Mf" + the same rounded to
//                                           float32 as the kernel gets them, "ortho" + max |M M^T - I|, "prop" + the largest violation of
//                                           sum_k (M c)_k Y_k(R d) = sum_k c_k Y_k(d) over unit vectors c and a few hundred directions
//   comp x1 y1 z1 w1 x2 y2 z2 w2         -> "comp" + max |M(q1 q2) - M(q1) M(q2)|
//   joint off count0 count1 seed         -> two sources of count0 (= off) and count1 Gaussians with pseudo-random `edited` bits, ORed
//                                           into a zeroed plane through merge_bit_word / merge_bit_mask, second source first and then
//                                           the other way round (the program fails if the two planes differ): "bits" + the 0/1
//                                           string of the concatenation, "words" + the plane in hex, "shared" + merge_joint_shared(off)
//   ident px py pz qx qy qz qw sx sy sz  -> "ident" + merge_is_identity, "valid" + merge_is_valid
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "merge_math.h"

using namespace gsx;

static float bits_float(unsigned u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// band l of a * b -> out (row-major m x m)
static void band_mul(const double* a, const double* b, int l, double* out) {
    const int m = kMergeBandSize[l], o = kMergeBandMatrix[l];
    for (int r = 0; r < m; ++r)
        for (int c = 0; c < m; ++c) {
            double s = 0.0;
            for (int k = 0; k < m; ++k) s += a[o + r * m + k] * b[o + k * m + c];
            out[r * m + c] = s;
        }
}

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        unsigned u[10];
        unsigned long long a0, a1, a2, a3;
        if (sscanf(line, "quat %x %x %x %x", &u[0], &u[1], &u[2], &u[3]) == 4) {
            const float q[4] = {bits_float(u[0]), bits_float(u[1]), bits_float(u[2]), bits_float(u[3])};
            double qn[4], M[kMergeShFloats], R[9];
            float Mf[kMergeShFloats];
            merge_unit_quat(q, qn);
            merge_sh_matrices_f64(qn, M);
            merge_sh_matrices(q, Mf);
            merge_quat_matrix(qn, R);
            printf("M");
            for (int k = 0; k < kMergeShFloats; ++k) printf(" %.17g", M[k]);
            printf("\nMf");
            for (int k = 0; k < kMergeShFloats; ++k) printf(" %.9g", (double)Mf[k]);
            double ortho = 0.0, prop = 0.0;
            for (int l = 0; l < 3; ++l) {
                const int m = kMergeBandSize[l], o = kMergeBandMatrix[l];
                for (int r = 0; r < m; ++r)
                    for (int c = 0; c < m; ++c) {
                        double s = 0.0;
                        for (int k = 0; k < m; ++k) s += M[o + r * m + k] * M[o + c * m + k];
                        ortho = fmax(ortho, fabs(s - (r == c ? 1.0 : 0.0)));
                    }
            }
            // directions that the construction did not use (another spiral), unit coefficient vectors e_k: (M e_k) . Y(R d) = Y_k(d)
            for (int i = 0; i < 300; ++i) {
                const double h = 1.0 - (2.0 * i + 1.0) / 300.0, rr = sqrt(1.0 - h * h), phi = 1.0 + 2.399963229728653 * i;
                const double d[3] = {rr * sin(phi), h, rr * cos(phi)};
                const double rd[3] = {R[0] * d[0] + R[1] * d[1] + R[2] * d[2], R[3] * d[0] + R[4] * d[1] + R[5] * d[2], R[6] * d[0] + R[7] * d[1] + R[8] * d[2]};
                double y[15], z[15];
                merge_sh_basis(d, y);
                merge_sh_basis(rd, z);
                for (int l = 0; l < 3; ++l) {
                    const int m = kMergeBandSize[l], o = kMergeBandMatrix[l], c0 = kMergeBandCoeff[l];
                    for (int k = 0; k < m; ++k) {
                        double s = 0.0;
                        for (int j = 0; j < m; ++j) s += M[o + j * m + k] * z[c0 + j];
                        prop = fmax(prop, fabs(s - y[c0 + k]));
                    }
                }
            }
            printf("\northo %.3g\nprop %.3g\n", ortho, prop);
        } else if (sscanf(line, "comp %x %x %x %x %x %x %x %x", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5], &u[6], &u[7]) == 8) {
            const float q1[4] = {bits_float(u[0]), bits_float(u[1]), bits_float(u[2]), bits_float(u[3])};
            const float q2[4] = {bits_float(u[4]), bits_float(u[5]), bits_float(u[6]), bits_float(u[7])};
            double a[4], b[4], M1[kMergeShFloats], M2[kMergeShFloats], M12[kMergeShFloats];
            merge_unit_quat(q1, a);
            merge_unit_quat(q2, b);
            // the quaternion product a b (x, y, z, w): the rotation R(a) R(b)
            const double ab[4] = {a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                                  a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]};
            merge_sh_matrices_f64(a, M1);
            merge_sh_matrices_f64(b, M2);
            merge_sh_matrices_f64(ab, M12);
            double worst = 0.0;
            for (int l = 0; l < 3; ++l) {
                double prod[49];
                band_mul(M1, M2, l, prod);
                for (int k = 0; k < kMergeBandSize[l] * kMergeBandSize[l]; ++k) worst = fmax(worst, fabs(prod[k] - M12[kMergeBandMatrix[l] + k]));
            }
            printf("comp %.3g\n", worst);
        } else if (sscanf(line, "joint %llu %llu %llu %llu", &a0, &a1, &a2, &a3) == 4) {
            if (a0 != a1) {
                fprintf(stderr, "joint: the first source ends where the second starts\n");
                return 2;
            }
            const uint64_t off[2] = {0, a0}, count[2] = {a1, a2}, total = a1 + a2;
            std::vector<std::vector<uint8_t>> bits(2);
            uint32_t lcg = (uint32_t)a3 * 2654435761u + 12345u;
            for (int s = 0; s < 2; ++s)
                for (uint64_t j = 0; j < count[s]; ++j) {
                    lcg = lcg * 1664525u + 1013904223u;
                    bits[s].push_back((lcg >> 16) & 1u);
                }
            std::vector<uint32_t> plane[2];
            for (int order = 0; order < 2; ++order) {
                plane[order].assign((size_t)((total + 31) / 32), 0u);  // exactly the plane: a word index past it is a sanitizer report
                for (int pass = 0; pass < 2; ++pass) {
                    const int s = order ? 1 - pass : pass;
                    for (uint64_t j = 0; j < count[s]; ++j)
                        if (bits[s][(size_t)j]) plane[order].at((size_t)merge_bit_word(off[s], j)) |= merge_bit_mask(off[s], j);
                }
            }
            if (plane[0] != plane[1]) {
                fprintf(stderr, "joint: the order of the sources changed the plane\n");
                return 2;
            }
            printf("bits ");
            for (int s = 0; s < 2; ++s)
                for (uint8_t b : bits[s]) putchar(b ? '1' : '0');
            printf("\nwords");
            for (uint32_t w : plane[0]) printf(" %x", w);
            printf("\nshared %d\n", merge_joint_shared(off[1]) ? 1 : 0);
        } else if (sscanf(line, "ident %x %x %x %x %x %x %x %x %x %x", &u[0], &u[1], &u[2], &u[3], &u[4], &u[5], &u[6], &u[7], &u[8], &u[9]) == 10) {
            const float p[3] = {bits_float(u[0]), bits_float(u[1]), bits_float(u[2])};
            const float q[4] = {bits_float(u[3]), bits_float(u[4]), bits_float(u[5]), bits_float(u[6])};
            const float s[3] = {bits_float(u[7]), bits_float(u[8]), bits_float(u[9])};
            printf("ident %d\nvalid %d\n", merge_is_identity(p, q, s) ? 1 : 0, merge_is_valid(p, q, s) ? 1 : 0);
        } else if (line[0] != '\n') {
            fprintf(stderr, "unknown command: %s", line);
            return 2;
        }
    }
    return 0;
}
