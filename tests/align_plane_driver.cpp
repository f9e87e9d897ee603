// align_plane_driver.cpp — csrc/align_plane_math.h (and, through it, csrc/align_math.h) played on the host, for
// tests/test_align_plane_cpu.py and tests/test_gpu_align_plane.py: a stand-alone program the tests build with the address and
// undefined-behaviour sanitizers and -ffp-contract=off and run as a child process (spec §27).  The sums are k_nearest_align_plane's,
// term for term, added in plain index order; the solve is the library's own header, not a restatement.  A float32 crosses as the hex
// of its 32 bits, a double as the hex of its 64 bits.  stdin, one command a line:
//   "step <max_variation> <12 matrix words> <m> <m rows of 10 float words: q x y z, t x y z, n x y z, variation>"
//        the rows are the FOUND pairs in index order, q already mapped; the matrix is only composed with the delta.
//        stdout "sums <pairs used> <left out> <38 doubles: sum q (3), centre (3), A (21), b (6), sum e^2, sum d2, rms_before, rms_plane_before>"
//               "solve <rank> <degenerate> <22 doubles: pos (3), quat (4), eigenvalues (6), centre (3), x (6)> <12 float words: xform_next>"
//   "solve <12 matrix words> <pairs used> <30 doubles: centre (3), A (21), b (6)>; every word hex"   stdout the "solve" line alone
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "align_plane_math.h"
#include "neighbors_math.h"

using namespace gsx;

static double f64(uint64_t bits) {
    double d;
    memcpy(&d, &bits, 8);
    return d;
}
static uint64_t bits64(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}
static uint32_t bits32(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

static void print_solve(const AlignPlaneSums& s, const float xform[12]) {
    const AlignPlaneDelta d = align_plane_solve(s);
    float next[12];
    if (d.delta.degenerate) {
        for (int k = 0; k < 12; ++k) next[k] = xform[k];
    } else {
        align_compose(d.delta, xform, next);
    }
    printf("solve %u %d", d.rank, (int)d.delta.degenerate);
    for (int k = 0; k < 3; ++k) printf(" %" PRIx64, bits64(d.delta.pos[k]));
    for (int k = 0; k < 4; ++k) printf(" %" PRIx64, bits64(d.delta.quat[k]));
    for (int k = 0; k < 6; ++k) printf(" %" PRIx64, bits64(d.eigenvalues[k]));
    for (int k = 0; k < 3; ++k) printf(" %" PRIx64, bits64(d.centre[k]));
    for (int k = 0; k < 6; ++k) printf(" %" PRIx64, bits64(d.x[k]));
    for (int k = 0; k < 12; ++k) printf(" %x", bits32(next[k]));
    printf("\n");
}

int main() {
    std::string line;
    for (int c; (c = getchar()) != EOF;) {
        if (c != '\n') {
            line.push_back((char)c);
            continue;
        }
        std::vector<uint64_t> w;
        char* save = nullptr;
        char* tok = strtok_r(&line[0], " ", &save);
        const std::string cmd = tok ? tok : "";
        while ((tok = strtok_r(nullptr, " ", &save))) w.push_back(strtoull(tok, nullptr, 16));
        if (cmd == "step" && w.size() >= 14 && w.size() == 14 + (size_t)w[13] * 10) {
            const float max_variation = nb_from_bits((uint32_t)w[0]);
            float xform[12];
            for (int k = 0; k < 12; ++k) xform[k] = nb_from_bits((uint32_t)w[1 + k]);
            const size_t m = (size_t)w[13];
            std::vector<float> rows(m * 10);
            for (size_t j = 0; j < m * 10; ++j) rows[j] = nb_from_bits((uint32_t)w[14 + j]);
            const auto used = [&](const float* r) { return r[9] < INFINITY && !(max_variation > 0.0f && !(r[9] <= max_variation)); };
            // pass 0
            double pairs = 0.0, left_out = 0.0, sum_q[3] = {0, 0, 0};
            for (size_t j = 0; j < m; ++j) {
                const float* r = &rows[j * 10];
                if (!used(r)) {
                    left_out += 1.0;
                    continue;
                }
                pairs += 1.0;
                for (int a = 0; a < 3; ++a) sum_q[a] += (double)r[a];
            }
            AlignPlaneSums s;
            s.n = pairs;
            float cf[3];
            for (int a = 0; a < 3; ++a) {
                s.centre[a] = align_plane_centre(sum_q[a], pairs);
                cf[a] = (float)s.centre[a];
            }
            // pass 1
            for (size_t j = 0; j < m; ++j) {
                const float* r = &rows[j * 10];
                if (!used(r)) continue;
                double d[3], g[3], J[6];
                for (int a = 0; a < 3; ++a) {
                    d[a] = (double)(r[a] - cf[a]);
                    g[a] = (double)(r[a] - r[3 + a]);
                    J[3 + a] = (double)r[6 + a];
                }
                J[0] = d[1] * J[5] - d[2] * J[4];
                J[1] = d[2] * J[3] - d[0] * J[5];
                J[2] = d[0] * J[4] - d[1] * J[3];
                const double e = (g[0] * J[3] + g[1] * J[4]) + g[2] * J[5];
                int at = 0;
                for (int p = 0; p < 6; ++p)
                    for (int q = p; q < 6; ++q) s.A[at++] += J[p] * J[q];
                for (int p = 0; p < 6; ++p) s.b[p] += J[p] * e;
                s.sum_e2 += e * e;
                s.sum_d2 += (double)nb_d2(r[0], r[1], r[2], r[3], r[4], r[5]);
            }
            printf("sums %" PRIu64 " %" PRIu64, (uint64_t)pairs, (uint64_t)left_out);
            for (int a = 0; a < 3; ++a) printf(" %" PRIx64, bits64(sum_q[a]));
            for (int a = 0; a < 3; ++a) printf(" %" PRIx64, bits64(s.centre[a]));
            for (uint32_t k = 0; k < kAlignPlaneTri; ++k) printf(" %" PRIx64, bits64(s.A[k]));
            for (int k = 0; k < 6; ++k) printf(" %" PRIx64, bits64(s.b[k]));
            printf(" %" PRIx64 " %" PRIx64, bits64(s.sum_e2), bits64(s.sum_d2));
            printf(" %" PRIx64 " %" PRIx64 "\n", bits64(pairs > 0.0 ? sqrt(s.sum_d2 / pairs) : 0.0), bits64(pairs > 0.0 ? sqrt(s.sum_e2 / pairs) : 0.0));
            print_solve(s, xform);
        } else if (cmd == "solve" && w.size() == 12 + 1 + 30) {
            float xform[12];
            for (int k = 0; k < 12; ++k) xform[k] = nb_from_bits((uint32_t)w[k]);
            AlignPlaneSums s;
            s.n = (double)w[12];
            for (int k = 0; k < 3; ++k) s.centre[k] = f64(w[13 + k]);
            for (uint32_t k = 0; k < kAlignPlaneTri; ++k) s.A[k] = f64(w[16 + k]);
            for (int k = 0; k < 6; ++k) s.b[k] = f64(w[37 + k]);
            print_solve(s, xform);
        } else {
            fprintf(stderr, "align_plane_driver: bad command '%s' with %zu words\n", cmd.c_str(), w.size());
            return 2;
        }
        line.clear();
    }
    return 0;
}
