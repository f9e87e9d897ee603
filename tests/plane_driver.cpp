// plane_driver.cpp — csrc/plane_math.h played on the host, for tests/test_plane_cpu.py and tests/test_gpu_plane.py: a stand-alone
// program the tests build with the address and undefined-behaviour sanitizers and -ffp-contract=off and run as a child process (spec
// §28).  The hash, the probe, the candidates, the inlier rule, the solve and gsx_plane_level's arithmetic are the library's own header,
// not a restatement; the counts and the moments are the kernels' terms added in plain index order.  A float32 crosses as the hex of
// its 32 bits, a double and a 64-bit integer as the hex of their 64 bits.  stdin, one command a line, every word hex:
//   "mix <seed> <h> <s> <t>"                                  stdout "mix <64 bits>"
//   "fit <sample> <seed> <H> <tolerance> <min_cos> <n> <n rows of 8 words: x y z, participates 0 / 1, kept normal x y z, variation>
//        [CALLER: <H planes of 4 words>]"
//        stdout H lines "cand <valid> <slot 0> <slot 1> <slot 2> <4 plane words as reported> <count>", then "winner <h or ffffffff>"
//   "moments <4 plane words> <tolerance> <min_cos> <n> <n rows as above>"
//        stdout "moments <11 doubles: count, sum p (3), sum r^2, scatter (6)>" over the plane's inliers
//   "solve <orient> <3 toward words> <10 doubles: count, sum p (3), scatter (6)>"
//        stdout "solve <ok> <4 plane words> <3 centre words> <3 doubles: eigenvalues>"
//   "level <4 plane words> <3 up words>"                       stdout "level <ok> <7 doubles: quat (4), pos (3)>"
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "plane_math.h"

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
static float f32(uint64_t bits) { return nb_from_bits((uint32_t)bits); }
static uint32_t bits32(float f) { return nm_bits(f); }

struct Row {
    float p[3];
    bool part;
    float k[3];
    float variation;
};
static std::vector<Row> rows_at(const std::vector<uint64_t>& w, size_t at, size_t n) {
    std::vector<Row> rows(n);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t* r = &w[at + 8 * i];
        rows[i] = Row{{f32(r[0]), f32(r[1]), f32(r[2])}, r[3] != 0, {f32(r[4]), f32(r[5]), f32(r[6])}, f32(r[7])};
    }
    return rows;
}
static bool row_inlier(const Plane& pl, const Row& r, float tolerance, float min_cos) {
    if (!r.part || !pl_inlier(pl_residual(pl, r.p[0], r.p[1], r.p[2]), tolerance)) return false;
    return !(min_cos > 0.0f) || pl_facing(pl, r.k[0], r.k[1], r.k[2], r.variation, min_cos);
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
        line.clear();
        if (cmd == "mix" && w.size() == 4) {
            printf("mix %" PRIx64 "\n", pl_mix(w[0], (uint32_t)w[1], (uint32_t)w[2], (uint32_t)w[3]));
        } else if (cmd == "fit" && w.size() >= 6) {
            const uint32_t sample = (uint32_t)w[0], H = (uint32_t)w[2];
            const uint64_t seed = w[1];
            const float tolerance = f32(w[3]), min_cos = f32(w[4]);
            const size_t n = (size_t)w[5];
            if (H < 1 || H > kPlaneMaxCandidates || w.size() != 6 + 8 * n + (sample == kPlaneSampleCaller ? 4 * (size_t)H : 0)) return 2;
            const std::vector<Row> rows = rows_at(w, 6, n);
            std::vector<uint32_t> counts(H, 0u), valid(H, 0u);
            for (uint32_t h = 0; h < H; ++h) {
                Plane pl = pl_invalid();
                uint32_t slot[3] = {kPlaneNone, kPlaneNone, kPlaneNone};
                bool ok = false;
                if (sample == kPlaneSampleCaller) {
                    const uint64_t* q = &w[6 + 8 * n + 4 * (size_t)h];
                    pl = Plane{{f32(q[0]), f32(q[1]), f32(q[2])}, f32(q[3])};
                    ok = pl_caller_ok(pl);
                } else if (sample == kPlaneSampleNormals) {
                    slot[0] = pl_probe(seed, h, 0u, n, [&](uint32_t j) { return rows[j].part && nm_is_fitted(rows[j].variation); });
                    if (slot[0] != kPlaneNone) {
                        pl = pl_from_normal(rows[slot[0]].p, rows[slot[0]].k);
                        ok = true;
                    }
                } else {
                    for (uint32_t s = 0; s < 3u; ++s) slot[s] = pl_probe(seed, h, s, n, [&](uint32_t j) { return (bool)rows[j].part; });
                    if (slot[0] != kPlaneNone && slot[1] != kPlaneNone && slot[2] != kPlaneNone && slot[0] != slot[1] && slot[0] != slot[2] && slot[1] != slot[2])
                        ok = pl_from_triple(rows[slot[0]].p, rows[slot[1]].p, rows[slot[2]].p, &pl);
                }
                if (!ok) pl = pl_invalid();
                valid[h] = ok ? 1u : 0u;
                for (size_t i = 0; i < n; ++i) counts[h] += row_inlier(pl, rows[i], tolerance, min_cos) ? 1u : 0u;
                if (!ok) pl = Plane{{0.0f, 0.0f, 0.0f}, 0.0f};
                printf("cand %u %x %x %x %x %x %x %x %x\n", valid[h], slot[0], slot[1], slot[2], bits32(pl.n[0]), bits32(pl.n[1]), bits32(pl.n[2]), bits32(pl.offset),
                       counts[h]);
            }
            printf("winner %x\n", pl_winner(counts.data(), valid.data(), H));
        } else if (cmd == "moments" && w.size() >= 7) {
            const Plane pl{{f32(w[0]), f32(w[1]), f32(w[2])}, f32(w[3])};
            const float tolerance = f32(w[4]), min_cos = f32(w[5]);
            const size_t n = (size_t)w[6];
            if (w.size() != 7 + 8 * n) return 2;
            const std::vector<Row> rows = rows_at(w, 7, n);
            PlaneSums s;
            for (const Row& r : rows) {
                if (!row_inlier(pl, r, tolerance, min_cos)) continue;
                const float res = pl_residual(pl, r.p[0], r.p[1], r.p[2]);
                s.count += 1.0;
                for (int a = 0; a < 3; ++a) s.sum_p[a] += (double)r.p[a];
                s.sum_r2 += (double)res * (double)res;
            }
            float c[3];
            for (int a = 0; a < 3; ++a) c[a] = pl_centre(s.sum_p[a], s.count);
            for (const Row& r : rows) {
                if (!row_inlier(pl, r, tolerance, min_cos)) continue;
                const double d[3] = {(double)(r.p[0] - c[0]), (double)(r.p[1] - c[1]), (double)(r.p[2] - c[2])};
                s.scatter[0] += d[0] * d[0];
                s.scatter[1] += d[0] * d[1];
                s.scatter[2] += d[0] * d[2];
                s.scatter[3] += d[1] * d[1];
                s.scatter[4] += d[1] * d[2];
                s.scatter[5] += d[2] * d[2];
            }
            printf("moments %" PRIx64, bits64(s.count));
            for (int a = 0; a < 3; ++a) printf(" %" PRIx64, bits64(s.sum_p[a]));
            printf(" %" PRIx64, bits64(s.sum_r2));
            for (int a = 0; a < 6; ++a) printf(" %" PRIx64, bits64(s.scatter[a]));
            printf("\n");
        } else if (cmd == "solve" && w.size() == 14) {
            const float toward[3] = {f32(w[1]), f32(w[2]), f32(w[3])};
            PlaneSums s;
            s.count = f64(w[4]);
            for (int a = 0; a < 3; ++a) s.sum_p[a] = f64(w[5 + a]);
            for (int a = 0; a < 6; ++a) s.scatter[a] = f64(w[8 + a]);
            const PlaneFit f = pl_solve(s, (uint32_t)w[0], toward);
            printf("solve %d %x %x %x %x %x %x %x", (int)f.ok, bits32(f.plane.n[0]), bits32(f.plane.n[1]), bits32(f.plane.n[2]), bits32(f.plane.offset), bits32(f.centre[0]),
                   bits32(f.centre[1]), bits32(f.centre[2]));
            for (int a = 0; a < 3; ++a) printf(" %" PRIx64, bits64(f.eigenvalues[a]));
            printf("\n");
        } else if (cmd == "level" && w.size() == 7) {
            const Plane pl{{f32(w[0]), f32(w[1]), f32(w[2])}, f32(w[3])};
            const float up[3] = {f32(w[4]), f32(w[5]), f32(w[6])};
            double q[4] = {0, 0, 0, 0}, p[3] = {0, 0, 0};
            const bool ok = pl_level(pl, up, q, p);
            printf("level %d", (int)ok);
            for (int a = 0; a < 4; ++a) printf(" %" PRIx64, bits64(q[a]));
            for (int a = 0; a < 3; ++a) printf(" %" PRIx64, bits64(p[a]));
            printf("\n");
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
