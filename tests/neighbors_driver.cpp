// neighbors_driver.cpp — csrc/neighbors_math.h (the grid, the cell of a coordinate and the bucket of a cell of the neighbour counts,
// spec §18) played on the host, for tests/test_neighbors_cpu.py: a stand-alone program the test builds with the address and
// undefined-behaviour sanitizers and -ffp-contract=off.  Every float crosses as the hex of its bits.  stdin, one command a line:
//   "grid <radius>"                       stdout "grid <ok 0|1> <r2> <h> <inv_h>"; sets the grid of what follows
//   "cells <bits> <ox oy oz> <x y z> ..." stdout "cells <cx cy cz bucket> ..." (decimal): nb_cell per axis and nb_bucket of every point
//   "auto <n> ..."                        stdout "auto <bits> ..." : nb_auto_bits
//   "pairs <seed> <rounds>"               generates pairs of points under the current grid and, for every pair with d2 <= r2, checks
//                                         that the cells of the two differ by at most 1 per axis, under several origins at or below
//                                         both; stdout "pairs <generated> <near> <exactly r2> <clamped> <violations>"
// The generated pairs: coordinates on exact multiples of the radius and of the cell edge, around zero on both sides, near the clamp
// (cell 32767) and past it, at 1e6 radii and at 3e38; offsets along one axis of exactly the radius, of one ulp either side of it,
// random inside the ball, random on its surface, and none (coincident).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "grid_replay.h"
#include "neighbors_math.h"

using namespace gsx;

struct Rng {
    uint64_t s;
    uint32_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)(s >> 16);
    }
    float unit() { return (float)(next() >> 8) / 16777216.0f; }       // [0, 1)
    float sym() { return unit() * 2.0f - 1.0f; }                       // [-1, 1)
    int32_t range(int32_t lo, int32_t hi) { return lo + (int32_t)(next() % (uint32_t)(hi - lo + 1)); }
};

// one coordinate of the first point of a pair
static float base_coord(Rng& g, const NbGrid& grid, float radius, uint32_t kind) {
    switch (kind) {
        case 0: return (float)g.range(-40000, 40000) * radius;            // exact multiples of the radius
        case 1: return (float)g.range(-40000, 40000) * grid.h;            // exact multiples of the cell edge
        case 2: return g.sym() * 100.0f * radius;                         // around zero, both signs
        case 3: return (float)g.range(32760, 32775) * grid.h * (g.next() & 1u ? 1.0f : -1.0f) + g.sym() * radius;  // at the clamp
        case 4: return g.sym() * 1.0e6f * radius;                         // far beyond it
        case 5: return g.sym() * 3.0e38f;                                 // the largest magnitudes
        default: return g.sym() * radius;                                 // within one cell of zero
    }
}

int main() {
    float radius = 1.0f;
    NbGrid grid = nb_grid(radius);
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        line = buf;
        while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof buf, stdin)) line += buf;
        const char* s = line.c_str();
        char cmd[32] = {0};
        int used = 0;
        if (sscanf(s, "%31s%n", cmd, &used) != 1) continue;
        s += used;
        if (!strcmp(cmd, "grid")) {
            const std::vector<uint32_t> w = words(s);
            if (w.size() != 1) return 2;
            radius = nb_from_bits(w[0]);
            const bool ok = nb_radius_ok(radius);
            if (ok) grid = nb_grid(radius);
            printf("grid %d %x %x %x\n", ok ? 1 : 0, ok ? bits_of(grid.r2) : 0u, ok ? bits_of(grid.h) : 0u, ok ? bits_of(grid.inv_h) : 0u);
        } else if (!strcmp(cmd, "cells")) {
            const std::vector<uint32_t> w = words(s);
            if (w.size() < 4 || (w.size() - 4) % 3 != 0 || w[0] < 1 || w[0] > kNbMaxBits) return 2;
            const float o[3] = {nb_from_bits(w[1]), nb_from_bits(w[2]), nb_from_bits(w[3])};
            printf("cells");
            for (size_t k = 4; k < w.size(); k += 3) {
                uint32_t c[3];
                for (int a = 0; a < 3; ++a) c[a] = nb_cell(nb_from_bits(w[k + a]), o[a], grid.inv_h);
                printf(" %u %u %u %u", c[0], c[1], c[2], nb_bucket(c[0], c[1], c[2], w[0]));
            }
            printf("\n");
        } else if (!strcmp(cmd, "auto")) {
            printf("auto");
            char* end = nullptr;
            for (;;) {
                const unsigned long long n = strtoull(s, &end, 10);
                if (end == s) break;
                printf(" %u", nb_auto_bits(n));
                s = end;
            }
            printf("\n");
        } else if (!strcmp(cmd, "pairs")) {
            unsigned long long seed = 1, rounds = 0;
            if (sscanf(s, "%llu %llu", &seed, &rounds) != 2) return 2;
            Rng g{seed * 0x9E3779B97F4A7C15ull + 1u};
            unsigned long long generated = 0, near = 0, exact = 0, clamped = 0, violations = 0;
            const float below = nextafterf(radius, 0.0f), above = nextafterf(radius, INFINITY);
            for (unsigned long long it = 0; it < rounds; ++it) {
                float a[3], b[3];
                const uint32_t kind = g.next() % 7u, offset = g.next() % 8u;
                for (int k = 0; k < 3; ++k) a[k] = base_coord(g, grid, radius, (g.next() & 3u) ? kind : g.next() % 7u);
                float d[3] = {0, 0, 0};
                if (offset < 3u) {  // along one axis: exactly the radius, or one ulp either side of it
                    const float len = offset == 0u ? radius : (offset == 1u ? below : above);
                    d[g.next() % 3u] = (g.next() & 1u) ? len : -len;
                } else if (offset < 5u) {  // inside the ball
                    const float s3 = 0.57735f * g.unit();
                    for (int k = 0; k < 3; ++k) d[k] = g.sym() * s3 * radius;
                } else if (offset < 7u) {  // on the surface, to rounding: some pass, some do not
                    float v[3], len2 = 0.0f;
                    for (int k = 0; k < 3; ++k) {
                        v[k] = g.sym();
                        len2 += v[k] * v[k];
                    }
                    const float inv = len2 > 0.0f ? radius / sqrtf(len2) : 0.0f;
                    for (int k = 0; k < 3; ++k) d[k] = v[k] * inv;
                }  // (offset 7: coincident)
                bool finite = true;
                for (int k = 0; k < 3; ++k) {
                    b[k] = a[k] + d[k];
                    finite = finite && nb_finite(a[k]) && nb_finite(b[k]);
                }
                if (!finite) continue;
                generated += 1;
                const float d2 = nb_d2(a[0], a[1], a[2], b[0], b[1], b[2]);
                if (!(d2 <= grid.r2)) continue;
                near += 1;
                if (d2 == grid.r2) exact += 1;
                for (int k = 0; k < 3; ++k) {
                    const float lo = fminf(a[k], b[k]);
                    // origins at or below both: the minimum itself, a few edges below, 1e6 radii below, the lowest float32s
                    const float origins[5] = {lo, lo - (float)g.range(0, 7) * grid.h, lo - g.unit() * 32760.0f * grid.h, lo - 1.0e6f * radius, -3.0e38f};
                    for (float o : origins) {
                        if (!(o <= lo) || !nb_finite(o)) continue;
                        const uint32_t ca = nb_cell(a[k], o, grid.inv_h), cb = nb_cell(b[k], o, grid.inv_h);
                        if (ca == kNbMaxCell || cb == kNbMaxCell) clamped += 1;
                        if ((ca > cb ? ca - cb : cb - ca) > 1u || ca > kNbMaxCell || cb > kNbMaxCell) violations += 1;
                        if ((a[k] <= b[k]) != (ca <= cb) && ca != cb) violations += 1;  // monotone
                    }
                }
            }
            printf("pairs %llu %llu %llu %llu %llu\n", generated, near, exact, clamped, violations);
        } else {
            return 3;
        }
    }
    return 0;
}
