// nearest_driver.cpp — csrc/nearest_math.h, csrc/align_math.h, csrc/knn_math.h and csrc/neighbors_math.h played on the host through a
// plain C++ version of the whole nearest search across models (spec §23), for tests/test_nearest_cpu.py: a stand-alone program the
// test builds with the address and undefined-behaviour sanitizers and -ffp-contract=off.  The loop over the rounds is the library's
// own, not a restatement: csrc/radius_search.h, which gsx_api_nearest.cpp runs, derives the radius floor and the first radius under
// the max_distance cap, rebuilds the grid, says which round is final, decides when the unresolved go to the exact fallback and counts
// the rounds.  This file supplies the work (but for one input of two rules that choose a path and no result: the first radius and
// knn_coarse take the targets' whole box here, where the device hands the loop the 10 permille trimmed box of the bounds passes;
// tests/test_gpu_nearest.py covers a box that is a point): the queries mapped by the matrix, the targets' extent, section 18's hashed
// grid over the targets by a counting sort (grid_replay.h), a round of one query an entry over 27 cells from its SIGNED cell with the
// own-cell test, the best (d2, index) pair and the proven rule under the cap, the unresolved list, and the fallback as 256 strided
// lanes folded by the key (d2 bits << 32) | index.  Every float crosses as the hex of its bits.  stdin, one command a line (hex words):
//   "search <max_distance> <hint> <grid_bits> <max_rounds> <n queries> <12 matrix words> <query x y z> ... <target x y z> ..."
//        stdout "search <queries that participate> <targets> <rounds> <n_brute> <first radius> <indices that differ from the O(n m) loop>
//                <d2 that differ> <signed cells seen: bit 0: -2, bit 1: -1, bit 2: 0, bit 3: the clamp>"
//               "index <n values>"  "d2 <n values>"
//   "cell <x> <origin> <inv_h>"     stdout "cell <nb_cell_signed as a decimal>"
//   "matrix <src pos[3] quat[4] scale[3]> <dst pos[3] quat[4] scale[3]>"   stdout "matrix <12 words>": nearest_model_matrix
//   "align <with_scale> <n> <q x y z> ... <t x y z> ..."
//        stdout "align <degenerate> <quat x y z w> <scale> <pos x y z>" as decimals (%.17g): the device's sums, then align_solve
//   "compose <quat x y z w> <scale> <pos x y z> <12 matrix words>"   stdout "compose <12 words>": align_compose of a float32 delta
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "align_math.h"
#include "grid_replay.h"
#include "knn_math.h"
#include "nearest_math.h"
#include "neighbors_math.h"
#include "radius_search.h"

using namespace gsx;

static uint32_t g_cells_seen = 0;
static void see_cell(int32_t c) {
    if (c == -2) g_cells_seen |= 1u;
    if (c == -1) g_cells_seen |= 2u;
    if (c == 0) g_cells_seen |= 4u;
    if (c == (int32_t)kNbMaxCell) g_cells_seen |= 8u;
}

// k_nearest_query's lane: true where the row is proven (best, best_index hold it; best_index none: nothing within the reach)
static bool query_entry(const Grid& gr, const Rec& self, float cap2, float& best, uint32_t& best_index) {
    const float reach2 = nearest_reach2(gr.g.r2, cap2), inv_h = gr.g.inv_h;
    const int32_t cx = nb_cell_signed(self.x, gr.origin[0], inv_h), cy = nb_cell_signed(self.y, gr.origin[1], inv_h), cz = nb_cell_signed(self.z, gr.origin[2], inv_h);
    see_cell(cx);
    see_cell(cy);
    see_cell(cz);
    best = INFINITY;
    best_index = kNearestNone;
    if (cx > -2 && cy > -2 && cz > -2) {
        for (uint32_t c = 0; c < 27u; ++c) {
            const uint32_t vx = (uint32_t)cx + (c % 3u) - 1u, vy = (uint32_t)cy + ((c / 3u) % 3u) - 1u, vz = (uint32_t)cz + (c / 9u) - 1u;
            if (vx > kNbMaxCell || vy > kNbMaxCell || vz > kNbMaxCell) continue;
            const uint32_t bucket = nb_bucket(vx, vy, vz, gr.bits);
            uint32_t q = bucket ? gr.ends[bucket - 1u] : 0u;
            const uint32_t end = gr.ends[bucket];
            for (; q < end; ++q) {
                const Rec& r = gr.records[q];
                const float d2 = nb_d2(self.x, self.y, self.z, r.x, r.y, r.z);
                if (d2 <= reach2 && nearest_better(d2, r.index, best, best_index) && nb_cell(r.x, gr.origin[0], inv_h) == vx && nb_cell(r.y, gr.origin[1], inv_h) == vy &&
                    nb_cell(r.z, gr.origin[2], inv_h) == vz) {
                    best = d2;
                    best_index = r.index;
                }
            }
        }
    }
    return best <= reach2;
}

// k_nearest_brute's workgroup
static void brute_entry(const std::vector<Rec>& records, const Rec& self, float cap2, float& best, uint32_t& best_index) {
    uint64_t key = ((uint64_t)bits_of(INFINITY) << 32) | kNearestNone;
    for (uint32_t t = 0; t < kKnnBruteLanes; ++t) {
        uint64_t mine_best = ((uint64_t)bits_of(INFINITY) << 32) | kNearestNone;
        for (size_t q = t; q < records.size(); q += kKnnBruteLanes) {
            const Rec& r = records[q];
            const float d2 = nb_d2(self.x, self.y, self.z, r.x, r.y, r.z);
            const uint64_t mine = ((uint64_t)bits_of(d2) << 32) | r.index;
            if (d2 <= cap2 && mine < mine_best) mine_best = mine;
        }
        key = std::min(key, mine_best);
    }
    best_index = (uint32_t)key;
    best = best_index == kNearestNone ? INFINITY : nb_from_bits((uint32_t)(key >> 32));
}

struct Result {
    uint32_t queries = 0, targets = 0, rounds = 0, n_brute = 0;
    float first_radius = 0.0f;
    std::vector<uint32_t> index;
    std::vector<float> d2;
};

static bool finite3(float x, float y, float z) { return nb_finite(x) && nb_finite(y) && nb_finite(z); }

static void mapped(const float* m, const std::vector<float>& qpos, std::vector<Rec>& out) {
    for (size_t i = 0; i < qpos.size() / 3; ++i) {
        const float x = qpos[3 * i], y = qpos[3 * i + 1], z = qpos[3 * i + 2];
        const Rec q{nearest_map_row(m + 0, x, y, z), nearest_map_row(m + 4, x, y, z), nearest_map_row(m + 8, x, y, z), (uint32_t)i};
        if (finite3(x, y, z) && finite3(q.x, q.y, q.z)) out.push_back(q);
    }
}

static void search(const float* m, const std::vector<float>& qpos, const std::vector<float>& tpos, float max_distance, float hint, uint32_t grid_bits,
                   uint32_t max_rounds, Result& out) {
    const size_t n = qpos.size() / 3, n_dst = tpos.size() / 3;
    out.index.assign(n, kNearestNone);
    out.d2.assign(n, INFINITY);
    std::vector<Rec> list[2], part;
    mapped(m, qpos, list[1]);
    std::reverse(list[1].begin(), list[1].end());  // (the first list's order is free)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < n_dst; ++i) {
        const Rec r{tpos[3 * i], tpos[3 * i + 1], tpos[3 * i + 2], (uint32_t)i};
        if (!finite3(r.x, r.y, r.z)) continue;
        part.push_back(r);
        mn[0] = fminf(mn[0], r.x); mn[1] = fminf(mn[1], r.y); mn[2] = fminf(mn[2], r.z);
        mx[0] = fmaxf(mx[0], r.x); mx[1] = fmaxf(mx[1], r.y); mx[2] = fmaxf(mx[2], r.z);
    }
    const uint32_t P = (uint32_t)part.size();
    out.queries = (uint32_t)list[1].size();
    out.targets = P;
    if (!P || list[1].empty()) return;
    const float cap2 = nearest_cap2(max_distance);
    RadiusSearch s{{}, {}, P, hint, 1u, max_distance, max_rounds};
    for (int a = 0; a < 3; ++a) s.ext[a] = s.trimmed[a] = (double)mx[a] - (double)mn[a];
    const uint32_t bits = grid_bits ? grid_bits : nb_auto_bits(n_dst);
    Grid gr;
    const std::vector<Rec>* src = &list[1];  // the first list: the mapped queries
    const auto store = [&](const Rec& self, float best, uint32_t best_index) {
        out.index[self.index] = best_index;
        out.d2[self.index] = best;
    };
    const auto grid = [&](float r, bool) {
        if (!nb_radius_ok(r)) abort();
        gr = build_grid(part, r, bits);
        return false;
    };
    const auto round = [&](uint32_t i, uint32_t U, bool final_round, uint32_t* left) {
        std::vector<Rec>& next = list[i & 1u];  // (round 0 reads list[1]: every round reads the list the one before wrote)
        next.clear();
        for (const Rec& self : *src) {
            float best;
            uint32_t best_index;
            if (query_entry(gr, self, cap2, best, best_index))
                store(self, best, best_index);
            else if (!final_round)
                next.push_back(self);
        }
        std::reverse(next.begin(), next.end());  // (the list's order is free)
        *left = (uint32_t)next.size();
        src = &next;
        return false;
    };
    const auto brute = [&](uint32_t) {
        for (const Rec& self : *src) {
            float best;
            uint32_t best_index;
            brute_entry(gr.records, self, cap2, best, best_index);
            if (best_index != kNearestNone) store(self, best, best_index);
        }
        return false;
    };
    radius_search<bool>(s, out.queries, grid, round, brute);
    out.first_radius = s.first_radius;
    out.rounds = s.rounds;
    out.n_brute = s.n_brute;
}

// the definition: every pair, the least (d2, index) within the cap
static void definition(const float* m, const std::vector<float>& qpos, const std::vector<float>& tpos, float max_distance, Result& out) {
    const size_t n = qpos.size() / 3, n_dst = tpos.size() / 3;
    out.index.assign(n, kNearestNone);
    out.d2.assign(n, INFINITY);
    std::vector<Rec> list;
    mapped(m, qpos, list);
    const float cap2 = nearest_cap2(max_distance);
    for (const Rec& q : list) {
        for (size_t j = 0; j < n_dst; ++j) {
            if (!finite3(tpos[3 * j], tpos[3 * j + 1], tpos[3 * j + 2])) continue;
            const float d2 = nb_d2(q.x, q.y, q.z, tpos[3 * j], tpos[3 * j + 1], tpos[3 * j + 2]);
            if (d2 <= cap2 && d2 < out.d2[q.index]) {  // (ascending j: the first of equal values is the smallest index)
                out.d2[q.index] = d2;
                out.index[q.index] = (uint32_t)j;
            }
        }
    }
}

// the sums as k_nearest_align takes them (the order of the additions aside)
static AlignSums sums_of(const std::vector<float>& q, const std::vector<float>& t) {
    AlignSums s;
    const size_t n = q.size() / 3;
    s.n = (double)n;
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            s.sum_q[a] += (double)q[3 * i + a];
            s.sum_t[a] += (double)t[3 * i + a];
        }
    float qm[3] = {0, 0, 0}, tm[3] = {0, 0, 0};
    for (int a = 0; a < 3 && n; ++a) {
        qm[a] = (float)(s.sum_q[a] / s.n);
        tm[a] = (float)(s.sum_t[a] / s.n);
    }
    for (size_t i = 0; i < n; ++i) {
        double dq[3], dt[3];
        for (int a = 0; a < 3; ++a) {
            dq[a] = (double)(q[3 * i + a] - qm[a]);
            dt[a] = (double)(t[3 * i + a] - tm[a]);
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) s.H[3 * a + b] += dq[a] * dt[b];
        s.spread_q += (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
        s.spread_t += (dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2];
    }
    return s;
}

int main() {
    std::string line;
    for (int c; (c = getchar()) != EOF;) {
        if (c != '\n') {
            line.push_back((char)c);
            continue;
        }
        const size_t space = line.find(' ');
        const std::string cmd = line.substr(0, space);
        const std::vector<uint32_t> w = words(space == std::string::npos ? "" : line.c_str() + space);
        if (cmd == "search" && w.size() >= 17 && (w.size() - 17) % 3 == 0 && (size_t)w[4] * 3 <= w.size() - 17) {
            float m[12];
            for (int k = 0; k < 12; ++k) m[k] = nb_from_bits(w[5 + k]);
            std::vector<float> qpos, tpos;
            for (size_t j = 17; j < w.size(); ++j) (j < 17 + (size_t)w[4] * 3 ? qpos : tpos).push_back(nb_from_bits(w[j]));
            Result got, want;
            g_cells_seen = 0;
            search(m, qpos, tpos, nb_from_bits(w[0]), nb_from_bits(w[1]), w[2], w[3], got);
            definition(m, qpos, tpos, nb_from_bits(w[0]), want);
            size_t bad_index = 0, bad_d2 = 0;
            for (size_t j = 0; j < got.index.size(); ++j) {
                bad_index += got.index[j] != want.index[j];
                bad_d2 += bits_of(got.d2[j]) != bits_of(want.d2[j]);
            }
            printf("search %u %u %u %u %x %zu %zu %u\nindex", got.queries, got.targets, got.rounds, got.n_brute, bits_of(got.first_radius), bad_index, bad_d2, g_cells_seen);
            for (uint32_t v : got.index) printf(" %x", v);
            printf("\nd2");
            for (float v : got.d2) printf(" %x", bits_of(v));
            printf("\n");
        } else if (cmd == "cell" && w.size() == 3) {
            printf("cell %d\n", (int)nb_cell_signed(nb_from_bits(w[0]), nb_from_bits(w[1]), nb_from_bits(w[2])));
        } else if (cmd == "matrix" && w.size() == 20) {
            float v[20], out[12];
            for (int k = 0; k < 20; ++k) v[k] = nb_from_bits(w[k]);
            nearest_model_matrix(v, v + 3, v + 7, v + 10, v + 13, v + 17, out);
            printf("matrix");
            for (float x : out) printf(" %x", bits_of(x));
            printf("\n");
        } else if (cmd == "align" && w.size() >= 2 && w.size() == 2 + (size_t)w[1] * 6) {
            std::vector<float> q, t;
            for (size_t j = 2; j < w.size(); ++j) (j < 2 + (size_t)w[1] * 3 ? q : t).push_back(nb_from_bits(w[j]));
            const AlignDelta d = align_solve(sums_of(q, t), w[0] != 0u);
            printf("align %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", (int)d.degenerate, d.quat[0], d.quat[1], d.quat[2], d.quat[3], d.scale, d.pos[0],
                   d.pos[1], d.pos[2]);
        } else if (cmd == "compose" && w.size() == 20) {
            AlignDelta d;
            for (int k = 0; k < 4; ++k) d.quat[k] = (double)nb_from_bits(w[k]);
            d.scale = (double)nb_from_bits(w[4]);
            for (int k = 0; k < 3; ++k) d.pos[k] = (double)nb_from_bits(w[5 + k]);
            float m[12], out[12];
            for (int k = 0; k < 12; ++k) m[k] = nb_from_bits(w[8 + k]);
            align_compose(d, m, out);
            printf("compose");
            for (float x : out) printf(" %x", bits_of(x));
            printf("\n");
        } else {
            printf("? %s\n", cmd.c_str());
        }
        line.clear();
    }
    return 0;
}
