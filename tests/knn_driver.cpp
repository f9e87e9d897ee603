// knn_driver.cpp — csrc/knn_math.h and csrc/neighbors_math.h played on the host through a plain C++ version of the whole search of the
// nearest neighbours (spec §20), for tests/test_knn_cpu.py: a stand-alone program the test builds with the address and
// undefined-behaviour sanitizers and -ffp-contract=off.  The loop over the rounds is the library's own, not a restatement:
// csrc/radius_search.h, which gsx_api_knn.cpp runs, derives the radius floor and the first radius, rebuilds the grid, decides when the
// unresolved go to the exact fallback and counts the rounds; this file supplies the work (but for one input: it hands the loop the
// whole box where the device hands it the 10 permille trimmed box of the bounds passes): section 18's hashed grid by a counting sort
// (grid_replay.h), a round of one query an entry over 27 cells with the own-cell test and the proven rule, the unresolved list, and the
// fallback as 256 strided per-lane lists merged with multiplicity by (value bits, lane).  Every float crosses as the hex of its bits.  stdin, one command a line (hex words):
//   "search <k> <score> <hint> <grid_bits> <max_rounds> <x y z> ..."
//        stdout "search <participants> <rounds> <n_brute> <first radius> <rows that differ from the O(n^2) loop> <scores that differ>"
//               "rows <n * k values>"  "scores <n values>"
//   "chain <K> <k> <v> ..."        stdout "chain <k values>": the chain's k best of the values, K in {4, 8, 16}
//   "floor <ex ey ez>"             stdout "floor <radius floor>" (the extents as float32)
//   "first <ex ey ez> <P> <k>"     stdout "first <radius>": the library's own first radius, before the clamp
//   "brute <U> <P> <rounds> <max_rounds> <next radius> <coarse>"   stdout "brute <0|1>": knn_go_brute
//   "coarse <next radius> <ex ey ez>"   stdout "coarse <0|1>": knn_coarse
//   "threshold <mean lo> <mean hi> <std lo> <std hi> <ratio>"  stdout "threshold <value>" (the doubles as two words, low first)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "grid_replay.h"
#include "knn_math.h"
#include "neighbors_math.h"
#include "radius_search.h"

using namespace gsx;

static double double_of(uint32_t lo, uint32_t hi) {
    const uint64_t u = ((uint64_t)hi << 32) | lo;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// k_knn_query's lane: true where the row is proven (b holds it)
template <int K>
static bool query_entry(const Grid& gr, const Rec& self, uint32_t k, float (&b)[K]) {
    const float r2 = gr.g.r2, inv_h = gr.g.inv_h;
    const uint32_t cx = nb_cell(self.x, gr.origin[0], inv_h), cy = nb_cell(self.y, gr.origin[1], inv_h), cz = nb_cell(self.z, gr.origin[2], inv_h);
    knn_clear(b, k);
    bool full_of_zeros = false;
    for (uint32_t c = 0; c < 27u && !full_of_zeros; ++c) {
        const uint32_t vx = cx + (c % 3u) - 1u, vy = cy + ((c / 3u) % 3u) - 1u, vz = cz + (c / 9u) - 1u;
        if (vx > kNbMaxCell || vy > kNbMaxCell || vz > kNbMaxCell) continue;
        const uint32_t bucket = nb_bucket(vx, vy, vz, gr.bits);
        uint32_t q = bucket ? gr.ends[bucket - 1u] : 0u;
        const uint32_t end = gr.ends[bucket];
        for (; q < end && !full_of_zeros; ++q) {
            const Rec& r = gr.records[q];
            const float d2 = nb_d2(self.x, self.y, self.z, r.x, r.y, r.z);
            if (d2 <= r2 && r.index != self.index && d2 < knn_kth(b)) {
                if (nb_cell(r.x, gr.origin[0], inv_h) == vx && nb_cell(r.y, gr.origin[1], inv_h) == vy && nb_cell(r.z, gr.origin[2], inv_h) == vz) {
                    knn_insert(b, d2);
                    full_of_zeros = knn_kth(b) == 0.0f;
                }
            }
        }
    }
    return knn_proven(knn_kth(b), r2);
}

// k_knn_brute's workgroup
template <int K>
static void brute_entry(const std::vector<Rec>& records, const Rec& self, uint32_t k, float (&row)[K]) {
    std::vector<float> best((size_t)K * kKnnBruteLanes);
    for (uint32_t t = 0; t < kKnnBruteLanes; ++t) {
        float b[K];
        knn_clear(b, k);
        for (size_t q = t; q < records.size(); q += kKnnBruteLanes) {
            const Rec& r = records[q];
            if (r.index == self.index) continue;
            const float d2 = nb_d2(self.x, self.y, self.z, r.x, r.y, r.z);
            if (d2 < knn_kth(b)) knn_insert(b, d2);
        }
        for (int q = 0; q < K; ++q) best[(size_t)q * kKnnBruteLanes + t] = b[q];
    }
    std::vector<uint32_t> head(kKnnBruteLanes, (uint32_t)K - k);
    knn_clear(row, k);
    for (uint32_t q = (uint32_t)K - k; q < (uint32_t)K; ++q) {
        uint64_t win = ~uint64_t(0);
        for (uint32_t t = 0; t < kKnnBruteLanes; ++t) {
            const float mine = head[t] < (uint32_t)K ? best[(size_t)head[t] * kKnnBruteLanes + t] : INFINITY;
            win = std::min(win, ((uint64_t)bits_of(mine) << 32) | t);
        }
        row[q] = nb_from_bits((uint32_t)(win >> 32));
        head[(uint32_t)win] += 1u;
    }
}

struct Result {
    uint32_t participants = 0, rounds = 0, n_brute = 0;
    float first_radius = 0.0f;
    std::vector<float> rows, scores;
};

template <int K>
static void search(const std::vector<float>& pos, uint32_t k, uint32_t score, float hint, uint32_t grid_bits, uint32_t max_rounds, Result& out) {
    const size_t n = pos.size() / 3;
    out.rows.assign(n * k, INFINITY);
    out.scores.assign(n, INFINITY);
    std::vector<Rec> part;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < n; ++i) {
        const Rec r{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], (uint32_t)i};
        if (!(nb_finite(r.x) && nb_finite(r.y) && nb_finite(r.z))) continue;
        part.push_back(r);
        mn[0] = fminf(mn[0], r.x); mn[1] = fminf(mn[1], r.y); mn[2] = fminf(mn[2], r.z);
        mx[0] = fmaxf(mx[0], r.x); mx[1] = fmaxf(mx[1], r.y); mx[2] = fmaxf(mx[2], r.z);
    }
    const uint32_t P = (uint32_t)part.size();
    out.participants = P;
    RadiusSearch s{{}, {}, P, hint, k, 0.0f, max_rounds};  // (uncapped; the extents stay 0 without participants)
    for (int a = 0; a < 3 && P; ++a) s.ext[a] = s.trimmed[a] = (double)mx[a] - (double)mn[a];
    const uint32_t bits = grid_bits ? grid_bits : nb_auto_bits(n);
    Grid gr;
    std::vector<Rec> list[2];
    const std::vector<Rec>* src = &gr.records;  // the first list: the grid's records
    const auto store = [&](const Rec& self, const float (&b)[K]) {
        out.scores[self.index] = knn_score(b, k, score);
        knn_store(b, k, &out.rows[(size_t)self.index * k]);
    };
    const auto grid = [&](float r, bool final_round) {
        if (!nb_radius_ok(r) || final_round) abort();
        gr = build_grid(part, r, bits);
        return false;
    };
    const auto round = [&](uint32_t i, uint32_t U, bool, uint32_t* left) {
        std::vector<Rec>& next = list[i & 1u];
        next.clear();
        for (const Rec& self : *src) {
            float b[K];
            if (query_entry<K>(gr, self, k, b))
                store(self, b);
            else
                next.push_back(self);
        }
        std::reverse(next.begin(), next.end());  // (the list's order is free)
        *left = (uint32_t)next.size();
        src = &next;
        return false;
    };
    const auto brute = [&](uint32_t) {
        for (const Rec& self : *src) {
            float row[K];
            brute_entry<K>(gr.records, self, k, row);
            store(self, row);
        }
        return false;
    };
    radius_search<bool>(s, P, grid, round, brute);
    out.first_radius = s.first_radius;
    out.rounds = s.rounds;
    out.n_brute = s.n_brute;
}

// the definition: every pair, self excluded by index, the k smallest with multiplicity
static void definition(const std::vector<float>& pos, uint32_t k, uint32_t score, Result& out) {
    const size_t n = pos.size() / 3;
    out.rows.assign(n * k, INFINITY);
    out.scores.assign(n, INFINITY);
    std::vector<uint8_t> part(n);
    for (size_t i = 0; i < n; ++i) part[i] = nb_finite(pos[3 * i]) && nb_finite(pos[3 * i + 1]) && nb_finite(pos[3 * i + 2]);
    std::vector<float> d;
    for (size_t i = 0; i < n; ++i) {
        if (!part[i]) continue;
        d.clear();
        for (size_t j = 0; j < n; ++j)
            if (j != i && part[j]) d.push_back(nb_d2(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]));
        std::sort(d.begin(), d.end());
        float b[16];
        knn_clear(b, k);
        for (uint32_t q = 0; q < k && q < d.size(); ++q) b[16u - k + q] = d[q];
        out.scores[i] = knn_score(b, k, score);
        knn_store(b, k, &out.rows[i * k]);
    }
}

template <int K>
static void chain(const std::vector<uint32_t>& w) {
    const uint32_t k = w[1];
    float b[K];
    knn_clear(b, k);
    for (size_t j = 2; j < w.size(); ++j) knn_insert(b, nb_from_bits(w[j]));
    float out[K];
    knn_store(b, k, out);
    printf("chain");
    for (uint32_t q = 0; q < k; ++q) printf(" %x", bits_of(out[q]));
    printf("\n");
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
        if (cmd == "search" && w.size() >= 5 && w[0] >= 1u && w[0] <= kKnnMaxK) {
            std::vector<float> pos;
            for (size_t j = 5; j < w.size(); ++j) pos.push_back(nb_from_bits(w[j]));
            pos.resize(pos.size() / 3 * 3);
            Result got, want;
            const float hint = nb_from_bits(w[2]);
            switch (knn_round_k(w[0])) {
                case 4u: search<4>(pos, w[0], w[1], hint, w[3], w[4], got); break;
                case 8u: search<8>(pos, w[0], w[1], hint, w[3], w[4], got); break;
                default: search<16>(pos, w[0], w[1], hint, w[3], w[4], got); break;
            }
            definition(pos, w[0], w[1], want);
            size_t bad_rows = 0, bad_scores = 0;
            for (size_t j = 0; j < got.rows.size(); ++j) bad_rows += bits_of(got.rows[j]) != bits_of(want.rows[j]);
            for (size_t j = 0; j < got.scores.size(); ++j) bad_scores += bits_of(got.scores[j]) != bits_of(want.scores[j]);
            printf("search %u %u %u %x %zu %zu\nrows", got.participants, got.rounds, got.n_brute, bits_of(got.first_radius), bad_rows, bad_scores);
            for (float v : got.rows) printf(" %x", bits_of(v));
            printf("\nscores");
            for (float v : got.scores) printf(" %x", bits_of(v));
            printf("\n");
        } else if (cmd == "chain" && w.size() >= 2 && w[1] >= 1u && w[1] <= w[0]) {
            if (w[0] == 4u) chain<4>(w);
            if (w[0] == 8u) chain<8>(w);
            if (w[0] == 16u) chain<16>(w);
        } else if (cmd == "floor" && w.size() == 3) {
            const double ext[3] = {(double)nb_from_bits(w[0]), (double)nb_from_bits(w[1]), (double)nb_from_bits(w[2])};
            printf("floor %x\n", bits_of(knn_radius_floor(ext)));
        } else if (cmd == "first" && w.size() == 5) {
            const double ext[3] = {(double)nb_from_bits(w[0]), (double)nb_from_bits(w[1]), (double)nb_from_bits(w[2])};
            printf("first %x\n", bits_of(knn_first_radius(ext, w[3], w[4])));
        } else if (cmd == "brute" && w.size() == 6) {
            printf("brute %d\n", (int)knn_go_brute(w[0], w[1], w[2], w[3], nb_from_bits(w[4]), w[5] != 0u));
        } else if (cmd == "coarse" && w.size() == 4) {
            const double ext[3] = {(double)nb_from_bits(w[1]), (double)nb_from_bits(w[2]), (double)nb_from_bits(w[3])};
            printf("coarse %d\n", (int)knn_coarse(nb_from_bits(w[0]), ext));
        } else if (cmd == "threshold" && w.size() == 5) {
            printf("threshold %x\n", bits_of(knn_threshold(double_of(w[0], w[1]), double_of(w[2], w[3]), nb_from_bits(w[4]))));
        } else {
            printf("? %s\n", cmd.c_str());
        }
        line.clear();
    }
    return 0;
}
