// normals_driver.cpp — csrc/normals_math.h and csrc/neighbors_math.h played on the host through a plain C++ version of the whole search
// of the model normals (spec §26), for tests/test_normals_cpu.py and tests/test_gpu_normals.py: a stand-alone program the tests build
// with the address and undefined-behaviour sanitizers and -ffp-contract=off.  The loop over the rounds is the library's own, not a
// restatement: csrc/radius_search.h, which gsx_api_normals.cpp runs; this file supplies the work (but for one input: it hands the loop
// the whole box where the device hands it the 10 permille trimmed box of the bounds passes): section 18's hashed grid by a counting
// sort (grid_replay.h), a round of one query an entry over 27 cells with the own-cell test, the keyed chain and the proven rule, the
// unresolved list, the fallback as 256 strided per-lane lists merged by key, and the plane fit of a resolved entry, gathered by index in
// list order.  Every float crosses as the hex of its bits.  stdin, one command a line (hex words):
//   "search <k> <orient> <tx> <ty> <tz> <hint> <grid_bits> <max_rounds> <x y z> ..."
//        stdout "search <participants> <rounds> <n_brute> <first radius> <lists that differ from the O(n^2) loop> <fits that differ>"
//               "index <n * k words>"  "normal <n * 3 values>"  "variation <n values>"
//               "stats <n_fitted> <variation_min> <variation_max> <mean lo> <mean hi>"   (the mean: the sum in index order)
//   "replay ..."   the same without the O(n^2) loop (the two counts are 0): for the sizes at which the loop would take seconds
//   "chain <K> <k> <hi lo> ..."    stdout "chain <k keys as hi lo>": the chain's k smallest of the keys, K in {4, 8, 16}
//   "hit <mode> <flags> <lo> <hi> <dx dy dz> <nx ny nz variation> ..."   stdout "hit <0|1> ..." then "dir <x y z>": nm_direction, nm_select_hit
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
#include "normals_math.h"
#include "radius_search.h"

using namespace gsx;

// k_normals_query's lane: true where the list is proven (b holds it)
template <int K>
static bool query_entry(const Grid& gr, const Rec& self, uint32_t k, uint64_t (&b)[K]) {
    const float r2 = gr.g.r2, inv_h = gr.g.inv_h;
    const uint32_t cx = nb_cell(self.x, gr.origin[0], inv_h), cy = nb_cell(self.y, gr.origin[1], inv_h), cz = nb_cell(self.z, gr.origin[2], inv_h);
    nm_reset(b, k);
    for (uint32_t c = 0; c < 27u; ++c) {
        const uint32_t vx = cx + (c % 3u) - 1u, vy = cy + ((c / 3u) % 3u) - 1u, vz = cz + (c / 9u) - 1u;
        if (vx > kNbMaxCell || vy > kNbMaxCell || vz > kNbMaxCell) continue;
        const uint32_t bucket = nb_bucket(vx, vy, vz, gr.bits);
        uint32_t q = bucket ? gr.ends[bucket - 1u] : 0u;
        const uint32_t end = gr.ends[bucket];
        for (; q < end; ++q) {
            const Rec& r = gr.records[q];
            const float d2 = nb_d2(self.x, self.y, self.z, r.x, r.y, r.z);
            if (d2 <= r2 && r.index != self.index) {
                const uint64_t key = nm_key(d2, r.index);
                if (key < nm_last(b) && nb_cell(r.x, gr.origin[0], inv_h) == vx && nb_cell(r.y, gr.origin[1], inv_h) == vy &&
                    nb_cell(r.z, gr.origin[2], inv_h) == vz)
                    nm_offer(b, key);
            }
        }
    }
    return nm_list_proven(nm_last(b), r2);
}

// k_normals_brute's workgroup
template <int K>
static void brute_entry(const std::vector<Rec>& records, const Rec& self, uint32_t k, uint64_t (&row)[K]) {
    std::vector<uint64_t> best((size_t)K * kNormalsBruteLanes);
    for (uint32_t t = 0; t < kNormalsBruteLanes; ++t) {
        uint64_t b[K];
        nm_reset(b, k);
        for (size_t q = t; q < records.size(); q += kNormalsBruteLanes) {
            const Rec& r = records[q];
            if (r.index == self.index) continue;
            const uint64_t key = nm_key(nb_d2(self.x, self.y, self.z, r.x, r.y, r.z), r.index);
            if (key < nm_last(b)) nm_offer(b, key);
        }
        for (int q = 0; q < K; ++q) best[(size_t)q * kNormalsBruteLanes + t] = b[q];
    }
    std::vector<uint32_t> head(kNormalsBruteLanes, (uint32_t)K - k);
    nm_reset(row, k);
    for (uint32_t q = (uint32_t)K - k; q < (uint32_t)K; ++q) {
        uint64_t win = kNormalsEmpty;
        uint32_t owner = kNormalsBruteLanes;
        for (uint32_t t = 0; t < kNormalsBruteLanes; ++t) {
            const uint64_t mine = head[t] < (uint32_t)K ? best[(size_t)head[t] * kNormalsBruteLanes + t] : kNormalsEmpty;
            if (mine < win) {
                win = mine;
                owner = t;
            }
        }
        row[q] = win;
        if (owner < kNormalsBruteLanes) head[owner] += 1u;
    }
}

struct Result {
    uint32_t participants = 0, rounds = 0, n_brute = 0;
    float first_radius = 0.0f;
    std::vector<uint32_t> index;
    std::vector<float> normal, variation;
};

struct Orient {
    uint32_t rule;
    float toward[3];
};

// what normals_store_entry does with a resolved list
template <int K>
static void store_entry(const std::vector<float>& pos, const Rec& self, uint32_t k, const uint64_t (&b)[K], const Orient& o, Result& out) {
    const size_t n = pos.size() / 3;
    const float p[3] = {self.x, self.y, self.z};
    const NormalFit f = nm_plane_fit(b, k, p, [&](uint32_t j, float (&at)[3]) {
        if (j >= n) abort();  // (a fitted list holds indices of Gaussians)
        for (int a = 0; a < 3; ++a) at[a] = pos[3 * (size_t)j + a];
    }, o.rule, o.toward);
    for (int a = 0; a < 3; ++a) out.normal[3 * (size_t)self.index + a] = f.n[a];
    out.variation[self.index] = f.variation;
    nm_store_indices(b, k, &out.index[(size_t)self.index * k]);
}

static std::vector<Rec> participants(const std::vector<float>& pos) {
    std::vector<Rec> part;
    for (size_t i = 0; i < pos.size() / 3; ++i) {
        const Rec r{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], (uint32_t)i};
        if (nb_finite(r.x) && nb_finite(r.y) && nb_finite(r.z)) part.push_back(r);
    }
    return part;
}

static void clear(Result& out, size_t n, uint32_t k) {
    out.index.assign(n * k, kNormalsNone);
    out.normal.assign(n * 3, 0.0f);
    out.variation.assign(n, INFINITY);
}

template <int K>
static void search(const std::vector<float>& pos, uint32_t k, const Orient& o, float hint, uint32_t grid_bits, uint32_t max_rounds, Result& out) {
    const size_t n = pos.size() / 3;
    clear(out, n, k);
    const std::vector<Rec> part = participants(pos);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const Rec& r : part) {
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
    const auto grid = [&](float r, bool final_round) {
        if (!nb_radius_ok(r) || final_round) abort();
        gr = build_grid(part, r, bits);
        return false;
    };
    const auto round = [&](uint32_t i, uint32_t, bool, uint32_t* left) {
        std::vector<Rec>& next = list[i & 1u];
        next.clear();
        for (const Rec& self : *src) {
            uint64_t b[K];
            if (query_entry<K>(gr, self, k, b))
                store_entry<K>(pos, self, k, b, o, out);
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
            uint64_t row[K];
            brute_entry<K>(gr.records, self, k, row);
            store_entry<K>(pos, self, k, row, o, out);
        }
        return false;
    };
    radius_search<bool>(s, P, grid, round, brute);
    out.first_radius = s.first_radius;
    out.rounds = s.rounds;
    out.n_brute = s.n_brute;
}

// the definition: every pair, self excluded by index, the k smallest keys in sorted order, fitted in that order
static void definition(const std::vector<float>& pos, uint32_t k, const Orient& o, Result& out) {
    const size_t n = pos.size() / 3;
    clear(out, n, k);
    const std::vector<Rec> part = participants(pos);
    std::vector<uint64_t> keys;
    for (const Rec& self : part) {
        keys.clear();
        for (const Rec& r : part)
            if (r.index != self.index) keys.push_back(nm_key(nb_d2(self.x, self.y, self.z, r.x, r.y, r.z), r.index));
        std::sort(keys.begin(), keys.end());
        uint64_t b[16];
        nm_reset(b, k);
        for (uint32_t q = 0; q < k && q < keys.size(); ++q) b[16u - k + q] = keys[q];
        store_entry<16>(pos, self, k, b, o, out);
    }
}

template <int K>
static void chain(const std::vector<uint32_t>& w) {
    const uint32_t k = w[1];
    uint64_t b[K];
    nm_reset(b, k);
    for (size_t j = 2; j + 1 < w.size(); j += 2) {
        const uint64_t key = ((uint64_t)w[j] << 32) | w[j + 1];
        if (key < nm_last(b)) nm_offer(b, key);
    }
    printf("chain");
    for (int q = 0; q < K; ++q)
        if ((uint32_t)q + k >= (uint32_t)K) printf(" %x %x", (uint32_t)(b[q] >> 32), (uint32_t)b[q]);
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
        if ((cmd == "search" || cmd == "replay") && w.size() >= 8 && w[0] >= kNormalsMinK && w[0] <= kNormalsMaxK) {
            std::vector<float> pos;
            for (size_t j = 8; j < w.size(); ++j) pos.push_back(nb_from_bits(w[j]));
            pos.resize(pos.size() / 3 * 3);
            const Orient o{w[1], {nb_from_bits(w[2]), nb_from_bits(w[3]), nb_from_bits(w[4])}};
            Result got, want;
            const float hint = nb_from_bits(w[5]);
            switch (knn_round_k(w[0])) {
                case 4u: search<4>(pos, w[0], o, hint, w[6], w[7], got); break;
                case 8u: search<8>(pos, w[0], o, hint, w[6], w[7], got); break;
                default: search<16>(pos, w[0], o, hint, w[6], w[7], got); break;
            }
            size_t bad_lists = 0, bad_fits = 0;
            if (cmd == "search") {
                definition(pos, w[0], o, want);
                for (size_t j = 0; j < got.index.size(); ++j) bad_lists += got.index[j] != want.index[j];
                for (size_t j = 0; j < got.normal.size(); ++j) bad_fits += bits_of(got.normal[j]) != bits_of(want.normal[j]);
                for (size_t j = 0; j < got.variation.size(); ++j) bad_fits += bits_of(got.variation[j]) != bits_of(want.variation[j]);
            }
            printf("search %u %u %u %x %zu %zu\nindex", got.participants, got.rounds, got.n_brute, bits_of(got.first_radius), bad_lists, bad_fits);
            for (uint32_t v : got.index) printf(" %x", v);
            printf("\nnormal");
            for (float v : got.normal) printf(" %x", bits_of(v));
            printf("\nvariation");
            for (float v : got.variation) printf(" %x", bits_of(v));
            uint32_t fitted = 0;
            float mn = INFINITY, mx = -INFINITY;
            double sum = 0.0;
            for (float v : got.variation)
                if (nm_is_fitted(v)) {
                    fitted += 1u;
                    mn = fminf(mn, v);
                    mx = fmaxf(mx, v);
                    sum += (double)v;
                }
            const double mean = fitted ? sum / (double)fitted : 0.0;
            uint64_t mean_bits;
            memcpy(&mean_bits, &mean, 8);
            printf("\nstats %x %x %x %x %x\n", fitted, fitted ? bits_of(mn) : 0u, fitted ? bits_of(mx) : 0u, (uint32_t)mean_bits, (uint32_t)(mean_bits >> 32));
        } else if (cmd == "chain" && w.size() >= 2 && w[1] >= 1u && w[1] <= w[0]) {
            if (w[0] == 4u) chain<4>(w);
            if (w[0] == 8u) chain<8>(w);
            if (w[0] == 16u) chain<16>(w);
        } else if (cmd == "hit" && w.size() >= 7 && (w.size() - 7) % 4 == 0) {
            const float raw[3] = {nb_from_bits(w[4]), nb_from_bits(w[5]), nb_from_bits(w[6])};
            float dir[3] = {0.0f, 0.0f, 0.0f};
            const bool ok = nm_direction(raw, dir);
            printf("hit");
            for (size_t j = 7; j < w.size(); j += 4) {
                const float nv[3] = {nb_from_bits(w[j]), nb_from_bits(w[j + 1]), nb_from_bits(w[j + 2])};
                printf(" %d", (int)nm_select_hit(w[0], w[1], nv, nb_from_bits(w[j + 3]), dir, nb_from_bits(w[2]), nb_from_bits(w[3])));
            }
            printf("\ndir %d %x %x %x\n", (int)ok, bits_of(dir[0]), bits_of(dir[1]), bits_of(dir[2]));
        } else {
            printf("? %s\n", cmd.c_str());
        }
        line.clear();
    }
    return 0;
}
