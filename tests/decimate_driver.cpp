// tests/decimate_driver.cpp — csrc/decimate_math.h played on the host, for tests/test_decimate_cpu.py and tests/test_gpu_decimate.py: a
// stand-alone program, built with -fsanitize=address,undefined and -ffp-contract=off and run as a child process.  It restates spec §22
// in float32 with the header's functions and the one cell function of neighbors_math.h: participants, origin, cells, representatives,
// the order of dst, out_map, the statistics, the rows of dst, and gsx_model_decimate_edge's bisection.
// One binary request on stdin, one binary answer on stdout (little-endian, as the arrays lie in memory):
//   request   u32 command (1 decimate, 2 edge, 3 desc)  u32 n  f32 cell  u32 0  u64 target
//             u8 kept[n] (passes the filter)  f32 pos[n][3]  u32 color[n]  f32 cov[n][6]  f32 sh[n][45]   (exactly dequantised planes)
//   decimate  u64 count  u64 n_nonfinite  u64 cells  u64 singletons  u32 largest_cell  u32 0
//             u32 map[n]  f32 pos[cells][3]  u32 color[cells]  f32 cov[cells][6]  f32 sh[cells][45]  f32 alpha[cells]  u32 members[cells]
//             (alpha: the opacity before its byte, for the float64 comparison; a one-member cell's is its byte / 255)
//   edge      f32 cell  u32 0  u64 cells
//   desc      u32 sizeof desc, sizeof stats, then the offsets of cell, grid_bits, reserved; cells, singletons, largest_cell, grid_bits
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <vector>

#include "decimate_math.h"
#include "gsx.h"

static_assert(sizeof(gsx_decimate_desc) == 24 && sizeof(gsx_decimate_stats_t) == 40, "spec section 22's layouts");

namespace {

struct Scene {
    uint32_t n = 0;
    std::vector<uint8_t> kept;
    std::vector<float> pos, cov, sh;
    std::vector<uint32_t> color;
};
struct Result {
    uint64_t count = 0, n_nonfinite = 0, cells = 0, singletons = 0;
    uint32_t largest = 0;
    std::vector<uint32_t> map, color, members;
    std::vector<float> pos, cov, sh, alpha;
};

template <class T>
bool read_all(std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, stdin) == count;
}
template <class T>
void write_all(const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), stdout);
}

bool participants(const Scene& s, std::vector<uint32_t>& idx, uint64_t* nonfinite, float origin[3]) {
    origin[0] = origin[1] = origin[2] = INFINITY;
    *nonfinite = 0;
    for (uint32_t i = 0; i < s.n; ++i) {
        if (!s.kept[i]) continue;
        const float* p = &s.pos[3 * (size_t)i];
        if (gsx::nb_finite(p[0]) && gsx::nb_finite(p[1]) && gsx::nb_finite(p[2])) {
            idx.push_back(i);
            for (int a = 0; a < 3; ++a) origin[a] = fminf(origin[a], p[a]);
        } else {
            *nonfinite += 1;
        }
    }
    return !idx.empty();
}

// the cells in ascending order of representative, each with its members in ascending index (count only: no rows)
void decimate(const Scene& s, float cell, bool rows, Result* out) {
    std::vector<uint32_t> idx;
    float origin[3];
    out->map.assign(s.n, gsx::kDecNoCell);
    participants(s, idx, &out->n_nonfinite, origin);
    out->count = idx.size();
    const float inv_h = gsx::dec_grid(cell).inv_h;
    std::map<uint64_t, uint32_t> cell_of;        // cell key -> dst index
    std::vector<std::vector<uint32_t>> members;  // by dst index: first seen in index order = ascending representative
    for (const uint32_t i : idx) {
        const float* p = &s.pos[3 * (size_t)i];
        const uint64_t key = gsx::dec_cell_key(gsx::nb_cell(p[0], origin[0], inv_h), gsx::nb_cell(p[1], origin[1], inv_h), gsx::nb_cell(p[2], origin[2], inv_h));
        const auto at = cell_of.emplace(key, (uint32_t)members.size());
        if (at.second) members.emplace_back();
        members[at.first->second].push_back(i);
        out->map[i] = at.first->second;
    }
    out->cells = members.size();
    for (const auto& m : members) {
        out->singletons += m.size() == 1 ? 1 : 0;
        out->largest = m.size() > out->largest ? (uint32_t)m.size() : out->largest;
    }
    if (!rows) return;
    for (const auto& m : members) {
        const uint32_t r = m[0];
        out->members.push_back((uint32_t)m.size());
        if (m.size() == 1) {  // copied as it is stored
            for (int a = 0; a < 3; ++a) out->pos.push_back(s.pos[3 * (size_t)r + a]);
            for (int a = 0; a < 6; ++a) out->cov.push_back(s.cov[6 * (size_t)r + a]);
            for (int a = 0; a < 45; ++a) out->sh.push_back(s.sh[45 * (size_t)r + a]);
            out->color.push_back(s.color[r]);
            out->alpha.push_back((float)(s.color[r] >> 24) / 255.0f);
            continue;
        }
        const float* pr = &s.pos[3 * (size_t)r];
        float acc_m[gsx::kDecColumns] = {}, acc_u[gsx::kDecColumns] = {};
        uint32_t max_a = 0;
        for (const uint32_t i : m) {  // strictly left to right in member order
            float v[gsx::kDecGeo];
            uint32_t a;
            const float mass = gsx::dec_member(&s.pos[3 * (size_t)i], pr, &s.cov[6 * (size_t)i], s.color[i], v, &a);
            max_a = a > max_a ? a : max_a;
            for (uint32_t c = 0; c < gsx::kDecColumns; ++c) {
                const float value = c < gsx::kDecGeo ? v[c] : s.sh[45 * (size_t)i + (c - gsx::kDecGeo)];
                acc_m[c] = gsx::dec_acc(acc_m[c], mass, value);
                acc_u[c] = gsx::dec_acc(acc_u[c], 1.0f, value);
            }
        }
        const float M = acc_m[0];
        const bool mass = gsx::dec_mass(M);
        const float* acc = mass ? acc_m : acc_u;
        float mu[3], cov[6], inv, alpha;
        uint32_t color;
        gsx::dec_finish(acc, mass, M, max_a, pr, mu, cov, &color, &inv, &alpha);
        for (int a = 0; a < 3; ++a) out->pos.push_back(mu[a]);
        for (int a = 0; a < 6; ++a) out->cov.push_back(cov[a]);
        for (uint32_t f = 0; f < 45u; ++f) out->sh.push_back(gsx::dec_sh(acc[gsx::kDecGeo + f], inv));
        out->color.push_back(color);
        out->alpha.push_back(alpha);
    }
}

template <class T>
void put(T v) {
    fwrite(&v, sizeof v, 1, stdout);
}

}  // namespace

int main() {
    struct {
        uint32_t command, n;
        float cell;
        uint32_t zero;
        uint64_t target;
    } head;
    static_assert(sizeof head == 24, "the request's head");
    if (fread(&head, sizeof head, 1, stdin) != 1) return 2;
    if (head.command == 3u) {
        put((uint32_t)sizeof(gsx_decimate_desc));
        put((uint32_t)sizeof(gsx_decimate_stats_t));
        put((uint32_t)offsetof(gsx_decimate_desc, cell));
        put((uint32_t)offsetof(gsx_decimate_desc, grid_bits));
        put((uint32_t)offsetof(gsx_decimate_desc, reserved));
        put((uint32_t)offsetof(gsx_decimate_stats_t, cells));
        put((uint32_t)offsetof(gsx_decimate_stats_t, singletons));
        put((uint32_t)offsetof(gsx_decimate_stats_t, largest_cell));
        put((uint32_t)offsetof(gsx_decimate_stats_t, grid_bits));
        return 0;
    }
    Scene s;
    s.n = head.n;
    const size_t n = s.n;
    if (!read_all(s.kept, n) || !read_all(s.pos, 3 * n) || !read_all(s.color, n) || !read_all(s.cov, 6 * n) || !read_all(s.sh, 45 * n)) return 2;
    if (head.command == 1u) {
        if (!gsx::dec_cell_ok(head.cell)) return 3;
        Result r;
        decimate(s, head.cell, true, &r);
        put(r.count);
        put(r.n_nonfinite);
        put(r.cells);
        put(r.singletons);
        put(r.largest);
        put((uint32_t)0);
        write_all(r.map);
        write_all(r.pos);
        write_all(r.color);
        write_all(r.cov);
        write_all(r.sh);
        write_all(r.alpha);
        write_all(r.members);
    } else if (head.command == 2u) {
        std::vector<uint32_t> idx;
        uint64_t nonfinite;
        float origin[3], cell = 0.0f;
        uint64_t cells = 0;
        if (participants(s, idx, &nonfinite, origin)) {
            float extent = 0.0f;
            for (int a = 0; a < 3; ++a) {
                float mx = -INFINITY;
                for (const uint32_t i : idx) mx = fmaxf(mx, s.pos[3 * (size_t)i + a]);
                extent = fmaxf(extent, mx - origin[a]);
            }
            const auto count = [&](float edge, uint64_t* out) {
                Result r;
                decimate(s, edge, false, &r);
                *out = r.cells;
                return 0;
            };
            gsx::dec_find_edge(extent, head.target, count, &cell, &cells);
        }
        put(cell);
        put((uint32_t)0);
        put(cells);
    } else {
        fprintf(stderr, "unknown command %u\n", head.command);
        return 2;
    }
    return fflush(stdout) == 0 ? 0 : 2;
}
