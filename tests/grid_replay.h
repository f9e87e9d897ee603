// grid_replay.h — what the host drivers of the grid operations share (neighbors_driver.cpp, knn_driver.cpp, nearest_driver.cpp): the hex
// words of a command line, a float's bits, and section 18's hashed grid built on the host by a counting sort, as the device's four
// passes leave it: the participants' minimum as the origin, the table of bucket ends, the records in bucket order.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "neighbors_math.h"

inline std::vector<uint32_t> words(const char* s) {
    std::vector<uint32_t> v;
    char* end = nullptr;
    for (;;) {
        while (*s == ' ') ++s;
        const unsigned long x = strtoul(s, &end, 16);
        if (end == s) break;
        v.push_back((uint32_t)x);
        s = end;
    }
    return v;
}
inline uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

struct Rec {
    float x, y, z;
    uint32_t index;
};
struct Grid {
    gsx::NbGrid g;
    float origin[3];
    uint32_t bits;
    std::vector<uint32_t> ends;  // the table after the scatter: bucket b holds records [ends[b - 1], ends[b])
    std::vector<Rec> records;
};

inline Grid build_grid(const std::vector<Rec>& part, float radius, uint32_t bits) {
    using namespace gsx;
    Grid gr;
    gr.g = nb_grid(radius);
    gr.bits = bits;
    for (int a = 0; a < 3; ++a) gr.origin[a] = INFINITY;
    for (const Rec& r : part) {
        gr.origin[0] = fminf(gr.origin[0], r.x);
        gr.origin[1] = fminf(gr.origin[1], r.y);
        gr.origin[2] = fminf(gr.origin[2], r.z);
    }
    const auto bucket = [&](const Rec& r) {
        return nb_bucket(nb_cell(r.x, gr.origin[0], gr.g.inv_h), nb_cell(r.y, gr.origin[1], gr.g.inv_h), nb_cell(r.z, gr.origin[2], gr.g.inv_h), bits);
    };
    std::vector<uint32_t> table(size_t(1) << bits, 0u);
    for (const Rec& r : part) table[bucket(r)] += 1u;
    uint32_t at = 0;
    for (uint32_t& w : table) {  // sizes -> starts
        const uint32_t size = w;
        w = at;
        at += size;
    }
    gr.records.resize(part.size());
    for (const Rec& r : part) gr.records[table[bucket(r)]++] = r;  // starts -> ends
    gr.ends = table;
    return gr;
}
