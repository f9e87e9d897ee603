// toolset_driver.cpp — plays scripts against csrc/toolset_state.h on the CPU and paints what it queues into a byte array with the
// rule of csrc/toolset_math.h, tile by tile as k_toolset_paint does (tests/test_toolset_cpu.py; built with the address and
// undefined-behaviour sanitizers).  Commands on stdin, one per line:
//   size W H | use_texture 0|1 | radius R | start TOOL OP X Y | pos X Y | end | query | state | render | dump
// Output: `query kind op p0x p0y p1x p1y radius`, `state active tool op sx sy px py`, `flush ...` for a queue that filled up and
// `render ...` for a render command (n_segs has_rect has_erase clear x0 y0 x1 y1 of the covered box), `tex` + H rows of W digits.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "toolset_state.h"

using namespace gsx;

static uint32_t W = 1, H = 1, tex_w = 0, tex_h = 0;
static std::vector<uint8_t> tex;
static ToolsetState ts;

static void flush(const char* what) {
    const bool resized = tex_w != W || tex_h != H;
    if (resized) tex.assign((size_t)W * H, 0x5a);  // (a fresh allocation holds anything: the clear must be exact)
    ToolsetPaint p;
    ToolsetBox cover;
    if (!ts.take(W, H, resized, &p, &cover)) {
        printf("%s idle\n", what);
        return;
    }
    tex_w = W;
    tex_h = H;
    if (p.clear) memset(tex.data(), 0, tex.size());
    printf("%s %u %u %u %u %d %d %d %d\n", what, p.n_segs, p.has_rect, p.has_erase, p.clear, cover.x0, cover.y0, cover.x1, cover.y1);
    if (toolset_box_empty(cover)) return;
    const int32_t T = (int32_t)GSX_TILE;
    for (int32_t ty = cover.y0 / T; ty < (cover.y1 + T - 1) / T; ++ty)
        for (int32_t tx = cover.x0 / T; tx < (cover.x1 + T - 1) / T; ++tx) {
            const int32_t x0 = tx * T, y0 = ty * T, x1 = std::min(x0 + T, (int32_t)W), y1 = std::min(y0 + T, (int32_t)H);
            uint64_t mask = 0;
            for (uint32_t j = 0; j < p.n_segs; ++j) {
                const ToolsetBox b = toolset_seg_box(p.seg[j], W, H);
                if (b.x0 < x1 && b.x1 > x0 && b.y0 < y1 && b.y1 > y0) mask |= 1ull << j;
            }
            for (int32_t y = y0; y < y1; ++y)
                for (int32_t x = x0; x < x1; ++x) {
                    const int v = toolset_texel(p, x, y, mask);
                    if (v >= 0) tex.at((size_t)y * W + x) = (uint8_t)v;
                }
        }
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char cmd[32] = "";
        float a = 0, b = 0;
        unsigned u0 = 0, u1 = 0;
        if (sscanf(line, "%31s", cmd) != 1) continue;
        const char* rest = line + strlen(cmd);
        if (!strcmp(cmd, "size") && sscanf(rest, "%u %u", &u0, &u1) == 2) {
            W = u0;
            H = u1;
        } else if (!strcmp(cmd, "use_texture") && sscanf(rest, "%u", &u0) == 1) {
            ts.set_use_texture(u0 != 0);
        } else if (!strcmp(cmd, "radius") && sscanf(rest, "%f", &a) == 1) {
            ts.update_brush_radius(a);
        } else if (!strcmp(cmd, "start") && sscanf(rest, "%u %u %f %f", &u0, &u1, &a, &b) == 4) {
            const float p[2] = {a, b};
            ts.start(u0, u1, p);
        } else if (!strcmp(cmd, "pos") && sscanf(rest, "%f %f", &a, &b) == 2) {
            const float p[2] = {a, b};
            ts.update_pos(p);
            if (ts.full()) flush("flush");
        } else if (!strcmp(cmd, "end")) {
            ts.end();
        } else if (!strcmp(cmd, "query")) {
            const gsx_query q = ts.query();
            printf("query %u %u %.9g %.9g %.9g %.9g %.9g\n", q.kind, q.selection_op, q.p0[0], q.p0[1], q.p1[0], q.p1[1], q.radius);
        } else if (!strcmp(cmd, "state")) {
            if (ts.active())
                printf("state 1 %u %u %.9g %.9g %.9g %.9g\n", ts.tool, ts.op, ts.start_pos[0], ts.start_pos[1], ts.pos[0], ts.pos[1]);
            else
                printf("state 0\n");
        } else if (!strcmp(cmd, "render")) {
            flush("render");
        } else if (!strcmp(cmd, "dump")) {
            printf("tex %u %u\n", tex_w, tex_h);
            for (uint32_t y = 0; y < tex_h; ++y) {
                std::string row(tex_w, '?');
                for (uint32_t x = 0; x < tex_w; ++x) {
                    const uint8_t v = tex[(size_t)y * tex_w + x];
                    row[x] = v == 255 ? '1' : (v == 0 ? '0' : '?');
                }
                puts(row.c_str());
            }
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
    }
    return 0;
}
