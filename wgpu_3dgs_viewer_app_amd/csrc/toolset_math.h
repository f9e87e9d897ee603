// toolset_math.h — the query toolset's painting rule (spec/RENDER_SPEC.md §7, "Toolset"), written once: k_toolset_paint
// (kernels_toolset.hip) and the host restatement of tests/toolset_driver.cpp both include it, so the two cannot drift.
// Plain float32 arithmetic, <math.h> only; no HIP include (the functions are __host__ __device__ under hipcc).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GSX_TS_HD __host__ __device__
#else
#define GSX_TS_HD
#endif

namespace gsx {

constexpr uint32_t kToolsetMaxSegs = 64;  // pending brush segments one launch takes (one per lane of a wave)

struct ToolsetSeg {
    float ax, ay, bx, by, r;  // capsule a -> b of radius r (a == b: a disc)
};
struct ToolsetBox {
    int32_t x0, y0, x1, y1;  // texels, max exclusive; clamped to the texture
};

// Brush: is the texel centre (px, py) within r of the segment a -> b?
GSX_TS_HD inline bool toolset_in_capsule(float px, float py, const ToolsetSeg& s) {
    const float dx = s.bx - s.ax, dy = s.by - s.ay;
    const float len2 = dx * dx + dy * dy;
    float t = 0.0f;  // the zero-length segment is its own case: a disc at a
    if (len2 > 0.0f) t = fminf(fmaxf(((px - s.ax) * dx + (py - s.ay) * dy) / len2, 0.0f), 1.0f);
    const float ex = px - (s.ax + t * dx), ey = py - (s.ay + t * dy);
    return ex * ex + ey * ey <= s.r * s.r;
}

// Rect: is the texel centre inside the rectangle (corners sorted: x0 <= x1, y0 <= y1)?
GSX_TS_HD inline bool toolset_in_rect(float px, float py, float x0, float y0, float x1, float y1) {
    return x0 <= px && px <= x1 && y0 <= py && py <= y1;
}

GSX_TS_HD inline int32_t toolset_clamp_texel(float v, uint32_t n) { return (int32_t)fminf(fmaxf(v, 0.0f), (float)n); }

// A conservative texel box of the centres x + 0.5 in [lo_x, hi_x] x [lo_y, hi_y] (one texel of slack either side: the exact test decides),
// clamped as floats first — a position may lie far outside the texture.
GSX_TS_HD inline ToolsetBox toolset_box(float lo_x, float lo_y, float hi_x, float hi_y, uint32_t w, uint32_t h) {
    ToolsetBox b;
    b.x0 = toolset_clamp_texel(floorf(lo_x - 0.5f) - 1.0f, w);
    b.y0 = toolset_clamp_texel(floorf(lo_y - 0.5f) - 1.0f, h);
    b.x1 = toolset_clamp_texel(floorf(hi_x - 0.5f) + 3.0f, w);
    b.y1 = toolset_clamp_texel(floorf(hi_y - 0.5f) + 3.0f, h);
    return b;
}
GSX_TS_HD inline ToolsetBox toolset_seg_box(const ToolsetSeg& s, uint32_t w, uint32_t h) {
    return toolset_box(fminf(s.ax, s.bx) - s.r, fminf(s.ay, s.by) - s.r, fmaxf(s.ax, s.bx) + s.r, fmaxf(s.ay, s.by) + s.r, w, h);
}
GSX_TS_HD inline bool toolset_box_empty(const ToolsetBox& b) { return b.x0 >= b.x1 || b.y0 >= b.y1; }
GSX_TS_HD inline ToolsetBox toolset_box_union(const ToolsetBox& a, const ToolsetBox& b) {
    if (toolset_box_empty(a)) return b;
    if (toolset_box_empty(b)) return a;
    ToolsetBox u;
    u.x0 = a.x0 < b.x0 ? a.x0 : b.x0;
    u.y0 = a.y0 < b.y0 ? a.y0 : b.y0;
    u.x1 = a.x1 > b.x1 ? a.x1 : b.x1;
    u.y1 = a.y1 > b.y1 ? a.y1 : b.y1;
    return u;
}

// One paint launch: every pending shape, by value.  erase: texels of this box that no shape sets are written 0 (a Rect repaint: what
// has been painted since the last clear); the rectangle (has_rect) has its corners sorted.
struct ToolsetPaint {
    uint32_t n_segs, has_rect, has_erase, clear;  // clear: the whole texture is zeroed in front of the launch (host side: a memset)
    float rx0, ry0, rx1, ry1;
    ToolsetBox erase;
    ToolsetSeg seg[kToolsetMaxSegs];
};

// value of texel (x, y) under one paint: 255 set, 0 erased, -1 left as it is
GSX_TS_HD inline int toolset_texel(const ToolsetPaint& p, int32_t x, int32_t y, uint64_t seg_mask) {
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    bool set = p.has_rect && toolset_in_rect(px, py, p.rx0, p.ry0, p.rx1, p.ry1);
    for (uint32_t j = 0; !set && j < p.n_segs; ++j)
        if ((seg_mask >> j) & 1ull) set = toolset_in_capsule(px, py, p.seg[j]);
    if (set) return 255;
    if (p.has_erase && x >= p.erase.x0 && x < p.erase.x1 && y >= p.erase.y0 && y < p.erase.y1) return 0;
    return -1;
}

}  // namespace gsx
