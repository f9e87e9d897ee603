// kernels_toolset.hip — the query toolset on the device (gfx950): the stroke painted into the viewer's query texture, and the stroke
// overlay / the cursor drawn by the RGBA8 resolve (spec/RENDER_SPEC.md §7, "Toolset"; src/tab/scene.rs:768-791, 2317-2325).
//   k_toolset_paint           one launch per gsx_toolset_render, whatever is pending: one 256-lane workgroup per 16x16 tile of the box that
//                             covers the pending shapes (k_overlay_raster's shape), one texel per lane.  Every wave tests the pending
//                             segments' boxes against its tile once — lane j takes segment j, the ballot is the same in all four waves —
//                             and the lanes walk only the segments that touch the tile.  Texels are bytes, rows are `width` bytes (the
//                             K1 kernels read tex[y * w + x]): plain byte stores, no read-modify-write — every writer writes 255, and the
//                             erased box of a Rect repaint is written by exactly the lanes that own its texels.
//   k_resolve_rgba8_toolset   k_resolve_rgba8 / k_resolve_rgba8_overlay with the stroke overlay or the cursor blended on top, launched only
//                             when one of them is to be drawn.
// The painting rule itself is toolset_math.h, shared with the host restatement of tests/toolset_driver.cpp.
#include "gsx_internal.h"

namespace gsx {

__global__ __launch_bounds__(256) void k_toolset_paint(ToolsetPaint p, uint32_t w, uint32_t h, uint32_t tile_x0, uint32_t tile_y0, uint32_t tiles_x,
                                                        uint8_t* __restrict__ tex) {
    const uint32_t tx = tile_x0 + blockIdx.x % tiles_x, ty = tile_y0 + blockIdx.x / tiles_x;
    const int32_t tx0 = (int32_t)(tx * kTile), ty0 = (int32_t)(ty * kTile);
    const int32_t tx1 = min(tx0 + kTile, (int32_t)w), ty1 = min(ty0 + kTile, (int32_t)h);
    const uint32_t lane = threadIdx.x & 63u;
    bool hit = false;
    if (lane < p.n_segs) {
        const ToolsetBox b = toolset_seg_box(p.seg[lane], w, h);
        hit = b.x0 < tx1 && b.x1 > tx0 && b.y0 < ty1 && b.y1 > ty0;
    }
    const unsigned long long mask = __ballot(hit);
    const uint32_t x = (uint32_t)tx0 + (threadIdx.x & 15u), y = (uint32_t)ty0 + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const int v = toolset_texel(p, (int32_t)x, (int32_t)y, mask);
    if (v >= 0) tex[(size_t)y * w + x] = (uint8_t)v;
}

// The colour k_resolve_rgba8 (overlay == nullptr) or k_resolve_rgba8_overlay rounds, then the toolset's blend, then their rounding.
template <bool kLines>
__global__ __launch_bounds__(256) void k_resolve_rgba8_toolset(const float4* __restrict__ fb, uint32_t first, uint32_t n, uint32_t w,
                                                                uint32_t tiles_x, float br, float bg, float bb,
                                                                const float4* __restrict__ overlay, const uint32_t* __restrict__ tile_flags,
                                                                const uint8_t* __restrict__ tex, ToolsetDraw d, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t px = first + i, x = px % w, y = px / w;
    const float4 p = fb[px];
    float r, g, b, a;
    if (kLines) {
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tile_flags[(y / kTile) * tiles_x + x / kTile]) o = overlay[px];
        const float k = 1.0f - o.w;
        r = fminf(fmaxf(fmaf(p.w, fmaf(k, br, o.x), p.x), 0.0f), 1.0f);
        g = fminf(fmaxf(fmaf(p.w, fmaf(k, bg, o.y), p.y), 0.0f), 1.0f);
        b = fminf(fmaxf(fmaf(p.w, fmaf(k, bb, o.z), p.z), 0.0f), 1.0f);
        a = fminf(fmaxf(1.0f - p.w * k, 0.0f), 1.0f);
    } else {
        r = fminf(fmaxf(fmaf(p.w, br, p.x), 0.0f), 1.0f);
        g = fminf(fmaxf(fmaf(p.w, bg, p.y), 0.0f), 1.0f);
        b = fminf(fmaxf(fmaf(p.w, bb, p.z), 0.0f), 1.0f);
        a = fminf(fmaxf(1.0f - p.w, 0.0f), 1.0f);
    }
    bool cover = false;
    if (d.mode == kToolsetDrawStroke) {  // (the texture has the frame's size; rows past it — an external framebuffer's padding — have no texel)
        cover = y < d.tex_h && tex[(size_t)y * w + x] != 0;
    } else {
        const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
        if (d.mode == kToolsetDrawRing) {
            const float ex = cx - d.x0, ey = cy - d.y0;
            cover = fabsf(sqrtf(ex * ex + ey * ey) - d.radius) <= d.half_thickness;
        } else {  // the rectangle's outline: within half_thickness of its boundary, Chebyshev, inside or outside
            const float t = d.half_thickness;
            const bool outer = cx >= d.x0 - t && cx <= d.x1 + t && cy >= d.y0 - t && cy <= d.y1 + t;
            const bool inner = cx > d.x0 + t && cx < d.x1 - t && cy > d.y0 + t && cy < d.y1 - t;
            cover = outer && !inner;
        }
    }
    if (cover) {  // straight alpha: rgb' = rgb (1 - O.a) + O.rgb O.a, a' = a (1 - O.a) + O.a
        const float k = 1.0f - d.rgba[3];
        r = fmaf(r, k, d.rgba[0] * d.rgba[3]);
        g = fmaf(g, k, d.rgba[1] * d.rgba[3]);
        b = fmaf(b, k, d.rgba[2] * d.rgba[3]);
        a = fmaf(a, k, d.rgba[3]);
    }
    uint32_t R = (uint32_t)floorf(r * 255.0f + 0.5f), G = (uint32_t)floorf(g * 255.0f + 0.5f);
    uint32_t B = (uint32_t)floorf(b * 255.0f + 0.5f), A = (uint32_t)floorf(a * 255.0f + 0.5f);
    out[i] = R | (G << 8) | (B << 16) | (A << 24);
}

hipError_t launch_toolset_paint(hipStream_t s, const ToolsetPaint& p, const ToolsetBox& cover, uint32_t w, uint32_t h, uint8_t* tex) {
    if (toolset_box_empty(cover)) return hipSuccess;
    // (the box is clamped to the texture: every tile of the grid holds a texel)
    const uint32_t tx0 = (uint32_t)cover.x0 / kTile, ty0 = (uint32_t)cover.y0 / kTile;
    const uint32_t tx1 = ((uint32_t)cover.x1 + kTile - 1) / kTile, ty1 = ((uint32_t)cover.y1 + kTile - 1) / kTile;
    GSX_LAUNCH(k_toolset_paint, dim3((tx1 - tx0) * (ty1 - ty0)), dim3(256), 0, s, p, w, h, tx0, ty0, tx1 - tx0, tex);
    return hipGetLastError();
}

hipError_t launch_resolve_rgba8_toolset(hipStream_t s, const float4* fb, uint32_t first, uint32_t n_px, uint32_t w, float bg_r, float bg_g,
                                        float bg_b, const float4* overlay_rgba, const uint32_t* tile_flags, const uint8_t* tex,
                                        const ToolsetDraw& d, uint32_t* out_rgba8) {
    if (!n_px) return hipSuccess;
    if (overlay_rgba)
        GSX_LAUNCH(k_resolve_rgba8_toolset<true>, dim3((n_px + 255) / 256), dim3(256), 0, s, fb, first, n_px, w, (w + kTile - 1) / kTile, bg_r, bg_g,
                   bg_b, overlay_rgba, tile_flags, tex, d, out_rgba8);
    else
        GSX_LAUNCH(k_resolve_rgba8_toolset<false>, dim3((n_px + 255) / 256), dim3(256), 0, s, fb, first, n_px, w, (w + kTile - 1) / kTile, bg_r, bg_g,
                   bg_b, overlay_rgba, tile_flags, tex, d, out_rgba8);
    return hipGetLastError();
}

}  // namespace gsx
