// gsx_api_overlay.cpp — C ABI for the overlay lines and the mask gizmos: the app's measurement pass (MeasurementRenderer,
// src/renderer/measurement.rs) and its gizmo pass (gs::MaskGizmo, src/tab/scene.rs:2141-2166), drawn by the library where a frame's depth
// snapshot is taken (depth_snapshot, gsx_frame.cpp; kernels_overlay.hip; spec §9 and §10).
#include <cmath>
#include <vector>

#include "gsx_state.h"

using namespace gsx;

static_assert(sizeof(gsx_overlay_line) == 32, "gsx_overlay_line is the reference's 32-byte HitPair");
static_assert(sizeof(gsx_mask_gizmo) == 64, "gsx_mask_gizmo is 64 bytes: four uint4 on the device");
static_assert(GSX_GIZMO_CIRCLE_SEGMENTS == kGizmoCircleSegs && GSX_MASK_BOX == kGizmoKindBox && GSX_MASK_ELLIPSOID == kGizmoKindEllipsoid,
              "gizmo_math.h restates gsx.h's constants");

extern "C" {

gsx_status gsx_viewer_set_overlay_lines(gsx_viewer* v, const gsx_overlay_line* lines, uint32_t n) {
    // (viewer_bind: frames in flight on lanes finish first — the next frame runs on the viewer itself while lines are set)
    gsx_status st = viewer_bind(v);
    if (st) return st;
    if (v->parent) return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_overlay_lines: called on a lane");
    if (n > GSX_OVERLAY_MAX_LINES)
        return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_overlay_lines: %u overlay lines, at most %u", n, GSX_OVERLAY_MAX_LINES);
    if (n && !lines) return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_overlay_lines: null overlay lines");
    if (!n && !v->overlay_n) return GSX_OK;  // nothing was set, nothing is: not a change
    if (n) {
        HIPCHK(gsx::op::StreamSynchronize(v->stream));  // (the set-up launch of a frame in flight may still read the old lines)
        HIPCHK(v->overlay_lines.ensure(sizeof(gsx_overlay_line) * (size_t)n));
        HIPCHK(gsx::op::MemcpyAsync(v->overlay_lines.p, lines, sizeof(gsx_overlay_line) * (size_t)n, hipMemcpyHostToDevice, v->stream));
        HIPCHK(gsx::op::StreamSynchronize(v->stream));
    }
    v->overlay_n = n;
    v->depth_cfg += 1;  // (frames preprocessed with the old lines are refused by gsx_render)
    return GSX_OK;
}

gsx_status gsx_viewer_set_mask_gizmos(gsx_viewer* v, const gsx_mask_gizmo* gizmos, uint32_t n) {
    // (viewer_bind, the lane, "not a change", depth_cfg: as gsx_viewer_set_overlay_lines)
    gsx_status st = viewer_bind(v);
    if (st) return st;
    if (v->parent) return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_mask_gizmos: called on a lane");
    if (n > GSX_GIZMO_MAX_SHAPES)
        return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_mask_gizmos: %u mask gizmos, at most %u", n, GSX_GIZMO_MAX_SHAPES);
    if (n && !gizmos) return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_mask_gizmos: null mask gizmos");
    if (!n && !v->gizmo_n) return GSX_OK;
    uint32_t segs = 0;
    if (n) {
        // the device buffer: circle table | first-record offsets | shapes
        std::vector<uint8_t> host(kGizmoShapesAt + sizeof(gsx_mask_gizmo) * (size_t)n);
        gizmo_circle_table(reinterpret_cast<GizmoCircle*>(host.data()));
        uint32_t* off = reinterpret_cast<uint32_t*>(host.data() + kGizmoOffsetsAt);
        for (uint32_t i = 0; i < n; ++i) {
            const gsx_mask_gizmo& g = gizmos[i];
            if (g.kind != GSX_MASK_BOX && g.kind != GSX_MASK_ELLIPSOID)
                return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_mask_gizmos: mask gizmo %u has kind %u (0 box, 1 ellipsoid)", i, g.kind);
            bool finite = std::isfinite(g.line_width);
            for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(g.pos[k]) && std::isfinite(g.scale[k]);
            for (int k = 0; k < 4; ++k) finite = finite && std::isfinite(g.quat_xyzw[k]) && std::isfinite(g.color[k]);
            if (!finite) return fail(GSX_ERR_INVALID_ARG, "gsx_viewer_set_mask_gizmos: mask gizmo %u has a field that is not finite", i);
            off[i] = segs;
            segs += gizmo_segment_count(g.kind);
        }
        off[n] = segs;
        memcpy(host.data() + kGizmoShapesAt, gizmos, sizeof(gsx_mask_gizmo) * (size_t)n);
        HIPCHK(gsx::op::StreamSynchronize(v->stream));  // (the set-up launch of a frame in flight may still read the old shapes)
        HIPCHK(v->gizmo_buf.ensure(host.size()));
        HIPCHK(gsx::op::MemcpyAsync(v->gizmo_buf.p, host.data(), host.size(), hipMemcpyHostToDevice, v->stream));
        HIPCHK(gsx::op::StreamSynchronize(v->stream));
    }
    v->gizmo_n = n;
    v->gizmo_segs = segs;
    v->gizmo_rec = (segs + 63u) / 64u * 64u;  // undrawn records up to a whole batch: the lines' records start on a batch boundary
    v->depth_cfg += 1;  // (frames preprocessed with the old gizmos are refused by gsx_render)
    return GSX_OK;
}

gsx_status gsx_download_overlay(gsx_viewer* v, float* rgba, float* depth) {
    gsx_status st = viewer_bind(v);
    if (st) return st;
    if ((st = finish_frame(v))) return st;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    const bool drawn = v->overlay_valid && !v->latest && v->overlay_w == v->width && v->overlay_h == v->height;
    const uint32_t w = v->width, h = v->height;
    const size_t npx = (size_t)w * h;
    if (rgba) {
        if (drawn) {
            const uint32_t tiles_x = (w + GSX_TILE - 1) / GSX_TILE, tiles_y = (h + GSX_TILE - 1) / GSX_TILE;
            std::vector<uint32_t> flags((size_t)tiles_x * tiles_y);
            HIPCHK(gsx::op::Memcpy(flags.data(), v->overlay_flags.p, 4 * flags.size(), hipMemcpyDeviceToHost));
            HIPCHK(gsx::op::Memcpy(rgba, v->overlay_rgba.p, sizeof(float4) * npx, hipMemcpyDeviceToHost));
            for (uint32_t ty = 0; ty < tiles_y; ++ty)  // tiles no line touches hold nothing on the device: zeros
                for (uint32_t tx = 0; tx < tiles_x; ++tx) {
                    if (flags[(size_t)ty * tiles_x + tx]) continue;
                    const uint32_t x0 = tx * GSX_TILE, x1 = std::min(x0 + GSX_TILE, w);
                    for (uint32_t y = ty * GSX_TILE; y < std::min((ty + 1) * GSX_TILE, h); ++y)
                        memset(rgba + 4 * ((size_t)y * w + x0), 0, sizeof(float) * 4 * (x1 - x0));
                }
        } else {
            memset(rgba, 0, sizeof(float) * 4 * npx);
        }
    }
    if (depth) {
        const float* src = v->depth_dev ? v->depth_dev : v->depth_owned.as<float>();
        if (drawn) {
            HIPCHK(gsx::op::Memcpy(depth, v->overlay_eff.p, 4 * npx, hipMemcpyDeviceToHost));
        } else if (src && v->depth_w == w && v->depth_h == h) {  // no overlay: E = D
            const uint64_t pitch = v->depth_dev ? v->depth_pitch : 4ull * w;
            for (uint32_t y = 0; y < h; ++y)
                HIPCHK(gsx::op::Memcpy(depth + (size_t)y * w, reinterpret_cast<const char*>(src) + y * pitch, 4ull * w, hipMemcpyDeviceToHost));
        } else {
            for (size_t i = 0; i < npx; ++i) depth[i] = 1.0f;
        }
    }
    return GSX_OK;
}

gsx_status gsx_overlay_device_ptrs(gsx_viewer* v, void** rgba, void** tile_flags, void** depth) {
    gsx_status st = viewer_bind(v);
    if (st) return st;
    if (!v->overlay_valid || v->latest)
        return fail(GSX_ERR_INVALID_ARG, "gsx_overlay_device_ptrs: the last frame drew no overlay lines or mask gizmos (gsx_viewer_set_overlay_lines / "
                    "gsx_viewer_set_mask_gizmos, then a frame)");
    if (rgba) *rgba = v->overlay_rgba.p;
    if (tile_flags) *tile_flags = v->overlay_flags.p;
    if (depth) *depth = v->overlay_eff.p;
    return GSX_OK;
}

}  // extern "C"
