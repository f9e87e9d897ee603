// gsx_api_toolset.cpp — C ABI of the query toolset (spec/RENDER_SPEC.md section 7, "Toolset"; toolset_state.h; kernels_toolset.hip):
// gs::QueryToolset's protocol with the strokes painted on the device, into the viewer's query texture.
#include <cmath>

#include "gsx_state.h"

using namespace gsx;

// The toolset calls do NOT come through viewer_bind (as the depth calls do not, gsx_api_shard.cpp): that orders the viewer's stream after
// the lanes' whole frames and the lanes' next frames after the viewer's stream — a stroke painted every frame of a drag would put the
// frames in flight back in single file.  Nothing of a lane reads the query texture: a frame with a query runs on the viewer itself,
// on the stream the paints are enqueued on.
static gsx_status toolset_viewer(gsx_viewer* v, const char* fn) {
    if (!v) return fail(GSX_ERR_INVALID_ARG, "%s: viewer is null", fn);
    if (v->parent) return fail(GSX_ERR_INVALID_ARG, "%s: called on a lane", fn);
    return GSX_OK;
}

// Enqueues what is queued as one launch (and the clear in front of it); (re)allocates and zero-fills the texture when the viewport
// has changed.  No host wait, no host copy.
static gsx_status toolset_flush(gsx_viewer* v) {
    HIPCHK(hipSetDevice(v->device));
    const uint32_t w = v->width, h = v->height;
    const size_t bytes = (size_t)w * h;
    const bool resized = !v->query_texture.p || v->query_tex_w != w || v->query_tex_h != h;
    // (growing frees the old texture, which waits for whatever still reads it; a viewport change is not a per-frame event)
    if (resized) HIPCHK(v->query_texture.ensure(bytes));
    ToolsetPaint paint;
    ToolsetBox cover;
    if (!v->toolset.take(w, h, resized, &paint, &cover)) return GSX_OK;
    if (paint.clear) HIPCHK(gsx::op::MemsetAsync(v->query_texture.p, 0, bytes, v->stream));
    v->query_tex_w = w;
    v->query_tex_h = h;
    HIPCHK(launch_toolset_paint(v->stream, paint, cover, w, h, v->query_texture.as<uint8_t>()));
    return GSX_OK;
}

static bool finite2(const float p[2]) { return std::isfinite(p[0]) && std::isfinite(p[1]); }

extern "C" {

gsx_status gsx_toolset_set_use_texture(gsx_viewer* v, uint32_t on) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_set_use_texture")) return st;
    v->toolset.set_use_texture(on != 0);
    return GSX_OK;
}

gsx_status gsx_toolset_update_brush_radius(gsx_viewer* v, float radius) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_update_brush_radius")) return st;
    if (!std::isfinite(radius) || !(radius > 0.0f)) return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_update_brush_radius: radius %g (needs a finite radius > 0)", (double)radius);
    v->toolset.update_brush_radius(radius);
    return GSX_OK;
}

gsx_status gsx_toolset_start(gsx_viewer* v, uint32_t tool, uint32_t selection_op, const float pos[2]) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_start")) return st;
    if (!pos) return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_start: null position");
    if (tool > GSX_TOOL_BRUSH || selection_op > GSX_SELECTION_REMOVE)
        return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_start: unknown tool %u / selection op %u", tool, selection_op);
    if (!finite2(pos)) return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_start: the position is not finite");
    v->toolset.start(tool, selection_op, pos);
    return GSX_OK;
}

gsx_status gsx_toolset_update_pos(gsx_viewer* v, const float pos[2]) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_update_pos")) return st;
    if (!pos) return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_update_pos: null position");
    if (!finite2(pos)) return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_update_pos: the position is not finite");
    v->toolset.update_pos(pos);
    if (v->toolset.full()) return toolset_flush(v);  // the queue is full: this call enqueues the paint itself — nothing is dropped
    return GSX_OK;
}

gsx_status gsx_toolset_end(gsx_viewer* v) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_end")) return st;
    v->toolset.end();
    return GSX_OK;
}

gsx_status gsx_toolset_query(gsx_viewer* v, gsx_query* out) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_query")) return st;
    if (!out) return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_query: null argument");
    *out = v->toolset.query();
    return GSX_OK;
}

gsx_status gsx_toolset_state(gsx_viewer* v, uint32_t* active, uint32_t* tool, uint32_t* selection_op, float start[2], float pos[2]) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_state")) return st;
    const ToolsetState& t = v->toolset;
    if (active) *active = t.active() ? 1u : 0u;
    if (!t.active()) return GSX_OK;
    if (tool) *tool = t.tool;
    if (selection_op) *selection_op = t.op;
    if (start) memcpy(start, t.start_pos, sizeof t.start_pos);
    if (pos) memcpy(pos, t.pos, sizeof t.pos);
    return GSX_OK;
}

gsx_status gsx_toolset_render(gsx_viewer* v) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_render")) return st;
    return toolset_flush(v);
}

gsx_status gsx_toolset_set_overlay(gsx_viewer* v, const float texture_rgba[4], const float cursor_rgba[4], float cursor_thickness) {
    if (gsx_status st = toolset_viewer(v, "gsx_toolset_set_overlay")) return st;
    if (!texture_rgba || !cursor_rgba) return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_set_overlay: null colour");
    for (int k = 0; k < 4; ++k)
        if (!(texture_rgba[k] >= 0.0f && texture_rgba[k] <= 1.0f) || !(cursor_rgba[k] >= 0.0f && cursor_rgba[k] <= 1.0f))
            return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_set_overlay: colour components must lie in [0, 1]");
    if (!std::isfinite(cursor_thickness) || cursor_thickness < 0.0f)
        return fail(GSX_ERR_INVALID_ARG, "gsx_toolset_set_overlay: cursor thickness %g (needs a finite thickness >= 0)", (double)cursor_thickness);
    memcpy(v->toolset.texture_rgba, texture_rgba, sizeof v->toolset.texture_rgba);
    memcpy(v->toolset.cursor_rgba, cursor_rgba, sizeof v->toolset.cursor_rgba);
    v->toolset.cursor_thickness = cursor_thickness;
    return GSX_OK;
}

gsx_status gsx_download_query_texture(gsx_viewer* v, uint8_t* texels, uint32_t width, uint32_t height) {
    gsx_status st = viewer_bind(v);
    if (st) return st;
    if (!texels || !v->query_texture.p || width != v->query_tex_w || height != v->query_tex_h)
        return fail(GSX_ERR_INVALID_ARG, "gsx_download_query_texture: the query texture is %ux%u", v->query_tex_w, v->query_tex_h);
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    HIPCHK(gsx::op::Memcpy(texels, v->query_texture.p, (size_t)width * height, hipMemcpyDeviceToHost));
    return GSX_OK;
}

}  // extern "C"
