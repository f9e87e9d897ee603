// toolset_state.h — the query toolset's state machine and its queue of pending paint operations (spec/RENDER_SPEC.md §7, "Toolset").
// Pure host C++, no HIP include (tests/toolset_driver.cpp plays scripts against it on the CPU); gsx_viewer holds one instance and
// gsx_api_toolset.cpp turns what take() hands out into one k_toolset_paint launch.
//
// The protocol is gs::QueryToolset's as the app drives it (src/tab/scene.rs:766-791): start / update_pos / end, one query() per frame.
// start and update_pos queue what they paint; nothing is ever dropped — when the queue is full() the owner flushes it at once.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gsx.h"
#include "toolset_math.h"

namespace gsx {

struct ToolsetState {
    static constexpr uint32_t kNoTool = 0xFFFFFFFFu;
    // -- gs::QueryToolset --
    bool use_texture = true;
    float brush_radius = 40.0f;
    uint32_t tool = kNoTool, op = GSX_SELECTION_SET;
    float start_pos[2] = {0, 0}, prev[2] = {0, 0}, pos[2] = {0, 0};
    bool ended = false;
    // the cursor: the last position start or update_pos reported, tool or not
    bool cursor_known = false;
    float cursor[2] = {0, 0};
    // -- the overlay's parameters (gsx_toolset_set_overlay); alpha 0: not drawn --
    float texture_rgba[4] = {0, 0, 0, 0}, cursor_rgba[4] = {0, 0, 0, 0};
    float cursor_thickness = 1.0f;
    // -- pending paint operations, in order: [clear] then the brush segments / the latest rectangle --
    bool pend_clear = false, pend_rect = false;
    float rect[4] = {0, 0, 0, 0};  // sorted: x0, y0, x1, y1
    uint32_t n_segs = 0;
    ToolsetSeg segs[kToolsetMaxSegs];
    // -- what the texture holds: the box painted since it was last cleared (a Rect repaint erases it) --
    ToolsetBox dirty{0, 0, 0, 0};

    bool active() const { return tool != kNoTool; }
    bool full() const { return n_segs == kToolsetMaxSegs; }
    bool pending() const { return pend_clear || pend_rect || n_segs != 0; }
    // a texture-tool stroke is being drawn: from start to the query() that hands out the Texture query
    bool stroke_shown() const { return active() && use_texture; }

    void set_use_texture(bool on) { use_texture = on; }
    void update_brush_radius(float r) { brush_radius = r; }

    void start(uint32_t tool_, uint32_t op_, const float p[2]) {
        tool = tool_;
        op = op_;
        for (int k = 0; k < 2; ++k) start_pos[k] = prev[k] = pos[k] = cursor[k] = p[k];
        cursor_known = true;
        ended = false;
        // the texture is cleared whatever the mode: what was queued before would be wiped anyway
        pend_clear = true;
        pend_rect = false;
        n_segs = 0;
        paint();
    }

    // (the owner checks full() afterwards and flushes: the next segment finds room)
    void update_pos(const float p[2]) {
        cursor[0] = p[0];
        cursor[1] = p[1];
        cursor_known = true;
        if (!active()) return;
        prev[0] = pos[0];
        prev[1] = pos[1];
        pos[0] = p[0];
        pos[1] = p[1];
        paint();
    }

    void end() { ended = active(); }

    // this frame's query; after end() in texture mode the one Texture query, then None
    gsx_query query() {
        gsx_query q;
        memset(&q, 0, sizeof q);
        q.kind = GSX_QUERY_NONE;
        if (!active()) return q;
        if (use_texture) {
            if (ended) {
                tool = kNoTool;
                q.kind = GSX_QUERY_TEXTURE;
                q.selection_op = op;
            }
            return q;
        }
        if (ended) {
            tool = kNoTool;
            return q;
        }
        q.selection_op = op;
        if (tool == GSX_TOOL_RECT) {
            q.kind = GSX_QUERY_RECT;
            q.p0[0] = start_pos[0]; q.p0[1] = start_pos[1];
            q.p1[0] = pos[0]; q.p1[1] = pos[1];
        } else {
            q.kind = GSX_QUERY_BRUSH;
            q.p0[0] = prev[0]; q.p0[1] = prev[1];
            q.p1[0] = pos[0]; q.p1[1] = pos[1];
            q.radius = brush_radius;
        }
        return q;
    }

    // The pending operations as one paint of a w x h texture, and the texel box the launch has to cover (empty: nothing but, perhaps,
    // the clear).  Consumes the queue.  resized: the texture has just been (re)allocated for another viewport — it is cleared, and what
    // was painted is gone.
    bool take(uint32_t w, uint32_t h, bool resized, ToolsetPaint* out, ToolsetBox* cover) {
        ToolsetPaint& p = *out;
        memset(&p, 0, sizeof p);
        *cover = ToolsetBox{0, 0, 0, 0};
        if (!pending() && !resized) return false;
        p.clear = (pend_clear || resized) ? 1u : 0u;
        if (p.clear) dirty = ToolsetBox{0, 0, 0, 0};
        ToolsetBox painted{0, 0, 0, 0};
        if (pend_rect) {
            p.has_rect = 1u;
            p.rx0 = rect[0]; p.ry0 = rect[1]; p.rx1 = rect[2]; p.ry1 = rect[3];
            painted = toolset_box(rect[0], rect[1], rect[2], rect[3], w, h);
            if (!toolset_box_empty(dirty)) {  // every repaint replaces what the texture held
                p.has_erase = 1u;
                p.erase = dirty;
                dirty = ToolsetBox{0, 0, 0, 0};
            }
        }
        p.n_segs = n_segs;
        for (uint32_t j = 0; j < n_segs; ++j) {
            p.seg[j] = segs[j];
            painted = toolset_box_union(painted, toolset_seg_box(segs[j], w, h));
        }
        *cover = p.has_erase ? toolset_box_union(painted, p.erase) : painted;
        dirty = toolset_box_union(dirty, painted);
        pend_clear = pend_rect = false;
        n_segs = 0;
        return true;
    }

private:
    void paint() {
        if (!use_texture) return;
        if (tool == GSX_TOOL_RECT) {
            rect[0] = fminf(start_pos[0], pos[0]);
            rect[1] = fminf(start_pos[1], pos[1]);
            rect[2] = fmaxf(start_pos[0], pos[0]);
            rect[3] = fmaxf(start_pos[1], pos[1]);
            pend_rect = true;
            n_segs = 0;  // (a rectangle replaces everything the stroke painted)
        } else if (n_segs < kToolsetMaxSegs) {
            segs[n_segs++] = ToolsetSeg{prev[0], prev[1], pos[0], pos[1], brush_radius};
        }
    }
};

}  // namespace gsx
