// frame_isolation.h — a model's own frame drawn into scratch, for the calls that walk its complete per-tile lists afterwards
// (gsx_api_visibility.cpp, gsx_api_depthmap.cpp).  The frame is the frame path's, unedited: do_preprocess / do_sort / do_render of
// ONE key as ONE unspeculated slab (progressive = 0, binned by tile), with the framebuffer redirected to v->vis_fb and the query
// switched off; everything that frame changes on the viewer and must not is saved by the constructor and put back by the destructor.
#pragma once
#include "gsx_state.h"

namespace gsx {

// the fields of a DevBuf, exchanged (a DevBuf owns its memory: it is not copied)
inline void swap_buf(DevBuf& a, DevBuf& b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
    std::swap(a.borrowed, b.borrowed);
}

// What the view's frame changes on the viewer and must not: saved by the constructor, put back by the destructor.
struct FrameIsolation {
    gsx_viewer* v;
    Model* m;
    gsx_render_options options;
    gsx_query query;
    gsx_viewer* latest;
    std::vector<std::string> last_keys;
    bool last_render_cont, depth_frame_closed, host_waited;
    uint32_t timing, pass_launches[GSX_PASS_COUNT];
    uint32_t flags_kind, flags_op, slabs_hint, stats_copy_tick;
    bool stats_copy_inflight;
    FrameIsolation(gsx_viewer* v_, Model* m_) : v(v_), m(m_) {
        options = v->options;
        query = v->query;
        latest = v->latest;
        last_keys = v->last_keys;
        last_render_cont = v->last_render_cont;
        depth_frame_closed = v->depth_frame_closed;
        host_waited = v->host_waited;
        timing = v->timing;
        memcpy(pass_launches, v->pass_launches, sizeof pass_launches);
        flags_kind = m->flags_kind;
        flags_op = m->flags_op;
        slabs_hint = m->slabs_hint;
        stats_copy_tick = m->stats_copy_tick;
        stats_copy_inflight = m->stats_copy_inflight;
        v->options.progressive = 0;  // one slab, binned by tile: complete per-tile lists
        v->options.frames_in_flight = 1;
        v->query.kind = GSX_QUERY_NONE;  // the query's flags and hits stay the last frame's
        v->timing = 0;
        swap_buf(v->fb, v->vis_fb);
        // a bracket of the speculation tuner that a gsx_preprocess opened and no gsx_render closed: this frame must not close it
        SpecTuner& t = m->tuner;
        if (t.active) {
            if (t.active->state == 1) {
                t.active->state = 0;
                if (t.active->probe) t.rules.probe_dropped();
            }
            t.active = nullptr;
        }
    }
    ~FrameIsolation() {
        swap_buf(v->fb, v->vis_fb);
        v->options = options;
        v->query = query;
        v->latest = latest;
        v->last_keys = last_keys;
        v->last_render_cont = last_render_cont;
        v->depth_frame_closed = depth_frame_closed;
        v->host_waited = host_waited;
        v->timing = timing;
        memcpy(v->pass_launches, pass_launches, sizeof pass_launches);
        m->flags_kind = flags_kind;
        m->flags_op = flags_op;
        m->slabs_hint = slabs_hint;
        // (a statistics copy this frame started is complete — the call has waited — and speaks of no frame the slab plan cares about)
        if (!stats_copy_inflight) m->stats_copy_inflight = false;
        m->stats_copy_tick = stats_copy_tick;
        // the records, the depth order and the lists are this view's, made without the viewer's query: nothing a later gsx_sort or
        // gsx_render may build on
        m->preprocessed = m->sorted = m->binned = m->lists_complete = false;
    }
    FrameIsolation(const FrameIsolation&) = delete;
    FrameIsolation& operator=(const FrameIsolation&) = delete;
};

}  // namespace gsx
