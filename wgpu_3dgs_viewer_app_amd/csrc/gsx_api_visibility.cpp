// gsx_api_visibility.cpp — C ABI of the per-Gaussian visibility (spec/RENDER_SPEC.md section 24; kernels_visibility.hip):
// gsx_model_visibility, gsx_model_select_visibility and gsx_model_visibility_reset.  (FrameIsolation, the save and restore around the view's
// frame, is frame_isolation.h's: gsx_api_depthmap.cpp uses it too.)
// The view is the model's own frame: preprocess, full depth sort and binning by tile as ONE unspeculated slab (a progressive = 0
// frame: do_preprocess / do_sort / do_render, unedited), with the framebuffer redirected to v->vis_fb, the query switched off and
// everything the frame changes on the viewer put back afterwards; k_vis_tiles then walks the complete per-tile lists that frame left
// in m->ranges / m->tile_list.  The planes belong to the model (Model::vis); the workspace is the viewer's (v->vis_ws): [the call's
// words, 128 B | the select's partials, 32 B per 1024 Gaussians | the view's transmittance, 4 B a pixel].
#include <cmath>

#include "frame_isolation.h"
#include "gsx_state.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_visibility_desc) == 16 && sizeof(gsx_visibility_select_desc) == 32 && sizeof(gsx_visibility_stats_t) == 40, "spec section 24's layouts");
static_assert(4 * kVisWords == 128, "the words are one 128-byte line");

constexpr size_t kWsPartials = 4 * kVisWords;
size_t ws_transmittance(uint64_t n) { return kWsPartials + extract_pad128(4 * kSelectPartialWords * (size_t)extract_groups(n)); }

// bind, find, refuse what the call does not draw (include/gsx.h: out of scope by design)
gsx_status visibility_model(gsx_viewer* v, const char* fn, const char* key, Model** out) {
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    if (v->parent) return fail(GSX_ERR_INVALID_ARG, "%s: called on a lane", fn);
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "%s: no model '%s'", fn, key);
    *out = m;
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_visibility_desc_default(gsx_visibility_desc* d) {
    if (!d) return;
    *d = gsx_visibility_desc{};
}

void gsx_visibility_select_desc_default(gsx_visibility_select_desc* d) {
    if (!d) return;
    *d = gsx_visibility_select_desc{};
    d->measure = GSX_VIS_PEAK;
    d->selection_op = GSX_SELECTION_SET;
    d->lo = 1.401298464324817e-45;  // the smallest positive float: every Gaussian that was seen at all
    d->hi = INFINITY;
}

gsx_status gsx_model_visibility(gsx_viewer* v, const char* key, const gsx_visibility_desc* desc, float* out_peak, double* out_weight, uint32_t* out_pixels,
                                float* out_transmittance, gsx_visibility_stats_t* out) {
    const char* fn = "gsx_model_visibility";
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (desc->flags & ~(uint32_t)GSX_VIS_ACCUMULATE) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", fn, desc->flags);
    if (desc->reserved[0] | desc->reserved[1] | desc->reserved[2]) return fail(GSX_ERR_INVALID_ARG, "%s: a reserved word is not 0", fn);
    Model* m = nullptr;
    gsx_status st = visibility_model(v, fn, key, &m);
    if (st) return st;
    // out of scope, by design (include/gsx.h)
    if (v->depth_compare != GSX_DEPTH_ALWAYS)
        return fail(GSX_ERR_INVALID_ARG, "%s: the depth test is not part of the visibility (gsx_viewer_set_depth_test(v, GSX_DEPTH_ALWAYS) first)", fn);
    if ((st = overlay_refuses(v, fn, "the visibility does"))) return st;
    if (v->band_lo != 0 || v->band_hi != 0xFFFFFFFFu) return fail(GSX_ERR_INVALID_ARG, "%s: a band is set (gsx_viewer_set_band)", fn);
    if (v->ext_fb) return fail(GSX_ERR_INVALID_ARG, "%s: an external framebuffer is set", fn);
    if (model_is_shard(m) || has_comm(v)) return fail(GSX_ERR_INVALID_ARG, "%s: model '%s' is a shard of a multi-GPU frame, or the viewer has a communicator", fn, key);
    const bool accumulate = (desc->flags & GSX_VIS_ACCUMULATE) != 0 && m->vis.p != nullptr;
    const uint64_t npx = (uint64_t)v->width * v->height;
    if (accumulate && ((uint64_t)m->vis_views + 1u) * npx >= (1ull << 32))
        return fail(GSX_ERR_INVALID_ARG, "%s: %u views of %ux%u pixels: the pixel plane would wrap", fn, m->vis_views + 1u, v->width, v->height);
    if (!accumulate && npx >= (1ull << 32)) return fail(GSX_ERR_INVALID_ARG, "%s: a viewport of %ux%u pixels: the pixel plane would wrap", fn, v->width, v->height);
    const uint64_t n = m->n;
    if (out) *out = gsx_visibility_stats_t{};

    // everything that can fail for memory, before anything of the model changes
    const size_t ws_t = ws_transmittance(n);
    HIPCHK(v->vis_ws.ensure(ws_t + 4 * (size_t)npx));
    const bool fresh = m->vis.p == nullptr;
    HIPCHK(m->vis.ensure(16 * std::max<size_t>((size_t)n, 1)));
    if (fresh) {  // (a failure below leaves all-zero planes of no view)
        m->vis_views = 0;
        HIPCHK(gsx::op::MemsetAsync(m->vis.p, 0, 16 * std::max<size_t>((size_t)n, 1), v->stream));
    }
    uint32_t* words = v->vis_ws.as<uint32_t>();
    float* d_trans = reinterpret_cast<float*>(v->vis_ws.as<char>() + ws_t);
    const VisPlanes planes = vis_planes(m->vis.p, n);
    uint64_t n_visible = 0;
    {
        FrameIsolation iso(v, m);
        const char* keys[1] = {key};
        if ((st = do_preprocess(v, m))) return st;
        if ((st = do_sort(v, m))) return st;
        if ((st = do_render(v, keys, 1))) return st;
        // the host catches up: the counts of this view; a frame whose lists overflowed the pair buffers is redone with larger ones
        if ((st = finish_frame(v))) return st;
        if (!m->binned || !m->lists_complete || m->h_counters->overflow)
            return fail(GSX_ERR_OOM, "%s: the frame of '%s' left no complete per-tile lists (the tile-pair buffers overflowed at a fixed capacity)", fn, key);
        n_visible = m->n_visible;
    }
    // The frame's state is put back; its records, ranges and lists are still in the model's buffers.  Only now do the planes change
    if (!accumulate) HIPCHK(gsx::op::MemsetAsync(m->vis.p, 0, 16 * std::max<size_t>((size_t)n, 1), v->stream));
    HIPCHK(gsx::op::MemsetAsync(words, 0, 4 * kVisWords, v->stream));
    {
        // (a caller that times the passes — gsx_set_pass_timing — reads the walk alone as the composite pass: tools/bench_visibility.py
        //  puts it beside k_composite over the same lists; the frame above is timed under no pass)
        ScopedPass t(v, GSX_PASS_COMPOSITE);
        HIPCHK(launch_vis_tiles(v->stream, m->fc, m->ranges.as<uint2>(), m->tile_list, m->proj_rec(), planes, d_trans, words));
    }
    HIPCHK(launch_vis_stats(v->stream, n, planes, words));
    m->vis_views = accumulate ? m->vis_views + 1u : 1u;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t host[kVisWords];
    HIPCHK(gsx::op::Memcpy(host, words, sizeof host, hipMemcpyDeviceToHost));
    if (out) {
        out->n_visible = n_visible;
        out->n_seen = host[kVisSeen];
        memcpy(&out->n_pairs, host + kVisPairs, 8);
        memcpy(&out->weight_fixed, host + kVisWeight, 8);
        memcpy(&out->peak_max, host + kVisPeakMax, 4);
        out->views = m->vis_views;
    }
    if (n && out_peak) HIPCHK(gsx::op::Memcpy(out_peak, planes.peak, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (n && out_pixels) HIPCHK(gsx::op::Memcpy(out_pixels, planes.pixels, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (n && out_weight) {
        std::vector<unsigned long long> fixed((size_t)n);
        HIPCHK(gsx::op::Memcpy(fixed.data(), planes.weight, 8 * (size_t)n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < (size_t)n; ++i) out_weight[i] = (double)fixed[i] * (1.0 / 16777216.0);
    }
    if (out_transmittance) HIPCHK(gsx::op::Memcpy(out_transmittance, d_trans, 4 * (size_t)npx, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_model_select_visibility(gsx_viewer* v, const char* key, const gsx_visibility_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected) {
    const char* fn = "gsx_model_select_visibility";
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (desc->measure > (uint32_t)GSX_VIS_PIXELS) return fail(GSX_ERR_INVALID_ARG, "%s: unknown measure %u", fn, desc->measure);
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, desc->filter);
    gsx_status st = check_selection_op(fn, desc->selection_op);
    if (st) return st;
    if (desc->reserved != 0u) return fail(GSX_ERR_INVALID_ARG, "%s: reserved is %u, not 0", fn, desc->reserved);
    if (!(desc->lo <= desc->hi))  // (a NaN bound compares false)
        return fail(GSX_ERR_INVALID_ARG, "%s: the range [%g, %g] is reversed or NaN", fn, desc->lo, desc->hi);
    Model* m = nullptr;
    if ((st = visibility_model(v, fn, key, &m))) return st;
    if (has_comm(v) || model_is_shard(m)) return fail(GSX_ERR_INVALID_ARG, "%s: model '%s' is a shard of a multi-GPU frame, or the viewer has a communicator", fn, key);
    if (!m->vis.p) return fail(GSX_ERR_INVALID_ARG, "%s: model '%s' has no visibility planes (gsx_model_visibility first; an upload, an import, a transform or a pod kind change drops them)", fn, key);
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    HIPCHK(v->vis_ws.ensure(ws_transmittance(n)));  // (before anything of the model changes)
    uint32_t* words = v->vis_ws.as<uint32_t>();
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    VisSelectJob job{};
    job.planes = vis_planes(m->vis.p, n);
    job.measure = desc->measure;
    job.lo = desc->lo;
    job.hi = desc->hi;
    job.words = words;
    if ((st = select_begin(v, m, desc->selection_op, reinterpret_cast<uint32_t*>(v->vis_ws.as<char>() + kWsPartials), &job.sel))) return st;
    HIPCHK(launch_vis_select(v->stream, n, f, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(m);
    uint32_t host[kVisWords];
    HIPCHK(gsx::op::Memcpy(host, words, sizeof host, hipMemcpyDeviceToHost));
    if (out_hit) *out_hit = host[kVisHit];
    if (out_selected) *out_selected = host[kVisSelected];
    return GSX_OK;
}

gsx_status gsx_model_visibility_reset(gsx_viewer* v, const char* key) {
    const char* fn = "gsx_model_visibility_reset";
    if (!v || !key) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    Model* m = nullptr;
    gsx_status st = visibility_model(v, fn, key, &m);
    if (st) return st;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    drop_visibility(m);
    return GSX_OK;
}

}  // extern "C"
