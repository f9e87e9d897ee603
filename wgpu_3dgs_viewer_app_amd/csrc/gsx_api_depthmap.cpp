// gsx_api_depthmap.cpp — C ABI of the splats' depth per pixel (spec/RENDER_SPEC.md section 25; kernels_depthmap.hip):
// gsx_render_depth_map, gsx_depth_map_device_ptrs and the host-only gsx_depth_map_unproject.
// Every model named is drawn as its own frame (frame_isolation.h: preprocess, full depth sort and binning by tile as ONE unspeculated
// slab into v->vis_fb — only a front model without carry keeps complete lists), then k_depth_tiles walks the models' lists nearest
// model first, carrying T, A, S and the crossing from model to model in the viewer's planes (v->depth_map: [the call's words, 128 B |
// surface | sum | alpha | transmittance | index | layer | ndc], 4 B a pixel each).  All frames are drawn before the first walk, so a
// frame that fails leaves the planes as they were.
#include <cmath>

#include "frame_isolation.h"
#include "gsx_state.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_depth_map_desc) == 16 && sizeof(gsx_depth_map_stats_t) == 32, "spec section 25's layouts");
static_assert(4 * kDepthMapWords == 128, "the words are one 128-byte line");

constexpr size_t kWords = 4 * kDepthMapWords;
constexpr uint32_t kPlanes = 7;

float* plane(const gsx_viewer* v, uint32_t k, size_t npx) { return reinterpret_cast<float*>(v->depth_map.as<char>() + kWords) + (size_t)k * npx; }
DepthMapPlanes planes_of(const gsx_viewer* v, size_t npx) {
    DepthMapPlanes p;
    p.surface = plane(v, 0, npx);
    p.sum = plane(v, 1, npx);
    p.alpha = plane(v, 2, npx);
    p.transmittance = plane(v, 3, npx);
    p.index = reinterpret_cast<uint32_t*>(plane(v, 4, npx));
    p.layer = reinterpret_cast<uint32_t*>(plane(v, 5, npx));
    return p;
}

// the depth test's projection class (gsx_frame.cpp, depth_snapshot): z_ndc = P23 / d - P22 grows with d towards 1
bool depth_projection(const float* P) {
    return P[2] == 0.0f && P[6] == 0.0f && P[3] == 0.0f && P[7] == 0.0f && P[15] == 0.0f && P[11] == -1.0f && P[14] < 0.0f && P[10] <= -1.0f;
}

// a 4 x 4 system in double, Gauss-Jordan with partial pivoting: x = M^-1 b (M row-major).  false: M is singular
bool solve4(double M[4][4], double b[4]) {
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
        if (!(std::fabs(M[p][c]) > 0.0)) return false;
        if (p != c) {
            for (int k = 0; k < 4; ++k) std::swap(M[p][k], M[c][k]);
            std::swap(b[p], b[c]);
        }
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double fct = M[r][c] / M[c][c];
            for (int k = c; k < 4; ++k) M[r][k] -= fct * M[c][k];
            b[r] -= fct * b[c];
        }
    }
    for (int c = 0; c < 4; ++c) b[c] /= M[c][c];
    return true;
}

}  // namespace

extern "C" {

void gsx_depth_map_desc_default(gsx_depth_map_desc* d) {
    if (!d) return;
    *d = gsx_depth_map_desc{};
    d->threshold = 0.5f;
}

gsx_status gsx_render_depth_map(gsx_viewer* v, const char* const* keys_far_to_near, uint32_t n_keys, const gsx_depth_map_desc* desc, float* out_surface,
                                float* out_sum, float* out_alpha, float* out_transmittance, uint32_t* out_index, uint32_t* out_layer,
                                gsx_depth_map_stats_t* out) {
    const char* fn = "gsx_render_depth_map";
    if (!v || !keys_far_to_near || !desc) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (n_keys == 0) return fail(GSX_ERR_INVALID_ARG, "%s: no keys", fn);
    if (desc->flags & ~(uint32_t)GSX_DEPTH_MAP_NDC) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", fn, desc->flags);
    if (desc->reserved[0] | desc->reserved[1]) return fail(GSX_ERR_INVALID_ARG, "%s: a reserved word is not 0", fn);
    for (uint32_t i = 0; i < n_keys; ++i) {
        if (!keys_far_to_near[i]) return fail(GSX_ERR_INVALID_ARG, "%s: key %u is null", fn, i);
        for (uint32_t j = 0; j < i; ++j)
            if (!strcmp(keys_far_to_near[i], keys_far_to_near[j])) return fail(GSX_ERR_INVALID_ARG, "%s: key '%s' is named twice", fn, keys_far_to_near[i]);
    }
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    if (v->parent) return fail(GSX_ERR_INVALID_ARG, "%s: called on a lane", fn);
    const float t_eps = v->params.t_epsilon;
    if (!std::isfinite(desc->threshold) || !(desc->threshold >= t_eps) || !(desc->threshold <= 1.0f))
        return fail(GSX_ERR_INVALID_ARG, "%s: the threshold %g is not finite or outside [t_epsilon = %g, 1]", fn, desc->threshold, t_eps);
    std::vector<Model*> models(n_keys);
    for (uint32_t i = 0; i < n_keys; ++i) {
        models[i] = find_model(v, keys_far_to_near[i]);
        if (!models[i]) return fail(GSX_ERR_NOT_FOUND, "%s: no model '%s'", fn, keys_far_to_near[i]);
    }
    // out of scope, by design (include/gsx.h)
    if (v->depth_compare != GSX_DEPTH_ALWAYS)
        return fail(GSX_ERR_INVALID_ARG, "%s: the depth test is not part of the depth map (gsx_viewer_set_depth_test(v, GSX_DEPTH_ALWAYS) first)", fn);
    if ((st = overlay_refuses(v, fn, "the depth map does"))) return st;
    if (v->band_lo != 0 || v->band_hi != 0xFFFFFFFFu) return fail(GSX_ERR_INVALID_ARG, "%s: a band is set (gsx_viewer_set_band)", fn);
    if (v->ext_fb) return fail(GSX_ERR_INVALID_ARG, "%s: an external framebuffer is set", fn);
    for (uint32_t i = 0; i < n_keys; ++i)
        if (model_is_shard(models[i]) || has_comm(v))
            return fail(GSX_ERR_INVALID_ARG, "%s: model '%s' is a shard of a multi-GPU frame, or the viewer has a communicator", fn, keys_far_to_near[i]);
    const bool want_ndc = (desc->flags & GSX_DEPTH_MAP_NDC) != 0;
    if (want_ndc && !depth_projection(v->proj))
        return fail(GSX_ERR_INVALID_ARG, "%s: GSX_DEPTH_MAP_NDC needs the depth test's perspective projection (P20 = P21 = P30 = P31 = P33 = 0, "
                    "P32 = -1, P23 < 0, P22 <= -1, as perspective_rh); this one is not", fn);
    const uint64_t npx64 = (uint64_t)v->width * v->height;
    if (npx64 >= (1ull << 32)) return fail(GSX_ERR_INVALID_ARG, "%s: a viewport of %ux%u pixels: the pixel counts would wrap", fn, v->width, v->height);
    const size_t npx = (size_t)npx64;

    // every model's own frame, before anything of the planes changes: the lists stay in the models' buffers
    for (uint32_t i = n_keys; i-- > 0;) {
        Model* m = models[i];
        FrameIsolation iso(v, m);
        const char* keys[1] = {keys_far_to_near[i]};
        if ((st = do_preprocess(v, m))) return st;
        if ((st = do_sort(v, m))) return st;
        if ((st = do_render(v, keys, 1))) return st;
        // the host catches up: a frame whose lists overflowed the pair buffers is redone with larger ones
        if ((st = finish_frame(v))) return st;
        if (!m->binned || !m->lists_complete || m->h_counters->overflow)
            return fail(GSX_ERR_OOM, "%s: the frame of '%s' left no complete per-tile lists (the tile-pair buffers overflowed at a fixed capacity)", fn,
                        keys_far_to_near[i]);
    }
    // The frames' state is put back; their records, ranges and lists are still in the models' buffers.  Only now do the planes change.
    HIPCHK(v->depth_map.ensure(kWords + 4 * (size_t)kPlanes * npx));
    uint32_t* words = v->depth_map.as<uint32_t>();
    const DepthMapPlanes planes = planes_of(v, npx);
    float* d_ndc = plane(v, 6, npx);
    v->depth_map_w = v->depth_map_h = 0;  // (a failure below leaves no depth map)
    HIPCHK(gsx::op::MemsetAsync(words, 0, kWords, v->stream));
    {
        // (a caller that times the passes — gsx_set_pass_timing — reads the walks alone as the composite pass: tools/bench_depthmap.py
        //  puts them beside k_composite and k_vis_tiles over the same lists; the frames above are timed under no pass)
        ScopedPass t(v, GSX_PASS_COMPOSITE);
        for (uint32_t i = n_keys; i-- > 0;) {
            Model* m = models[i];
            HIPCHK(launch_depth_tiles(v->stream, m->fc, m->ranges.as<uint2>(), m->tile_list, m->proj_rec(), planes, desc->threshold, i, i + 1 == n_keys));
        }
    }
    HIPCHK(launch_depth_finish(v->stream, npx, planes, want_ndc ? d_ndc : nullptr, v->proj[10], v->proj[14], words));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    v->depth_map_w = v->width;
    v->depth_map_h = v->height;
    v->depth_map_ndc = want_ndc;
    uint32_t host[kDepthMapWords];
    HIPCHK(gsx::op::Memcpy(host, words, sizeof host, hipMemcpyDeviceToHost));
    if (out) {
        *out = gsx_depth_map_stats_t{};
        out->n_covered = host[kDepthMapCovered];
        out->n_crossed = host[kDepthMapCrossed];
        const uint32_t lo = ~host[kDepthMapMin];  // (kept inverted, so that the words start as zeros)
        memcpy(&out->surface_min, &lo, 4);
        memcpy(&out->surface_max, host + kDepthMapMax, 4);
        if (!host[kDepthMapCrossed]) out->surface_min = INFINITY;  // (and surface_max = 0)
        out->models = n_keys;
    }
    if (out_surface) HIPCHK(gsx::op::Memcpy(out_surface, planes.surface, 4 * npx, hipMemcpyDeviceToHost));
    if (out_sum) HIPCHK(gsx::op::Memcpy(out_sum, planes.sum, 4 * npx, hipMemcpyDeviceToHost));
    if (out_alpha) HIPCHK(gsx::op::Memcpy(out_alpha, planes.alpha, 4 * npx, hipMemcpyDeviceToHost));
    if (out_transmittance) HIPCHK(gsx::op::Memcpy(out_transmittance, planes.transmittance, 4 * npx, hipMemcpyDeviceToHost));
    if (out_index) HIPCHK(gsx::op::Memcpy(out_index, planes.index, 4 * npx, hipMemcpyDeviceToHost));
    if (out_layer) HIPCHK(gsx::op::Memcpy(out_layer, planes.layer, 4 * npx, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_depth_map_device_ptrs(gsx_viewer* v, void** surface, void** sum, void** alpha, void** transmittance, void** index, void** layer, void** ndc,
                                     uint32_t* width, uint32_t* height) {
    const char* fn = "gsx_depth_map_device_ptrs";
    if (!v) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (v->parent) return fail(GSX_ERR_INVALID_ARG, "%s: called on a lane", fn);
    if (!v->depth_map.p || !v->depth_map_w || v->depth_map_w != v->width || v->depth_map_h != v->height)
        return fail(GSX_ERR_INVALID_ARG, "%s: no depth map of this viewport (gsx_render_depth_map first; a viewport change drops it)", fn);
    const size_t npx = (size_t)v->depth_map_w * v->depth_map_h;
    const DepthMapPlanes p = planes_of(v, npx);
    if (surface) *surface = p.surface;
    if (sum) *sum = p.sum;
    if (alpha) *alpha = p.alpha;
    if (transmittance) *transmittance = p.transmittance;
    if (index) *index = p.index;
    if (layer) *layer = p.layer;
    if (ndc) *ndc = v->depth_map_ndc ? plane(v, 6, npx) : nullptr;
    if (width) *width = v->depth_map_w;
    if (height) *height = v->depth_map_h;
    return GSX_OK;
}

gsx_status gsx_depth_map_unproject(const float view[16], const float proj[16], uint32_t width, uint32_t height, float px, float py, float view_depth,
                                   float out_world[3]) {
    const char* fn = "gsx_depth_map_unproject";
    if (!view || !proj || !out_world) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (width == 0 || height == 0) return fail(GSX_ERR_INVALID_ARG, "%s: an empty viewport", fn);
    if (!std::isfinite(view_depth) || !std::isfinite(px) || !std::isfinite(py)) return fail(GSX_ERR_INVALID_ARG, "%s: a pixel or a depth that is not finite", fn);
    // section 4.6 backwards: ndc from the pixel, then the view-space point with z = -view_depth whose clip x / w and y / w are that ndc
    const double nx = 2.0 * (double)px / (double)width - 1.0, ny = 1.0 - 2.0 * (double)py / (double)height, z = -(double)view_depth;
    auto P = [&](int row, int col) { return (double)proj[col * 4 + row]; };  // column-major
    const double a00 = P(0, 0) - nx * P(3, 0), a01 = P(0, 1) - nx * P(3, 1), b0 = nx * (P(3, 2) * z + P(3, 3)) - (P(0, 2) * z + P(0, 3));
    const double a10 = P(1, 0) - ny * P(3, 0), a11 = P(1, 1) - ny * P(3, 1), b1 = ny * (P(3, 2) * z + P(3, 3)) - (P(1, 2) * z + P(1, 3));
    const double det = a00 * a11 - a01 * a10;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return fail(GSX_ERR_INVALID_ARG, "%s: the projection does not determine x and y", fn);
    const double xv = (b0 * a11 - a01 * b1) / det, yv = (a00 * b1 - b0 * a10) / det;
    double M[4][4], b[4] = {xv, yv, z, 1.0};
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) M[r][c] = (double)view[c * 4 + r];
    if (!solve4(M, b) || !(std::fabs(b[3]) > 0.0)) return fail(GSX_ERR_INVALID_ARG, "%s: the view matrix is singular", fn);
    for (int k = 0; k < 3; ++k) out_world[k] = (float)(b[k] / b[3]);
    return GSX_OK;
}

}  // extern "C"
