// gsx_api_merge.cpp — C ABI of the model merge (spec/RENDER_SPEC.md section 13; kernels_merge.hip, kernels_extract.hip).
#include "gsx_state.h"

#include <vector>

using namespace gsx;

namespace gsx {
void quat_to_rows(const float q[4], float r[9]);  // kernels_project.hip: the float32 R_m of frame_consts_setup
}

namespace {
// one source's part of the workspace: [keep words | partials | bases], each padded to 128 B; the totals of all sources lie in front
struct Region {
    Model* m;
    size_t keep, partials, bases;  // byte offsets into the workspace
    uint64_t groups;
    bool identity;
};
}  // namespace

extern "C" {

gsx_status gsx_model_merge(gsx_viewer* v, const char* const* src_keys, uint32_t n_src, const char* dst_key, const gsx_extract_desc* desc,
                           uint64_t* out_counts, uint64_t* out_total) {
    if (!v || !src_keys || !dst_key || !desc || !out_total) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: null argument");
    if (n_src == 0 || n_src > GSX_MERGE_MAX_SOURCES) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: n_src %u is not in [1, %u]", n_src, GSX_MERGE_MAX_SOURCES);
    if (desc->filter & ~(GSX_BOUNDS_MASKED | GSX_BOUNDS_SKIP_HIDDEN | GSX_BOUNDS_SELECTED))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: unknown filter bits 0x%x", desc->filter);
    if (desc->flags & ~(GSX_EXTRACT_INVERT | GSX_EXTRACT_DROP_EDITS)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: unknown flag bits 0x%x", desc->flags);
    for (uint32_t s = 0; s < n_src; ++s) {
        if (!src_keys[s]) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: src_keys[%u] is null", s);
        if (!strcmp(src_keys[s], dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: dst_key equals src_keys[%u] '%s'", s, dst_key);
    }
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    if (v->models.count(dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: model '%s' exists", dst_key);
    std::vector<Region> src(n_src);
    for (uint32_t s = 0; s < n_src; ++s)  // (a key may appear twice: the same model, instantiated twice)
        if (!(src[s].m = find_model(v, src_keys[s]))) return fail(GSX_ERR_NOT_FOUND, "gsx_model_merge: no model '%s'", src_keys[s]);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_merge: the viewer has a communicator (merge before gsx_viewer_comm_init, or on one GPU)");
    const gsx_sh_kind sh_kind = src[0].m->sh_kind;
    const gsx_cov3d_kind cov_kind = src[0].m->cov_kind;
    size_t ws_bytes = extract_pad128(sizeof(uint64_t) * n_src);
    for (uint32_t s = 0; s < n_src; ++s) {
        Region& r = src[s];
        const Model* m = r.m;
        if (m->shard_win_set || m->shard_limit_valid || m->shard_next_valid || m->shard_override_tiles)
            return fail(GSX_ERR_UNSUPPORTED, "gsx_model_merge: model '%s' is a shard of a multi-GPU frame", src_keys[s]);
        if (m->sh_kind != sh_kind || m->cov_kind != cov_kind)
            return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: model '%s' is a Sh%d/Cov3d%d pod, '%s' a Sh%d/Cov3d%d pod (no conversion between kinds)",
                        src_keys[s], (int)m->sh_kind, (int)m->cov_kind, src_keys[0], (int)sh_kind, (int)cov_kind);
        if (!merge_is_valid(m->mt.pos, m->mt.quat, m->mt.scale))
            return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: the transform of model '%s' has a non-finite component or a zero quaternion", src_keys[s]);
        r.identity = merge_is_identity(m->mt.pos, m->mt.quat, m->mt.scale);
        r.groups = extract_groups(m->n);
        r.keep = ws_bytes;
        r.partials = r.keep + extract_pad128(4 * (size_t)((m->n + 31) / 32));
        r.bases = r.partials + extract_pad128(4 * (size_t)r.groups);
        ws_bytes = r.bases + extract_pad128(4 * (size_t)r.groups);
    }
    *out_total = 0;
    if (out_counts)
        for (uint32_t s = 0; s < n_src; ++s) out_counts[s] = 0;

    HIPCHK(v->extract_ws.ensure(ws_bytes));
    char* ws = v->extract_ws.as<char>();
    uint64_t* d_totals = reinterpret_cast<uint64_t*>(ws);
    HIPCHK(gsx::op::MemsetAsync(d_totals, 0, sizeof(uint64_t) * n_src, v->stream));  // (an empty source runs no scan)
    const bool invert = (desc->flags & GSX_EXTRACT_INVERT) != 0;
    for (uint32_t s = 0; s < n_src; ++s) {  // the keep and scan passes of every source first
        const Region& r = src[s];
        const Model* m = r.m;
        if (m->n == 0) continue;
        ExtractFilter f{};
        if ((desc->filter & GSX_BOUNDS_MASKED) && m->has_mask) f.mask = m->mask.as<uint32_t>();
        if ((desc->filter & GSX_BOUNDS_SKIP_HIDDEN) && m->has_edits) {
            f.edited = m->edited.as<uint32_t>();
            f.edit_a = m->edit_a.as<float4>();
        }
        if (desc->filter & GSX_BOUNDS_SELECTED) {
            if (m->has_selection) f.selection = m->selection.as<uint32_t>();
            else f.select_none = 1u;
        }
        f.invert = invert ? 1u : 0u;
        uint32_t* partials = reinterpret_cast<uint32_t*>(ws + r.partials);
        HIPCHK(launch_extract_keep(v->stream, m->n, f, reinterpret_cast<uint32_t*>(ws + r.keep), partials));
        HIPCHK(launch_extract_scan(v->stream, partials, r.groups, reinterpret_cast<uint32_t*>(ws + r.bases), d_totals + s));
    }
    // the one wait of the call: dst is sized by the kept counts
    std::vector<uint64_t> counts(n_src);
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    HIPCHK(gsx::op::Memcpy(counts.data(), d_totals, sizeof(uint64_t) * n_src, hipMemcpyDeviceToHost));
    uint64_t total = 0;
    bool any_edits = false;
    for (uint32_t s = 0; s < n_src; ++s) {
        total += counts[s];
        any_edits = any_edits || src[s].m->has_edits;
    }
    if (total == 0) return GSX_OK;  // nothing kept anywhere: no model

    Model* d = nullptr;
    // (every plane of every Gaussian of dst is written below: no zero fill)
    if ((st = model_create(v, dst_key, total, sh_kind, cov_kind, false, &d))) return st;
    const bool edits = any_edits && !(desc->flags & GSX_EXTRACT_DROP_EDITS);
    if (edits && (st = ensure_edit_buffers(v, d)) == GSX_OK)  // (zeroes dst's `edited` plane: the joint words are ORed into)
        d->edit_epoch += 1;
    uint64_t off = 0;
    for (uint32_t s = 0; s < n_src && st == GSX_OK; ++s) {
        const Region& r = src[s];
        const Model* m = r.m;
        if (counts[s] == 0) continue;
        const bool carried = edits && m->has_edits;
        const uint32_t* keep = reinterpret_cast<const uint32_t*>(ws + r.keep);
        const uint32_t* bases = reinterpret_cast<const uint32_t*>(ws + r.bases);
        hipError_t e;
        if (r.identity) {
            // stored bits; a source without edit records leaves dst's `edited` bits clear, and its records are then never read
            e = launch_extract_scatter(v->stream, (int)sh_kind, (int)cov_kind, m->n, total, off, keep, bases, extract_planes(m, carried),
                                       extract_planes(d, carried));
            if (e == hipSuccess && edits && !carried) {
                e = gsx::op::MemsetAsync(d->edit_a.as<char>() + 16 * off, 0, 16 * counts[s], v->stream);
                if (e == hipSuccess) e = gsx::op::MemsetAsync(d->edit_b.as<char>() + 16 * off, 0, 16 * counts[s], v->stream);
            }
        } else {
            MergeBake b;
            quat_to_rows(m->mt.quat, b.R);
            for (int k = 0; k < 3; ++k) {
                b.s[k] = m->mt.scale[k];
                b.t[k] = m->mt.pos[k];
            }
            merge_sh_matrices(m->mt.quat, b.sh);
            e = launch_merge_bake(v->stream, (int)sh_kind, (int)cov_kind, m->n, total, off, keep, bases, extract_planes(m, carried), extract_planes(d, edits), b);
        }
        if (e != hipSuccess) st = fail(e == hipErrorOutOfMemory ? GSX_ERR_OOM : GSX_ERR_HIP, "gsx_model_merge: the copy of '%s' failed: %s", src_keys[s], hipGetErrorString(e));
        off += counts[s];
    }
    if (st) {  // no dst left behind
        (void)gsx::op::StreamSynchronize(v->stream);
        v->models.erase(dst_key);
        return st;
    }
    d->has_edits = edits;  // (identity transform, no mask, no selection, show_unedited off, no speculation windows: a new model)
    if (out_counts)
        for (uint32_t s = 0; s < n_src; ++s) out_counts[s] = counts[s];
    *out_total = total;
    return GSX_OK;
}

}  // extern "C"
