// gsx_api_merge.cpp — C ABI of the model merge (spec/RENDER_SPEC.md section 13; kernels_merge.hip, kernels_extract.hip).
#include "gsx_state.h"

using namespace gsx;

namespace gsx {
void quat_to_rows(const float q[4], float r[9]);  // kernels_project.hip: the float32 R_m of frame_consts_setup
}

extern "C" {

gsx_status gsx_model_merge(gsx_viewer* v, const char* const* src_keys, uint32_t n_src, const char* dst_key, const gsx_extract_desc* desc,
                           uint64_t* out_counts, uint64_t* out_total) {
    if (!v || !src_keys || !dst_key || !desc || !out_total) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: null argument");
    if (n_src == 0 || n_src > GSX_MERGE_MAX_SOURCES) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: n_src %u is not in [1, %u]", n_src, GSX_MERGE_MAX_SOURCES);
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: unknown filter bits 0x%x", desc->filter);
    if (desc->flags & ~(GSX_EXTRACT_INVERT | GSX_EXTRACT_DROP_EDITS)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: unknown flag bits 0x%x", desc->flags);
    for (uint32_t s = 0; s < n_src; ++s) {
        if (!src_keys[s]) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: src_keys[%u] is null", s);
        if (!strcmp(src_keys[s], dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: dst_key equals src_keys[%u] '%s'", s, dst_key);
    }
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    if (v->models.count(dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: model '%s' exists", dst_key);
    KeptSet src[GSX_MERGE_MAX_SOURCES];
    bool identity[GSX_MERGE_MAX_SOURCES];
    for (uint32_t s = 0; s < n_src; ++s)  // (a key may appear twice: the same model, instantiated twice)
        if (!(src[s].m = find_model(v, src_keys[s]))) return fail(GSX_ERR_NOT_FOUND, "gsx_model_merge: no model '%s'", src_keys[s]);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_merge: the viewer has a communicator (merge before gsx_viewer_comm_init, or on one GPU)");
    const gsx_sh_kind sh_kind = src[0].m->sh_kind;
    const gsx_cov3d_kind cov_kind = src[0].m->cov_kind;
    for (uint32_t s = 0; s < n_src; ++s) {
        const Model* m = src[s].m;
        if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_merge: model '%s' is a shard of a multi-GPU frame", src_keys[s]);
        if (m->sh_kind != sh_kind || m->cov_kind != cov_kind)
            return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: model '%s' is a Sh%d/Cov3d%d pod, '%s' a Sh%d/Cov3d%d pod (no conversion between kinds)",
                        src_keys[s], (int)m->sh_kind, (int)m->cov_kind, src_keys[0], (int)sh_kind, (int)cov_kind);
        if (!merge_is_valid(m->mt.pos, m->mt.quat, m->mt.scale))
            return fail(GSX_ERR_INVALID_ARG, "gsx_model_merge: the transform of model '%s' has a non-finite component or a zero quaternion", src_keys[s]);
        identity[s] = merge_is_identity(m->mt.pos, m->mt.quat, m->mt.scale);
    }
    *out_total = 0;
    if (out_counts)
        for (uint32_t s = 0; s < n_src; ++s) out_counts[s] = 0;

    if ((st = kept_sets(v, src, n_src, desc->filter, (desc->flags & GSX_EXTRACT_INVERT) != 0))) return st;
    uint64_t total = 0;
    bool any_edits = false;
    for (uint32_t s = 0; s < n_src; ++s) {
        total += src[s].total;
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
        const Model* m = src[s].m;
        const uint64_t count = src[s].total;
        if (count == 0) continue;
        const bool carried = edits && m->has_edits;
        const uint32_t *keep = src[s].d_keep, *bases = src[s].d_bases;
        hipError_t e;
        if (identity[s]) {
            // stored bits; a source without edit records leaves dst's `edited` bits clear, and its records are then never read
            e = launch_extract_scatter(v->stream, (int)sh_kind, (int)cov_kind, m->n, total, off, keep, bases, extract_planes(m, carried),
                                       extract_planes(d, carried));
            if (e == hipSuccess && edits && !carried) {
                e = gsx::op::MemsetAsync(d->edit_a.as<char>() + 16 * off, 0, 16 * count, v->stream);
                if (e == hipSuccess) e = gsx::op::MemsetAsync(d->edit_b.as<char>() + 16 * off, 0, 16 * count, v->stream);
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
        off += count;
    }
    if (st) {  // no dst left behind
        (void)gsx::op::StreamSynchronize(v->stream);
        v->models.erase(dst_key);
        return st;
    }
    d->has_edits = edits;  // (identity transform, no mask, no selection, show_unedited off, no speculation windows: a new model)
    if (out_counts)
        for (uint32_t s = 0; s < n_src; ++s) out_counts[s] = src[s].total;
    *out_total = total;
    return GSX_OK;
}

}  // extern "C"
