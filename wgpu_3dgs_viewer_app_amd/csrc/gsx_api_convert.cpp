// gsx_api_convert.cpp — C ABI of the model convert (spec/RENDER_SPEC.md section 16; kernels_convert.hip): gsx_model_pod_kind,
// gsx_model_convert (gsx_model_extract into a model of another pod kind) and gsx_model_set_pod_kind (the same under the model's own
// key, keeping its mask, selection and edit buffers).  The kept-set pass, the model creation and the planes are gsx_model_extract's
// (kept_sets, model_create, ensure_edit_buffers, extract_planes).
#include "gsx_state.h"

using namespace gsx;

namespace {

bool kind_in_range(uint32_t sh, uint32_t cov3d) { return sh <= (uint32_t)GSX_SH_NONE && cov3d <= (uint32_t)GSX_COV3D_HALF; }

// The kept Gaussians of `m` under (filter, flags) as the new model `dst_key` of kind (sh, cov3d): gsx_model_extract's body with the
// kind of dst free.  The same kind takes launch_extract_scatter, every other launch_convert_kind.  Nothing kept: GSX_OK, *out null.
// A failure leaves no dst behind.  `fn` names the entry point in messages.
gsx_status convert_into(gsx_viewer* v, const char* fn, const Model* m, const char* dst_key, uint32_t filter, uint32_t flags, gsx_sh_kind sh,
                        gsx_cov3d_kind cov3d, Model** out, uint64_t* out_count) {
    *out = nullptr;
    *out_count = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    gsx_status st = GSX_OK;
    KeptSet kept;
    kept.m = m;
    if ((st = kept_sets(v, &kept, 1, filter, (flags & GSX_EXTRACT_INVERT) != 0))) return st;
    const uint64_t count = kept.total;
    if (count == 0) return GSX_OK;  // nothing kept: no model

    Model* d = nullptr;
    // (every plane of every Gaussian of dst is written below: no zero fill)
    if ((st = model_create(v, dst_key, count, sh, cov3d, false, &d))) return st;
    const bool edits = m->has_edits && !(flags & GSX_EXTRACT_DROP_EDITS);
    if (edits && (st = ensure_edit_buffers(v, d)) == GSX_OK)  // (zeroes dst's `edited` plane)
        d->edit_epoch += 1;
    if (st == GSX_OK) {
        const ExtractPlanes sp = extract_planes(m, edits), dp = extract_planes(d, edits);
        hipError_t e;
        if (sh == m->sh_kind && cov3d == m->cov_kind)
            e = launch_extract_scatter(v->stream, (int)sh, (int)cov3d, n, count, 0, kept.d_keep, kept.d_bases, sp, dp);
        else
            e = launch_convert_kind(v->stream, (int)m->sh_kind, (int)m->cov_kind, (int)sh, (int)cov3d, n, count, 0, kept.d_keep, kept.d_bases, sp, dp);
        if (e != hipSuccess) st = fail(e == hipErrorOutOfMemory ? GSX_ERR_OOM : GSX_ERR_HIP, "%s: the kernel launch failed: %s", fn, hipGetErrorString(e));
    }
    if (st) {  // no dst left behind
        (void)gsx::op::StreamSynchronize(v->stream);
        v->models.erase(dst_key);
        return st;
    }
    d->mt = m->mt;
    d->has_edits = edits;
    *out = d;
    *out_count = count;
    return GSX_OK;
}

// dst takes src's allocation; src is left empty (owned buffers only: a model of the viewer itself, never a lane's view)
void move_buf(DevBuf& dst, DevBuf& src) {
    dst.release();
    dst.p = src.p;
    dst.bytes = src.bytes;
    dst.borrowed = src.borrowed;
    src.p = nullptr;
    src.bytes = 0;
    src.borrowed = false;
}

}  // namespace

extern "C" {

void gsx_convert_desc_default(gsx_convert_desc* d) {
    if (!d) return;
    *d = gsx_convert_desc{0u, 0u, 0u, 0u};
}

gsx_status gsx_model_pod_kind(gsx_viewer* v, const char* key, gsx_sh_kind* out_sh, gsx_cov3d_kind* out_cov3d) {
    if (!v || !key || !out_sh || !out_cov3d) return fail(GSX_ERR_INVALID_ARG, "gsx_model_pod_kind: null argument");
    const Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "gsx_model_pod_kind: no model '%s'", key);
    *out_sh = m->sh_kind;
    *out_cov3d = m->cov_kind;
    return GSX_OK;
}

gsx_status gsx_model_convert(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_convert_desc* desc, uint64_t* out_count) {
    if (!v || !src_key || !dst_key || !desc || !out_count) return fail(GSX_ERR_INVALID_ARG, "gsx_model_convert: null argument");
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "gsx_model_convert: unknown filter bits 0x%x", desc->filter);
    if (desc->flags & ~(GSX_EXTRACT_INVERT | GSX_EXTRACT_DROP_EDITS)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_convert: unknown flag bits 0x%x", desc->flags);
    if (!kind_in_range(desc->sh, desc->cov3d)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_convert: unknown pod kind Sh%u/Cov3d%u", desc->sh, desc->cov3d);
    if (!strcmp(src_key, dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_convert: dst_key equals src_key '%s'", src_key);
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    if (v->models.count(dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_convert: model '%s' exists", dst_key);
    Model* m = find_model(v, src_key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "gsx_model_convert: no model '%s'", src_key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_convert: the viewer has a communicator (convert before gsx_viewer_comm_init, or on one GPU)");
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_convert: model '%s' is a shard of a multi-GPU frame", src_key);
    Model* d = nullptr;
    return convert_into(v, "gsx_model_convert", m, dst_key, desc->filter, desc->flags, (gsx_sh_kind)desc->sh, (gsx_cov3d_kind)desc->cov3d, &d, out_count);
}

gsx_status gsx_model_set_pod_kind(gsx_viewer* v, const char* key, gsx_sh_kind sh, gsx_cov3d_kind cov3d) {
    if (!v || !key) return fail(GSX_ERR_INVALID_ARG, "gsx_model_set_pod_kind: null argument");
    if ((int)sh < 0 || (int)cov3d < 0 || !kind_in_range((uint32_t)sh, (uint32_t)cov3d))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_set_pod_kind: unknown pod kind Sh%d/Cov3d%d", (int)sh, (int)cov3d);
    gsx_status st = viewer_bind(v);
    if (st) return st;
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "gsx_model_set_pod_kind: no model '%s'", key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_set_pod_kind: the viewer has a communicator (convert before gsx_viewer_comm_init, or on one GPU)");
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_set_pod_kind: model '%s' is a shard of a multi-GPU frame", key);
    if (sh == m->sh_kind && cov3d == m->cov_kind) return GSX_OK;  // nothing changes: the serial and the speculation state stay

    // The new planes are built beside the old ones, as a model of their own under a key no caller can name; a failure (GSX_ERR_OOM
    // among them) leaves that model out and `m` as it was.  The edit records are not carried by the kernel: the buffers move below.
    const std::string tmp = std::string(key) + "\x01gsx_model_set_pod_kind";
    if (v->models.count(tmp)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_set_pod_kind: model '%s' is being converted", key);
    Model* d = nullptr;
    uint64_t count = 0;
    if (m->n == 0) {
        if ((st = model_create(v, tmp.c_str(), 0, sh, cov3d, true, &d))) return st;
    } else {
        if ((st = convert_into(v, "gsx_model_set_pod_kind", m, tmp.c_str(), 0u, GSX_EXTRACT_DROP_EDITS, sh, cov3d, &d, &count))) return st;
        if (!d || count != m->n) {  // (filter 0 keeps every Gaussian)
            if (d) {
                (void)gsx::op::StreamSynchronize(v->stream);
                v->models.erase(tmp);
            }
            return fail(GSX_ERR_HIP, "gsx_model_set_pod_kind: kept %llu of %llu Gaussians", (unsigned long long)count, (unsigned long long)m->n);
        }
    }
    // the kernel has read the old planes, and the lanes' frames that read them are complete (viewer_bind ordered this stream behind them)
    hipError_t e = gsx::op::StreamSynchronize(v->stream);
    if (e != hipSuccess) {
        v->models.erase(tmp);
        return fail(GSX_ERR_HIP, "gsx_model_set_pod_kind: hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    std::unique_ptr<Model> nm = std::move(v->models[tmp]);
    v->models.erase(tmp);
    // what the model keeps: moved, neither copied nor derived again
    nm->key = key;
    nm->mt = m->mt;
    move_buf(nm->mask, m->mask);
    nm->has_mask = m->has_mask;
    nm->mask_program_hash = m->mask_program_hash;
    move_buf(nm->selection, m->selection);
    nm->has_selection = m->has_selection;
    move_buf(nm->edited, m->edited);
    move_buf(nm->edit_a, m->edit_a);
    move_buf(nm->edit_b, m->edit_b);
    move_buf(nm->keep, m->keep);  // (allocated with the edit planes, ensure_edit_buffers; its contents are derived per frame)
    nm->has_edits = m->has_edits;
    nm->show_unedited = m->show_unedited;
    nm->edit_epoch = m->edit_epoch + 1;  // (k_edit_prepare runs again for the new model: prep_epoch is 0)
    // Everything a frame caches starts again: the new Model has no speculation windows, a fresh tuner and a NEW serial, by which the
    // lanes' shadow models notice (lane_sync).  Their shadows of the old model borrow its planes and its tuner: dropped here, as
    // gsx_model_remove drops them.
    for (gsx_viewer* l : v->lanes) l->models.erase(key);
    v->models[key] = std::move(nm);  // (frees the old planes)
    return GSX_OK;
}

}  // extern "C"
