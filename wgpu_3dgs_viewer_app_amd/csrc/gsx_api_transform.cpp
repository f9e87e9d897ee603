// gsx_api_transform.cpp — C ABI of the model transform (spec/RENDER_SPEC.md section 21; kernels_transform.hip):
// gsx_model_apply_transform moves the kept Gaussians of a resident model where they lie.  The kept set is gsx_model_extract's
// (kept_sets: the keep words and the count, the call's one wait); the rules of the transform are csrc/transform_math.h's.
#include "gsx_state.h"
#include "transform_math.h"

using namespace gsx;

extern "C" {

void gsx_transform_desc_default(gsx_transform_desc* d) {
    if (!d) return;
    *d = gsx_transform_desc{0u, 0u, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 1.0f}, {1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f}, 0u};
}

gsx_status gsx_model_apply_transform(gsx_viewer* v, const char* key, const gsx_transform_desc* desc, uint64_t* out_count) {
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "gsx_model_apply_transform: null argument");
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "gsx_model_apply_transform: unknown filter bits 0x%x", desc->filter);
    if (desc->flags & ~GSX_EXTRACT_INVERT) return fail(GSX_ERR_INVALID_ARG, "gsx_model_apply_transform: unknown flag bits 0x%x", desc->flags);
    if (desc->reserved != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_apply_transform: reserved is 0x%x, not 0", desc->reserved);
    if (!transform_is_valid(desc->pos, desc->quat, desc->scale, desc->pivot))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_apply_transform: the transform has a non-finite component or a zero quaternion");
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "gsx_model_apply_transform: no model '%s'", key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_apply_transform: the viewer has a communicator (transform before gsx_viewer_comm_init, or on one GPU)");
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_apply_transform: model '%s' is a shard of a multi-GPU frame", key);
    if (out_count) *out_count = 0;
    if (m->n == 0) return GSX_OK;

    // the workspace grows here, before anything of the model changes: a GSX_ERR_OOM leaves the model as it was
    KeptSet kept;
    kept.m = m;
    if ((st = kept_sets(v, &kept, 1, desc->filter, (desc->flags & GSX_EXTRACT_INVERT) != 0))) return st;
    if (out_count) *out_count = kept.total;
    if (kept.total == 0) return GSX_OK;  // nothing kept: nothing is written, nothing is reset
    const int mode = transform_mode(desc->pos, desc->quat, desc->scale);
    if (mode == kTransformIdentity) return GSX_OK;  // whatever the pivot: nothing is written, nothing is reset

    TransformBake tb{};
    quat_to_rows(desc->quat, tb.b.R);  // the quaternion as given, as frame_consts_setup and gsx_model_merge take a model transform's
    for (int k = 0; k < 3; ++k) {
        tb.b.s[k] = desc->scale[k];
        tb.b.t[k] = desc->pos[k];
        tb.c[k] = desc->pivot[k];
    }
    tb.use_pivot = transform_pivot_is_zero(desc->pivot) ? 0u : 1u;
    if (mode == kTransformFull) merge_sh_matrices(desc->quat, tb.b.sh);
    const hipError_t e = launch_transform_inplace(v->stream, (int)m->sh_kind, (int)m->cov_kind, mode, m->n, kept.d_keep, extract_planes(m, false), tb);
    if (e != hipSuccess) return fail(GSX_ERR_HIP, "gsx_model_apply_transform: the kernel launch failed: %s", hipGetErrorString(e));
    // What a frame caches from the planes.  The tuner's timings belong to the scene as it was (as after the in-place uploads); the
    // mask was evaluated over the old positions, so the same program is no longer "the same mask" (gsx_mask_evaluate keeps the
    // tuner's state while the hash stands).  Nothing else is keyed on the planes: the speculation windows are guesses that every
    // frame verifies, prep_epoch follows the mask, selection and edit buffers alone, and the lanes' shadow models borrow these
    // planes and this tuner and copy the hash at their next frame (lane_sync).
    m->tuner.reset();
    m->mask_program_hash = 0;
    drop_visibility(m);  // (the planes were measured on the old pod planes; hipFree waits for the kernel above)
    drop_normals(m);
    return GSX_OK;
}

}  // extern "C"
