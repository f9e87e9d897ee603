// gsx_api_extract.cpp — C ABI of the model extract (spec/RENDER_SPEC.md section 12; kernels_extract.hip).
#include "gsx_state.h"

using namespace gsx;

namespace {
// the workspace: [total, padded to 128 B | keep words, padded to 128 B | partials | bases]
constexpr size_t kWsKeep = 128;

}  // namespace

extern "C" {

void gsx_extract_desc_default(gsx_extract_desc* d) {
    if (!d) return;
    *d = gsx_extract_desc{0u, 0u};
}

gsx_status gsx_model_extract(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_extract_desc* desc, uint64_t* out_count) {
    if (!v || !src_key || !dst_key || !desc || !out_count) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: null argument");
    if (desc->filter & ~(GSX_BOUNDS_MASKED | GSX_BOUNDS_SKIP_HIDDEN | GSX_BOUNDS_SELECTED))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: unknown filter bits 0x%x", desc->filter);
    if (desc->flags & ~(GSX_EXTRACT_INVERT | GSX_EXTRACT_DROP_EDITS)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: unknown flag bits 0x%x", desc->flags);
    if (!strcmp(src_key, dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: dst_key equals src_key '%s'", src_key);
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    if (v->models.count(dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: model '%s' exists", dst_key);
    Model* m = find_model(v, src_key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "gsx_model_extract: no model '%s'", src_key);
    // index sharding assumes every rank knows the global count
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_extract: the viewer has a communicator (extract before gsx_viewer_comm_init, or on one GPU)");
    if (m->shard_win_set || m->shard_limit_valid || m->shard_next_valid || m->shard_override_tiles)
        return fail(GSX_ERR_UNSUPPORTED, "gsx_model_extract: model '%s' is a shard of a multi-GPU frame", src_key);
    *out_count = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;

    const uint64_t groups = extract_groups(n);
    const size_t ws_partials = kWsKeep + extract_pad128(4 * (size_t)((n + 31) / 32)), ws_bases = ws_partials + extract_pad128(4 * (size_t)groups);
    HIPCHK(v->extract_ws.ensure(ws_bases + 4 * (size_t)groups));
    char* ws = v->extract_ws.as<char>();
    uint64_t* d_total = reinterpret_cast<uint64_t*>(ws);
    uint32_t* keep = reinterpret_cast<uint32_t*>(ws + kWsKeep);
    uint32_t* partials = reinterpret_cast<uint32_t*>(ws + ws_partials);
    uint32_t* bases = reinterpret_cast<uint32_t*>(ws + ws_bases);

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
    f.invert = (desc->flags & GSX_EXTRACT_INVERT) ? 1u : 0u;
    HIPCHK(launch_extract_keep(v->stream, n, f, keep, partials));
    HIPCHK(launch_extract_scan(v->stream, partials, groups, bases, d_total));
    // the one wait of the call: dst is sized by the kept count
    uint64_t count = 0;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    HIPCHK(gsx::op::Memcpy(&count, d_total, sizeof count, hipMemcpyDeviceToHost));
    if (count == 0) return GSX_OK;  // nothing kept: no model

    Model* d = nullptr;
    // (every plane of every Gaussian of dst is written below: no zero fill)
    if ((st = model_create(v, dst_key, count, m->sh_kind, m->cov_kind, false, &d))) return st;
    const bool edits = m->has_edits && !(desc->flags & GSX_EXTRACT_DROP_EDITS);
    hipError_t e = hipSuccess;
    if (edits && (st = ensure_edit_buffers(v, d)) == GSX_OK)  // (zeroes dst's `edited` plane)
        d->edit_epoch += 1;
    if (st == GSX_OK) {
        e = launch_extract_scatter(v->stream, (int)m->sh_kind, (int)m->cov_kind, n, count, 0, keep, bases, extract_planes(m, edits), extract_planes(d, edits));
        if (e != hipSuccess) st = fail(e == hipErrorOutOfMemory ? GSX_ERR_OOM : GSX_ERR_HIP, "gsx_model_extract: the scatter failed: %s", hipGetErrorString(e));
    }
    if (st) {  // no dst left behind
        (void)gsx::op::StreamSynchronize(v->stream);
        v->models.erase(dst_key);
        return st;
    }
    d->mt = m->mt;
    d->has_edits = edits;
    *out_count = count;
    return GSX_OK;
}

}  // extern "C"
