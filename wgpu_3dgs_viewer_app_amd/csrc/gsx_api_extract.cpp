// gsx_api_extract.cpp — C ABI of the model extract (spec/RENDER_SPEC.md section 12; kernels_extract.hip), and the kept-set pass
// that gsx_model_extract, gsx_model_merge and gsx_model_export share (kept_sets).
#include "gsx_state.h"

using namespace gsx;

namespace gsx {

gsx_status kept_sets(gsx_viewer* v, KeptSet* src, uint32_t n_src, uint32_t filter_bits, bool invert, std::vector<uint32_t>* host_bases) {
    uint64_t n[GSX_MERGE_MAX_SOURCES];
    ExtractRegion region[GSX_MERGE_MAX_SOURCES];
    bool any_empty = false;
    for (uint32_t s = 0; s < n_src; ++s) {
        n[s] = src[s].m->n;
        any_empty = any_empty || n[s] == 0;
    }
    HIPCHK(v->extract_ws.ensure(extract_ws_layout(n, n_src, region)));
    char* ws = v->extract_ws.as<char>();
    uint64_t* d_totals = reinterpret_cast<uint64_t*>(ws);
    if (any_empty) HIPCHK(gsx::op::MemsetAsync(d_totals, 0, sizeof(uint64_t) * n_src, v->stream));  // (an empty source runs no scan)
    for (uint32_t s = 0; s < n_src; ++s) {  // the keep and scan passes of every source first
        KeptSet& k = src[s];
        k.groups = extract_groups(n[s]);
        if (n[s] == 0) continue;
        uint32_t* keep = reinterpret_cast<uint32_t*>(ws + region[s].keep);
        uint32_t* partials = reinterpret_cast<uint32_t*>(ws + region[s].partials);
        uint32_t* bases = reinterpret_cast<uint32_t*>(ws + region[s].bases);
        HIPCHK(launch_extract_keep(v->stream, n[s], model_filter(k.m, filter_bits, invert), keep, partials));
        HIPCHK(launch_extract_scan(v->stream, partials, k.groups, bases, d_totals + s));
        k.d_keep = keep;
        k.d_bases = bases;
    }
    // the one wait of the call: what follows is sized by the kept counts
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    if (host_bases) {  // (one source: its total and its bases lie side by side, one copy)
        std::vector<uint32_t> host(region[0].bases / 4 + src[0].groups);
        HIPCHK(gsx::op::Memcpy(host.data(), ws, 4 * host.size(), hipMemcpyDeviceToHost));
        memcpy(&src[0].total, host.data(), sizeof src[0].total);
        host_bases->assign(host.begin() + region[0].bases / 4, host.end());
        host_bases->push_back((uint32_t)src[0].total);
        return GSX_OK;
    }
    uint64_t totals[GSX_MERGE_MAX_SOURCES];
    HIPCHK(gsx::op::Memcpy(totals, d_totals, sizeof(uint64_t) * n_src, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < n_src; ++s) src[s].total = totals[s];
    return GSX_OK;
}

}  // namespace gsx

extern "C" {

void gsx_extract_desc_default(gsx_extract_desc* d) {
    if (!d) return;
    *d = gsx_extract_desc{0u, 0u};
}

gsx_status gsx_model_extract(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_extract_desc* desc, uint64_t* out_count) {
    if (!v || !src_key || !dst_key || !desc || !out_count) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: null argument");
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: unknown filter bits 0x%x", desc->filter);
    if (desc->flags & ~(GSX_EXTRACT_INVERT | GSX_EXTRACT_DROP_EDITS)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: unknown flag bits 0x%x", desc->flags);
    if (!strcmp(src_key, dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: dst_key equals src_key '%s'", src_key);
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    if (v->models.count(dst_key)) return fail(GSX_ERR_INVALID_ARG, "gsx_model_extract: model '%s' exists", dst_key);
    Model* m = find_model(v, src_key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "gsx_model_extract: no model '%s'", src_key);
    // index sharding assumes every rank knows the global count
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_extract: the viewer has a communicator (extract before gsx_viewer_comm_init, or on one GPU)");
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "gsx_model_extract: model '%s' is a shard of a multi-GPU frame", src_key);
    *out_count = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;

    KeptSet kept;
    kept.m = m;
    if ((st = kept_sets(v, &kept, 1, desc->filter, (desc->flags & GSX_EXTRACT_INVERT) != 0))) return st;
    const uint64_t count = kept.total;
    if (count == 0) return GSX_OK;  // nothing kept: no model

    Model* d = nullptr;
    // (every plane of every Gaussian of dst is written below: no zero fill)
    if ((st = model_create(v, dst_key, count, m->sh_kind, m->cov_kind, false, &d))) return st;
    const bool edits = m->has_edits && !(desc->flags & GSX_EXTRACT_DROP_EDITS);
    hipError_t e = hipSuccess;
    if (edits && (st = ensure_edit_buffers(v, d)) == GSX_OK)  // (zeroes dst's `edited` plane)
        d->edit_epoch += 1;
    if (st == GSX_OK) {
        e = launch_extract_scatter(v->stream, (int)m->sh_kind, (int)m->cov_kind, n, count, 0, kept.d_keep, kept.d_bases, extract_planes(m, edits), extract_planes(d, edits));
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
