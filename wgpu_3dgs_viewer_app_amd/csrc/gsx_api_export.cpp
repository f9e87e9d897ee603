// gsx_api_export.cpp — C ABI of the model export (spec/RENDER_SPEC.md section 14; kernels_export.hip, kernels_extract.hip).
#include "gsx_state.h"

#include <string>
#include <vector>

using namespace gsx;

namespace gsx {
std::string ply_header(uint64_t count);  // gsx_ply.cpp: the one header writer
}

gsx_status gsx::row_streams(gsx_viewer* v) {
    if (v->row_stream) return GSX_OK;
    HIPCHK(hipStreamCreateWithFlags(&v->row_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
        HIPCHK(hipEventCreateWithFlags(&v->row_kernel_done[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&v->row_copy_done[b], hipEventDisableTiming));
    }
    return GSX_OK;
}

namespace {
constexpr uint64_t kDefaultStagingBytes = 32ull << 20;  // one staging buffer when the desc says 0

constexpr uint64_t row_bytes(uint32_t format) { return format == GSX_EXPORT_GAUSSIANS ? sizeof(gsx_gaussian) : 248u; }

// what the keep and scan passes of one call leave behind
struct Kept : KeptSet {
    std::vector<uint32_t> bases;  // host copy, groups + 1 entries (the last: the total); only with `want_bases`
};

// validation, viewer_bind, then the kept set (kept_sets: the keep and scan passes, the one wait before the rows: the kept count
// sizes the output, the bases cut the source into chunks)
gsx_status export_keep(gsx_viewer* v, const char* key, const gsx_export_desc* desc, const char* who, bool check_format, bool want_bases, Kept* k) {
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", who, desc->filter);
    if (desc->flags & ~(GSX_EXTRACT_INVERT | GSX_EXPORT_BAKE_EDITS)) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", who, desc->flags);
    if (check_format && desc->format != GSX_EXPORT_GAUSSIANS && desc->format != GSX_EXPORT_PLY_VERTICES) return fail(GSX_ERR_INVALID_ARG, "%s: unknown format %u", who, desc->format);
    if (desc->reserved) return fail(GSX_ERR_INVALID_ARG, "%s: reserved is %u, not 0", who, desc->reserved);
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (st) return st;
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "%s: no model '%s'", who, key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "%s: the viewer has a communicator (export before gsx_viewer_comm_init, or on one GPU)", who);
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "%s: model '%s' is a shard of a multi-GPU frame", who, key);
    k->m = m;
    if (m->n == 0) return GSX_OK;
    return kept_sets(v, k, 1, desc->filter, (desc->flags & GSX_EXTRACT_INVERT) != 0, want_bases ? &k->bases : nullptr);
}

// the chunk loop: k->total rows of `format` into out (k->total > 0, out holds them)
gsx_status export_rows(gsx_viewer* v, const gsx_export_desc* desc, uint32_t format, const Kept& k, char* out) {
    const Model* m = k.m;
    const uint64_t rb = row_bytes(format);
    // a staging buffer holds whole workgroups' rows: at least one workgroup's worth
    uint64_t stage_rows = (desc->staging_bytes ? desc->staging_bytes : kDefaultStagingBytes) / rb;
    if (stage_rows < kExtractGroup) stage_rows = kExtractGroup;
    if (stage_rows > k.total) stage_rows = k.total;  // (no chunk has more rows than the call)
    gsx_status st = row_streams(v);
    if (st) return st;
    for (int b = 0; b < 2; ++b) HIPCHK(v->row_stage[b].ensure((size_t)(stage_rows * rb)));
    const bool bake = (desc->flags & GSX_EXPORT_BAKE_EDITS) && m->has_edits;
    const ExtractPlanes src = extract_planes(m, bake);

    // chunk c: the workgroups [g0, g1) with at most stage_rows kept Gaussians, as many as fit (a workgroup keeps at most 1024)
    struct Chunk {
        uint64_t g0, g1;
    };
    std::vector<Chunk> chunks;
    for (uint64_t g0 = 0; g0 < k.groups;) {
        if (k.bases[g0 + 1] == k.bases[g0]) {  // (workgroups that keep nothing start no chunk)
            ++g0;
            continue;
        }
        uint64_t g1 = g0 + 1;
        while (g1 < k.groups && (uint64_t)k.bases[g1 + 1] - k.bases[g0] <= stage_rows) ++g1;
        chunks.push_back({g0, g1});
        g0 = g1;
    }
    // The kernel of chunk c + 1 is enqueued BEFORE the copy of chunk c: a copy into pageable memory holds the calling thread, and
    // the kernel runs beside it.  A kernel waits for the copy that last read its buffer (chunk c - 1's, enqueued an iteration ago).
    hipError_t e = hipSuccess;
    auto rows_kernel = [&](size_t c) {
        const int b = (int)(c & 1u);
        const Chunk& ch = chunks[c];
        hipError_t r = c >= 2 ? gsx::op::StreamWaitEvent(v->stream, v->row_copy_done[b], 0) : hipSuccess;
        if (r == hipSuccess)
            r = launch_export_rows(v->stream, (int)m->sh_kind, (int)m->cov_kind, format, m->n, (uint32_t)ch.g0, (uint32_t)(ch.g1 - ch.g0), k.bases[ch.g0], k.d_keep,
                                   k.d_bases, src, v->row_stage[b].p);
        if (r == hipSuccess) r = gsx::op::EventRecord(v->row_kernel_done[b], v->stream);
        return r;
    };
    if (!chunks.empty()) e = rows_kernel(0);
    for (size_t c = 0; c < chunks.size() && e == hipSuccess; ++c) {
        const int b = (int)(c & 1u);
        const Chunk& ch = chunks[c];
        if (c + 1 < chunks.size()) e = rows_kernel(c + 1);
        const uint64_t rows = (uint64_t)k.bases[ch.g1] - k.bases[ch.g0];
        if (e == hipSuccess) e = gsx::op::StreamWaitEvent(v->row_stream, v->row_kernel_done[b], 0);
        if (e == hipSuccess) e = gsx::op::MemcpyAsync(out + (uint64_t)k.bases[ch.g0] * rb, v->row_stage[b].p, (size_t)(rows * rb), hipMemcpyDeviceToHost, v->row_stream);
        if (e == hipSuccess) e = gsx::op::EventRecord(v->row_copy_done[b], v->row_stream);
    }
    gsx_status err = GSX_OK;
    if (e != hipSuccess) err = fail(e == hipErrorOutOfMemory ? GSX_ERR_OOM : GSX_ERR_HIP, "gsx_model_export: a chunk failed: %s", hipGetErrorString(e));
    // the call returns when `out` is complete (and, after an error, when nothing of it is in flight any more)
    hipError_t e1 = gsx::op::StreamSynchronize(v->row_stream), e2 = gsx::op::StreamSynchronize(v->stream);
    if (err) return err;
    HIPCHK(e1);
    HIPCHK(e2);
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_export_desc_default(gsx_export_desc* d) {
    if (!d) return;
    *d = gsx_export_desc{0u, 0u, GSX_EXPORT_GAUSSIANS, 0u, 0ull};
}

gsx_status gsx_model_export(gsx_viewer* v, const char* key, const gsx_export_desc* desc, void* out, uint64_t capacity_bytes, uint64_t* out_count) {
    if (!v || !key || !desc || !out_count) return fail(GSX_ERR_INVALID_ARG, "gsx_model_export: null argument");
    Kept k;
    gsx_status st = export_keep(v, key, desc, "gsx_model_export", true, out != nullptr, &k);
    if (st) return st;
    *out_count = k.total;
    if (!out || k.total == 0) return GSX_OK;  // the count alone; or nothing kept: nothing written
    const uint64_t rb = row_bytes(desc->format);
    if (capacity_bytes / rb < k.total)
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_export: buffer too small (%llu bytes < %llu rows of %llu bytes)", (unsigned long long)capacity_bytes,
                    (unsigned long long)k.total, (unsigned long long)rb);
    return export_rows(v, desc, desc->format, k, static_cast<char*>(out));
}

gsx_status gsx_model_export_ply(gsx_viewer* v, const char* key, const gsx_export_desc* desc, void* out, uint64_t capacity, uint64_t* out_size) {
    if (!v || !key || !desc || !out_size) return fail(GSX_ERR_INVALID_ARG, "gsx_model_export_ply: null argument");
    Kept k;
    gsx_status st = export_keep(v, key, desc, "gsx_model_export_ply", false, out != nullptr, &k);  // (desc->format is ignored: the rows are PLY rows)
    if (st) return st;
    std::string header;
    try {  // (nothing may leave an extern "C" function by exception)
        header = ply_header(k.total);
    } catch (...) {
        return fail(GSX_ERR_OOM, "gsx_model_export_ply: no memory for the header");
    }
    *out_size = header.size() + k.total * 248ull;
    if (!out) return GSX_OK;
    if (capacity < *out_size)
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_export_ply: buffer too small (%llu < %llu)", (unsigned long long)capacity, (unsigned long long)*out_size);
    memcpy(out, header.data(), header.size());
    if (k.total == 0) return GSX_OK;
    return export_rows(v, desc, GSX_EXPORT_PLY_VERTICES, k, static_cast<char*>(out) + header.size());
}

}  // extern "C"
