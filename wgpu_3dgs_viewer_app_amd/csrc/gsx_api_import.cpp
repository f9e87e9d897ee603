// gsx_api_import.cpp — C ABI of the PLY import (spec/RENDER_SPEC.md section 15; kernels_import.hip, import_math.h): binary vertex
// rows go from the caller's memory through the viewer's two row staging buffers straight into the resident pod planes.
#include "gsx_state.h"

#include <algorithm>

using namespace gsx;

namespace {
constexpr uint64_t kDefaultStagingBytes = 32ull << 20;  // one staging buffer when the desc says 0
constexpr uint64_t kMinStageRows = 1024;                // a staging buffer is raised to this many rows

gsx_status check_desc(const gsx_import_desc* desc, const char* who) {
    if (desc->flags) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", who, desc->flags);
    if (desc->reserved) return fail(GSX_ERR_INVALID_ARG, "%s: reserved is %u, not 0", who, desc->reserved);
    return GSX_OK;
}

// the header of the caller (or of gsx_ply_read_header) before a row is read
gsx_status check_header(const gsx_ply_header* h, const char* who) {
    int bad = -1;
    switch (im_check_header(*h, &bad)) {
        case 0: return GSX_OK;
        case 1:
            if (h->is_ascii) return fail(GSX_ERR_UNSUPPORTED, "%s: an ascii PLY is not decoded on the device (use gsx_ply_read_gaussians)", who);
            return fail(GSX_ERR_UNSUPPORTED, "%s: a vertex of %u bytes is more than %u (use gsx_ply_read_gaussians)", who, h->vertex_bytes, kImportMaxStride);
        default:
            if (h->vertex_bytes == 0) return fail(GSX_ERR_INVALID_ARG, "%s: the header's vertex_bytes is 0", who);
            if (h->offsets[bad] < 0) return fail(GSX_ERR_INVALID_ARG, "%s: the header lacks required property %d", who, bad);
            return fail(GSX_ERR_INVALID_ARG, "%s: offset %d of property %d is outside a vertex of %u bytes", who, h->offsets[bad], bad, h->vertex_bytes);
    }
}

// The chunk loop, export_rows' in the other direction: n > 0 rows of `h` at `rows` into the Gaussians [start, start + n) of m.  The
// copy of chunk c + 1 is issued on row_stream BEHIND the launch of chunk c's kernel on the viewer's stream: a copy out of pageable
// memory holds the calling thread, and the kernel runs beside it.  A copy into a buffer waits for the kernel that last read it
// (chunk c - 1's); a kernel waits for the copy that filled its buffer.  Returns when the caller's memory is no longer read and the
// kernels are complete (after an error too: nothing is in flight any more).
gsx_status import_rows(gsx_viewer* v, Model* m, uint64_t start, const char* rows, uint64_t n, const gsx_ply_header* h, const gsx_import_desc* desc,
                       const char* who) {
    const uint64_t vb = h->vertex_bytes;
    uint64_t stage_rows = (desc->staging_bytes ? desc->staging_bytes : kDefaultStagingBytes) / vb;
    stage_rows = std::min(std::max(stage_rows, kMinStageRows), n);  // (no chunk has more rows than the call)
    const uint64_t chunks = (n + stage_rows - 1) / stage_rows;
    gsx_status st = row_streams(v);
    if (st) return st;
    for (uint64_t b = 0; b < std::min<uint64_t>(chunks, 2); ++b) HIPCHK(v->row_stage[b].ensure((size_t)(stage_rows * vb)));
    const ImportLayout lay = im_layout(*h);
    const PodPlanes pod = m->pod();

    hipError_t e = hipSuccess;
    auto copy_chunk = [&](uint64_t c) {
        const int b = (int)(c & 1u);
        const uint64_t r0 = c * stage_rows, rn = std::min(stage_rows, n - r0);
        hipError_t r = c >= 2 ? gsx::op::StreamWaitEvent(v->row_stream, v->row_kernel_done[b], 0) : hipSuccess;
        if (r == hipSuccess) r = gsx::op::MemcpyAsync(v->row_stage[b].p, rows + r0 * vb, (size_t)(rn * vb), hipMemcpyHostToDevice, v->row_stream);
        if (r == hipSuccess) r = gsx::op::EventRecord(v->row_copy_done[b], v->row_stream);
        return r;
    };
    e = copy_chunk(0);
    for (uint64_t c = 0; c < chunks && e == hipSuccess; ++c) {
        const int b = (int)(c & 1u);
        const uint64_t r0 = c * stage_rows, rn = std::min(stage_rows, n - r0);
        e = gsx::op::StreamWaitEvent(v->stream, v->row_copy_done[b], 0);
        if (e == hipSuccess) e = launch_import_rows(v->stream, v->row_stage[b].p, rn, start + r0, m->n, pod, lay);
        if (e == hipSuccess) e = gsx::op::EventRecord(v->row_kernel_done[b], v->stream);
        if (e == hipSuccess && c + 1 < chunks) e = copy_chunk(c + 1);
    }
    gsx_status err = GSX_OK;
    if (e != hipSuccess) err = fail(e == hipErrorOutOfMemory ? GSX_ERR_OOM : GSX_ERR_HIP, "%s: a chunk failed: %s", who, hipGetErrorString(e));
    hipError_t e1 = gsx::op::StreamSynchronize(v->row_stream), e2 = gsx::op::StreamSynchronize(v->stream);
    if (err) return err;
    HIPCHK(e1);
    HIPCHK(e2);
    m->tuner.reset();
    drop_visibility(m);
    drop_normals(m);
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_import_desc_default(gsx_import_desc* d) {
    if (!d) return;
    *d = gsx_import_desc{0u, 0u, 0ull};
}

gsx_status gsx_model_upload_ply_rows(gsx_viewer* v, const char* key, uint64_t start, const void* rows, uint64_t n, const gsx_ply_header* header,
                                     const gsx_import_desc* desc) {
    const char* who = "gsx_model_upload_ply_rows";
    if (!v || !key || !header || !desc) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", who);
    gsx_status st = check_desc(desc, who);
    if (st) return st;
    if ((st = check_header(header, who))) return st;
    if ((st = viewer_bind(v))) return st;  // behind the frames in flight on the lanes
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "%s: no model '%s'", who, key);
    if (n == 0) return GSX_OK;
    if (!rows) return fail(GSX_ERR_INVALID_ARG, "%s: rows is null", who);
    if (start > m->n || n > m->n - start)
        return fail(GSX_ERR_INVALID_ARG, "%s: range [%llu,+%llu) exceeds model length %llu", who, (unsigned long long)start, (unsigned long long)n,
                    (unsigned long long)m->n);
    return import_rows(v, m, start, static_cast<const char*>(rows), n, header, desc, who);
}

gsx_status gsx_model_import_ply(gsx_viewer* v, const char* key, const void* data, uint64_t size, gsx_sh_kind sh, gsx_cov3d_kind cov3d,
                                const gsx_import_desc* desc, uint64_t* out_count) {
    const char* who = "gsx_model_import_ply";
    if (!v || !key || !data || !desc || !out_count) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", who);
    gsx_status st = check_desc(desc, who);
    if (st) return st;
    gsx_ply_header h;
    if ((st = gsx_ply_read_header(data, size, &h))) return st;  // GSX_ERR_PLY, the reader's message
    if ((st = check_header(&h, who))) return st == GSX_ERR_INVALID_ARG ? fail(GSX_ERR_PLY, "%s: the header is inconsistent", who) : st;
    if (h.count > (size - h.header_bytes) / h.vertex_bytes)
        return fail(GSX_ERR_IO, "%s: PLY data truncated: need %llu bytes, have %llu", who,
                    (unsigned long long)(h.header_bytes + h.count * (uint64_t)h.vertex_bytes), (unsigned long long)size);
    if ((st = viewer_bind(v))) return st;  // behind the frames in flight on the lanes; their next frames behind this call (epoch)
    if (v->models.count(key)) return fail(GSX_ERR_INVALID_ARG, "%s: model '%s' exists", who, key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "%s: the viewer has a communicator (import before gsx_viewer_comm_init, or on one GPU)", who);
    *out_count = 0;
    if (h.count == 0) return GSX_OK;  // nothing to load: no model
    Model* m = nullptr;
    // (every plane of every Gaussian is written below: no zero fill)
    if ((st = model_create(v, key, h.count, sh, cov3d, false, &m))) return st;
    st = import_rows(v, m, 0, static_cast<const char*>(data) + h.header_bytes, h.count, &h, desc, who);
    if (st) {  // no model left behind (import_rows has waited for both streams)
        v->models.erase(key);
        return st;
    }
    *out_count = h.count;
    return GSX_OK;
}

}  // extern "C"
