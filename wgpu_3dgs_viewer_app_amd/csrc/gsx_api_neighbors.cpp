// gsx_api_neighbors.cpp — C ABI of the neighbour counts (spec/RENDER_SPEC.md section 18; kernels_neighbors.hip):
// gsx_model_neighbors and gsx_model_select_neighbors.  The filter is model_filter's, the workspace the model operations'
// (v->extract_ws): [result block, 128 B | 4096 histogram words | the scan's total | the workgroups' partials | the participant bits |
// the bucket table | the scan's block sums and bases | the counts, 4 B a Gaussian | the records, 16 B a Gaussian].
#include "gsx_state.h"
#include "neighbors_math.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_neighbor_desc) == 24 && sizeof(gsx_neighbor_stats_t) == 24 && sizeof(gsx_neighbor_select_desc) == 40, "spec section 18's layouts");
static_assert(GSX_NEIGHBOR_MAX_COUNT == kNbMaxCount, "neighbors_math.h restates the cap");

constexpr size_t kWsHist = 4 * kNbResultWords;                 // 128
constexpr size_t kWsTotal = kWsHist + 4 * (kNbMaxCount + 1u);  // 16 512
constexpr size_t kWsPartials = kWsTotal + 128;
static_assert(kWsHist == 128 && kWsPartials % 128 == 0, "the workspace regions are whole 128-byte lines");

// The workspace of a model of n Gaussians under a table of 2^bits buckets; returns its bytes.
size_t neighbor_ws(char* ws, uint64_t n, uint32_t bits, NeighborJob* job) {
    const size_t words = size_t(1) << bits, blocks = (words + kNbScanBlock - 1u) / kNbScanBlock;
    size_t at = kWsPartials;
    const auto take = [&](size_t bytes) {  // the next region: whole 128-byte lines
        const size_t here = at;
        at += extract_pad128(bytes);
        return reinterpret_cast<uintptr_t>(ws) + here;
    };
    const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
    job->result = reinterpret_cast<uint32_t*>(base);
    job->hist = reinterpret_cast<uint32_t*>(base + kWsHist);
    job->scan_total = reinterpret_cast<uint64_t*>(base + kWsTotal);
    job->partials = reinterpret_cast<uint32_t*>(take(4 * kNbPartialWords * (size_t)extract_groups(n)));
    job->participants = reinterpret_cast<uint32_t*>(take(4 * (size_t)((n + 31u) / 32u)));
    job->table = reinterpret_cast<uint32_t*>(take(4 * words));
    job->scan_sums = reinterpret_cast<uint32_t*>(take(4 * blocks));
    job->scan_bases = reinterpret_cast<uint32_t*>(take(4 * blocks));
    job->counts = reinterpret_cast<uint32_t*>(take(4 * (size_t)n));
    job->records = reinterpret_cast<uint4*>(take(16 * (size_t)n));
    return at;
}

// what both calls check about (filter, flags, radius, max_count, grid_bits)
gsx_status check_desc(const char* fn, uint32_t filter, uint32_t flags, float radius, uint32_t max_count, uint32_t grid_bits) {
    if (filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, filter);
    if (flags) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (none are defined)", fn, flags);
    if (!nb_radius_ok(radius)) return fail(GSX_ERR_INVALID_ARG, "%s: the radius %g is not finite and above 0, or its float32 square is 0 or inf", fn, (double)radius);
    if (max_count < 1u || max_count > kNbMaxCount) return fail(GSX_ERR_INVALID_ARG, "%s: max_count %u is not in 1 .. %u", fn, max_count, kNbMaxCount);
    if (grid_bits > kNbMaxBits) return fail(GSX_ERR_INVALID_ARG, "%s: grid_bits %u is above %u", fn, grid_bits, kNbMaxBits);
    return GSX_OK;
}

// bind, find, refuse what gsx_model_extract refuses
gsx_status neighbor_model(gsx_viewer* v, const char* fn, const char* key, Model** out) {
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes
    if (st) return st;
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "%s: no model '%s'", fn, key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "%s: the viewer has a communicator (call it before gsx_viewer_comm_init, or on one GPU)", fn);
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "%s: model '%s' is a shard of a multi-GPU frame", fn, key);
    *out = m;
    return GSX_OK;
}

// The workspace (grown if need be: the only step that can fail for memory) and the job of a call; n > 0.
gsx_status neighbor_job(gsx_viewer* v, const Model* m, float radius, uint32_t max_count, uint32_t grid_bits, NeighborJob* job) {
    const uint32_t bits = grid_bits ? grid_bits : nb_auto_bits(m->n);
    NeighborJob sized{};
    HIPCHK(v->extract_ws.ensure(neighbor_ws(nullptr, m->n, bits, &sized)));
    *job = NeighborJob{};
    neighbor_ws(v->extract_ws.as<char>(), m->n, bits, job);
    const NbGrid g = nb_grid(radius);
    job->r2 = g.r2;
    job->inv_h = g.inv_h;
    job->bits = bits;
    job->max_count = max_count;
    return GSX_OK;
}

// Every pass up to the query, enqueued: the counts and the histogram are in the workspace when the stream reaches its end.
gsx_status enqueue_counts(gsx_viewer* v, const Model* m, const ModelFilter& f, const NeighborJob& job) {
    const uint4* pc = extract_planes(m, false).pc;
    HIPCHK(gsx::op::MemsetAsync(job.result, 0, kWsTotal + 8, v->stream));  // the result block, the bins, the scan's total
    HIPCHK(gsx::op::MemsetAsync(job.table, 0, 4 * (size_t(1) << job.bits), v->stream));
    HIPCHK(launch_neighbors_reduce(v->stream, m->n, f, pc, job));
    HIPCHK(launch_neighbors_cell(v->stream, m->n, f, pc, job));
    HIPCHK(launch_neighbors_scan(v->stream, job));
    HIPCHK(launch_neighbors_scatter(v->stream, m->n, pc, job));
    HIPCHK(launch_neighbors_query(v->stream, m->n, job));
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_neighbor_desc_default(gsx_neighbor_desc* d) {
    if (!d) return;
    *d = gsx_neighbor_desc{};
    d->radius = 1.0f;
    d->max_count = GSX_NEIGHBOR_MAX_COUNT;
}

gsx_status gsx_model_neighbors(gsx_viewer* v, const char* key, const gsx_neighbor_desc* desc, uint32_t* out_counts, uint64_t* out_hist, gsx_neighbor_stats_t* out) {
    if (!v || !key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_neighbors: null argument");
    gsx_status st = check_desc("gsx_model_neighbors", desc->filter, desc->flags, desc->radius, desc->max_count, desc->grid_bits);
    if (st) return st;
    if (desc->reserved != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_neighbors: reserved is %u, not 0", desc->reserved);
    Model* m = nullptr;
    if ((st = neighbor_model(v, "gsx_model_neighbors", key, &m))) return st;
    *out = gsx_neighbor_stats_t{};
    out->grid_bits = desc->grid_bits ? desc->grid_bits : nb_auto_bits(m->n);
    if (out_hist)
        for (uint32_t c = 0; c <= desc->max_count; ++c) out_hist[c] = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    NeighborJob job;
    if ((st = neighbor_job(v, m, desc->radius, desc->max_count, desc->grid_bits, &job))) return st;
    if ((st = enqueue_counts(v, m, model_filter(m, desc->filter, false), job))) return st;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    std::vector<uint32_t> host(kNbResultWords + (out_hist ? desc->max_count + 1u : 0u));  // the result block and the bins: one copy
    HIPCHK(gsx::op::Memcpy(host.data(), job.result, 4 * host.size(), hipMemcpyDeviceToHost));
    out->count = host[kNbCount];
    out->n_nonfinite = host[kNbNonfinite];
    if (out_hist)
        for (uint32_t c = 0; c <= desc->max_count; ++c) out_hist[c] = host[kNbResultWords + c];  // (32-bit on the device: n < 2^32)
    if (out_counts) HIPCHK(gsx::op::Memcpy(out_counts, job.counts, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_model_select_neighbors(gsx_viewer* v, const char* key, const gsx_neighbor_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected) {
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_neighbors: null argument");
    gsx_status st = check_desc("gsx_model_select_neighbors", desc->filter, desc->flags, desc->radius, desc->max_count, desc->grid_bits);
    if (st) return st;
    if (desc->selection_op > (uint32_t)GSX_SELECTION_REMOVE) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_neighbors: unknown selection op %u", desc->selection_op);
    if (desc->count_lo > desc->count_hi || desc->count_hi > desc->max_count)
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_neighbors: counts [%u, %u] under max_count %u", desc->count_lo, desc->count_hi, desc->max_count);
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_neighbors: a reserved word is not 0");
    Model* m = nullptr;
    if ((st = neighbor_model(v, "gsx_model_select_neighbors", key, &m))) return st;
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    NeighborJob job;
    if ((st = neighbor_job(v, m, desc->radius, desc->max_count, desc->grid_bits, &job))) return st;  // (before anything of the model changes)
    // what gsx_model_select_range does: the epoch, the buffer, the write on the viewer's stream, the wait, then "has a selection"
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    m->edit_epoch += 1;
    if ((st = ensure_selection(v, m))) return st;
    job.count_lo = desc->count_lo;
    job.count_hi = desc->count_hi;
    job.op = desc->selection_op;
    job.selection_valid = m->has_selection ? 1u : 0u;
    job.selection = m->selection.as<uint32_t>();
    if ((st = enqueue_counts(v, m, f, job))) return st;
    HIPCHK(launch_neighbors_select(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    m->has_selection = true;
    uint32_t host[kNbResultWords];
    HIPCHK(gsx::op::Memcpy(host, job.result, sizeof host, hipMemcpyDeviceToHost));
    if (out_hit) *out_hit = host[kNbHit];
    if (out_selected) *out_selected = host[kNbSelected];
    return GSX_OK;
}

}  // extern "C"
