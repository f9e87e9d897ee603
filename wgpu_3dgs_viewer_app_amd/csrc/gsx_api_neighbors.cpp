// gsx_api_neighbors.cpp — C ABI of the neighbour counts (spec/RENDER_SPEC.md section 18; kernels_neighbors.hip):
// gsx_model_neighbors and gsx_model_select_neighbors.  The filter is model_filter's, the workspace the model operations'
// (v->extract_ws), laid out by neighbors_host.h, which also holds what the clusters (gsx_api_clusters.cpp) share with these calls.
#include "gsx_state.h"
#include "neighbors_math.h"
#include "neighbors_host.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_neighbor_desc) == 24 && sizeof(gsx_neighbor_stats_t) == 24 && sizeof(gsx_neighbor_select_desc) == 40, "spec section 18's layouts");
static_assert(GSX_NEIGHBOR_MAX_COUNT == kNbMaxCount, "neighbors_math.h restates the cap");

// The workspace (grown if need be: the only step that can fail for memory) and the job of a call; n > 0.
gsx_status neighbor_job(gsx_viewer* v, const Model* m, float radius, uint32_t max_count, uint32_t grid_bits, NeighborJob* job) {
    const uint32_t bits = grid_bits ? grid_bits : nb_auto_bits(m->n);
    const gsx_status st = place_job(v, job, [&](char* ws, NeighborJob* j) { return neighbor_ws(ws, m->n, bits, j); });
    if (st) return st;
    const NbGrid g = nb_grid(radius);
    job->r2 = g.r2;
    job->inv_h = g.inv_h;
    job->bits = bits;
    job->max_count = max_count;
    return GSX_OK;
}

// Every pass up to the query, enqueued: the counts and the histogram are in the workspace when the stream reaches its end.
gsx_status enqueue_counts(gsx_viewer* v, const Model* m, const ModelFilter& f, const NeighborJob& job) {
    const gsx_status st = enqueue_grid(v, m, f, job);
    if (st) return st;
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
    if ((st = check_selection_op("gsx_model_select_neighbors", desc->selection_op))) return st;
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
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    if ((st = select_begin(v, m, desc->selection_op, job.partials, &job.sel))) return st;
    job.count_lo = desc->count_lo;
    job.count_hi = desc->count_hi;
    if ((st = enqueue_counts(v, m, f, job))) return st;
    HIPCHK(launch_neighbors_select(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(m);
    uint32_t host[kNbResultWords];
    HIPCHK(gsx::op::Memcpy(host, job.result, sizeof host, hipMemcpyDeviceToHost));
    if (out_hit) *out_hit = host[kNbHit];
    if (out_selected) *out_selected = host[kNbSelected];
    return GSX_OK;
}

}  // extern "C"
