// gsx_api_clusters.cpp — C ABI of the model clusters (spec/RENDER_SPEC.md section 19; kernels_clusters.hip): gsx_model_clusters and
// gsx_model_select_clusters.  The filter is model_filter's, the grid section 18's (neighbors_host.h), the workspace the model
// operations' (v->extract_ws): the grid's regions, then [the labels | the label sizes | the sizes by Gaussian | the seeded labels],
// 4 B a Gaussian each.
#include "gsx_state.h"
#include "clusters_math.h"
#include "neighbors_host.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_cluster_desc) == 24 && sizeof(gsx_cluster_stats_t) == 40 && sizeof(gsx_cluster_select_desc) == 40, "spec section 19's layouts");
static_assert(GSX_CLUSTER_NONE == kClNone, "clusters_math.h restates the label of a non-participant");
static_assert(GSX_CLUSTER_BY_SIZE == kClBySize && GSX_CLUSTER_LARGEST == kClLargest && GSX_CLUSTER_SEEDED == kClSeeded, "the kernels' modes");

// The workspace of a model of n Gaussians under a table of 2^bits buckets; returns its bytes.
size_t cluster_ws(char* ws, uint64_t n, uint32_t bits, ClusterJob* job) {
    WsCursor c{ws, neighbor_ws(ws, n, bits, &job->nb)};
    job->label = c.take<uint32_t>(4 * (size_t)n);
    job->size = c.take<uint32_t>(4 * (size_t)n);
    job->sizes = c.take<uint32_t>(4 * (size_t)n);
    job->seeded = c.take<uint32_t>(4 * (size_t)n);
    return c.at;
}

// The workspace (grown if need be: the only step that can fail for memory) and the job of a call; n > 0.
gsx_status cluster_job(gsx_viewer* v, const Model* m, float radius, uint32_t grid_bits, ClusterJob* job) {
    const uint32_t bits = grid_bits ? grid_bits : nb_auto_bits(m->n);
    const gsx_status st = place_job(v, job, [&](char* ws, ClusterJob* j) { return cluster_ws(ws, m->n, bits, j); });
    if (st) return st;
    const NbGrid g = nb_grid(radius);
    job->nb.r2 = g.r2;
    job->nb.inv_h = g.inv_h;
    job->nb.bits = bits;
    job->nb.max_count = kNbMaxCount;
    return GSX_OK;
}

// Every pass up to the stats, enqueued: labels, sizes and the result block are in the workspace when the stream reaches its end.
gsx_status enqueue_clusters(gsx_viewer* v, const Model* m, const ModelFilter& f, const ClusterJob& job) {
    const gsx_status st = enqueue_grid(v, m, f, job.nb);
    if (st) return st;
    HIPCHK(gsx::op::MemsetAsync(job.size, 0, 4 * (size_t)m->n, v->stream));
    if (job.seeds) HIPCHK(gsx::op::MemsetAsync(job.seeded, 0, 4 * (size_t)m->n, v->stream));
    HIPCHK(launch_clusters_hook(v->stream, m->n, job));  // (after the cell pass, which zeroes the region that is parent[] here)
    HIPCHK(launch_clusters_label(v->stream, m->n, job));
    HIPCHK(launch_clusters_stats(v->stream, m->n, job));
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_cluster_desc_default(gsx_cluster_desc* d) {
    if (!d) return;
    *d = gsx_cluster_desc{};
    d->radius = 1.0f;
}

gsx_status gsx_model_clusters(gsx_viewer* v, const char* key, const gsx_cluster_desc* desc, uint32_t* out_labels, uint32_t* out_sizes, gsx_cluster_stats_t* out) {
    if (!v || !key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_clusters: null argument");
    gsx_status st = check_desc("gsx_model_clusters", desc->filter, desc->flags, desc->radius, kNbMaxCount, desc->grid_bits);
    if (st) return st;
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_clusters: a reserved word is not 0");
    Model* m = nullptr;
    if ((st = neighbor_model(v, "gsx_model_clusters", key, &m))) return st;
    *out = gsx_cluster_stats_t{};
    out->largest_label = GSX_CLUSTER_NONE;
    out->grid_bits = desc->grid_bits ? desc->grid_bits : nb_auto_bits(m->n);
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    ClusterJob job;
    if ((st = cluster_job(v, m, desc->radius, desc->grid_bits, &job))) return st;
    if ((st = enqueue_clusters(v, m, model_filter(m, desc->filter, false), job))) return st;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t host[kNbResultWords];
    HIPCHK(gsx::op::Memcpy(host, job.nb.result, sizeof host, hipMemcpyDeviceToHost));
    out->count = host[kNbCount];
    out->n_nonfinite = host[kNbNonfinite];
    out->n_clusters = host[kClClusters];
    out->largest_size = host[kClKey + 1u];
    out->largest_label = ~host[kClKey];  // (0 participants: the key is 0, the label GSX_CLUSTER_NONE)
    if (out_labels) HIPCHK(gsx::op::Memcpy(out_labels, job.label, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (out_sizes) HIPCHK(gsx::op::Memcpy(out_sizes, job.sizes, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_model_select_clusters(gsx_viewer* v, const char* key, const gsx_cluster_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected) {
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_clusters: null argument");
    gsx_status st = check_desc("gsx_model_select_clusters", desc->filter, desc->flags, desc->radius, kNbMaxCount, desc->grid_bits);
    if (st) return st;
    if ((st = check_selection_op("gsx_model_select_clusters", desc->selection_op))) return st;
    if (desc->mode > (uint32_t)GSX_CLUSTER_SEEDED) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_clusters: unknown mode %u", desc->mode);
    if (desc->mode == (uint32_t)GSX_CLUSTER_BY_SIZE ? (desc->size_lo < 1u || desc->size_lo > desc->size_hi) : (desc->size_lo != 0u || desc->size_hi != 0u))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_clusters: sizes [%u, %u] in mode %u (by size: 1 <= size_lo <= size_hi; otherwise both 0)", desc->size_lo,
                    desc->size_hi, desc->mode);
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_clusters: a reserved word is not 0");
    Model* m = nullptr;
    if ((st = neighbor_model(v, "gsx_model_select_clusters", key, &m))) return st;
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    ClusterJob job;
    if ((st = cluster_job(v, m, desc->radius, desc->grid_bits, &job))) return st;  // (before anything of the model changes)
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    if ((st = select_begin(v, m, desc->selection_op, job.nb.partials, &job.nb.sel))) return st;  // (a model without a selection has no seeds)
    job.mode = desc->mode;
    job.size_lo = desc->size_lo;
    job.size_hi = desc->size_hi;
    job.seeds = desc->mode == (uint32_t)GSX_CLUSTER_SEEDED ? 1u : 0u;
    if ((st = enqueue_clusters(v, m, f, job))) return st;
    HIPCHK(launch_clusters_select(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(m);
    uint32_t host[kNbResultWords];
    HIPCHK(gsx::op::Memcpy(host, job.nb.result, sizeof host, hipMemcpyDeviceToHost));
    if (out_hit) *out_hit = host[kNbHit];
    if (out_selected) *out_selected = host[kNbSelected];
    return GSX_OK;
}

}  // extern "C"
