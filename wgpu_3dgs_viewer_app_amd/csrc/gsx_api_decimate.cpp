// gsx_api_decimate.cpp — C ABI of the model decimate (spec/RENDER_SPEC.md section 22; kernels_decimate.hip): gsx_model_decimate and
// gsx_model_decimate_edge.  The filter is model_filter's, the grid gsx_model_neighbors' (neighbors_host.h: enqueue_grid) with the cell
// edge given instead of a radius, the workspace the model operations' (v->extract_ws): the grid's regions first, the decimate's behind
// them: [its words, 128 B | the two scans' totals, 128 B | the big buckets | the head bits | their partials | their bases | the keep
// bits | their partials | their bases | run_start | run_dst | cell_start | cell_len | the map | the ordered records, 16 B a Gaussian].
#include "decimate_math.h"
#include "gsx_state.h"
#include "neighbors_host.h"
#include "neighbors_math.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_decimate_desc) == 24 && sizeof(gsx_decimate_stats_t) == 40, "spec section 22's layouts");

// The decimate's regions behind the grid's `at` bytes; returns the workspace's bytes.
size_t decimate_ws(char* ws, size_t at, uint64_t n, DecimateJob* job) {
    const size_t groups = (size_t)extract_groups(n), bit_words = (size_t)((n + 31u) / 32u);
    WsCursor c{ws, at};
    job->words = c.take<uint32_t>(4 * kDecWords);
    job->totals = c.take<uint64_t>(16);
    job->big_cap = (uint32_t)(n / 64u + 2u);
    job->big = c.take<uint32_t>(4 * (size_t)job->big_cap);
    job->heads = c.take<uint32_t>(4 * bit_words);
    job->head_partials = c.take<uint32_t>(4 * groups);
    job->head_bases = c.take<uint32_t>(4 * groups);
    job->keep = c.take<uint32_t>(4 * bit_words);
    job->keep_partials = c.take<uint32_t>(4 * groups);
    job->keep_bases = c.take<uint32_t>(4 * groups);
    job->run_start = c.take<uint32_t>(4 * ((size_t)n + 1u));
    job->run_dst = c.take<uint32_t>(4 * (size_t)n);
    job->cell_start = c.take<uint32_t>(4 * (size_t)n);
    job->cell_len = c.take<uint32_t>(4 * (size_t)n);
    job->map = c.take<uint32_t>(4 * (size_t)n);
    job->sorted = c.take<uint4>(16 * (size_t)n);
    return c.at;
}

// what both calls check about (filter, flags, grid_bits)
gsx_status check_filter(const char* fn, uint32_t filter, uint32_t flags, uint32_t grid_bits) {
    if (filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, filter);
    if (flags & ~(uint32_t)GSX_EXTRACT_INVERT) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (GSX_EXTRACT_INVERT alone is defined)", fn, flags);
    if (grid_bits > kNbMaxBits) return fail(GSX_ERR_INVALID_ARG, "%s: grid_bits %u is above %u", fn, grid_bits, kNbMaxBits);
    return GSX_OK;
}

// The workspace (grown if need be: the only step before dst that can fail for memory) and the job of a model; n > 0.
gsx_status decimate_job(gsx_viewer* v, const Model* m, uint32_t bits, DecimateJob* job) {
    // (decimate's regions start behind the grid's bytes)
    const gsx_status st = place_job(v, job, [&](char* ws, DecimateJob* j) { return decimate_ws(ws, neighbor_ws(ws, m->n, bits, &j->nb), m->n, j); });
    if (st) return st;
    job->nb.bits = bits;
    job->nb.max_count = 1u;
    return GSX_OK;
}

struct DecimateCount {
    uint64_t count, n_nonfinite, cells, singletons;
    uint32_t largest_cell;
};

// The grid of the edge, the ordering and the cells, enqueued and waited for: the one wait of a call.
gsx_status count_cells(gsx_viewer* v, const Model* m, const ModelFilter& f, float cell, DecimateJob& job, DecimateCount* out) {
    const uint64_t n = m->n;
    job.nb.inv_h = dec_grid(cell).inv_h;
    job.nb.r2 = 0.0f;
    gsx_status st = enqueue_grid(v, m, f, job.nb);
    if (st) return st;
    HIPCHK(gsx::op::MemsetAsync(job.words, 0, 4 * (kDecBig + 1u), v->stream));
    HIPCHK(gsx::op::MemsetAsync(job.totals, 0, 16, v->stream));
    HIPCHK(gsx::op::MemsetAsync(job.keep, 0, 4 * (size_t)((n + 31u) / 32u), v->stream));
    HIPCHK(gsx::op::MemsetAsync(job.map, 0xFF, 4 * (size_t)n, v->stream));
    HIPCHK(launch_decimate_order(v->stream, n, job));
    HIPCHK(launch_decimate_cells(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t nb_words[kNbResultWords], words[kDecWords];
    uint64_t totals[2];
    HIPCHK(gsx::op::Memcpy(nb_words, job.nb.result, sizeof nb_words, hipMemcpyDeviceToHost));
    HIPCHK(gsx::op::Memcpy(words, job.words, sizeof words, hipMemcpyDeviceToHost));
    HIPCHK(gsx::op::Memcpy(totals, job.totals, sizeof totals, hipMemcpyDeviceToHost));
    if (totals[0] != totals[1] || totals[0] > nb_words[kNbCount])
        return fail(GSX_ERR_HIP, "gsx_model_decimate: %llu heads, %llu representatives, %u participants", (unsigned long long)totals[0],
                    (unsigned long long)totals[1], nb_words[kNbCount]);
    out->count = nb_words[kNbCount];
    out->n_nonfinite = nb_words[kNbNonfinite];
    out->cells = totals[0];
    out->singletons = words[kDecSingletons];
    out->largest_cell = words[kDecLargest];
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_decimate_desc_default(gsx_decimate_desc* d) {
    if (!d) return;
    *d = gsx_decimate_desc{};
}

gsx_status gsx_model_decimate(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_decimate_desc* desc, uint32_t* out_map,
                              gsx_decimate_stats_t* out) {
    static const char* fn = "gsx_model_decimate";
    if (!v || !src_key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    gsx_status st = check_filter(fn, desc->filter, desc->flags, desc->grid_bits);
    if (st) return st;
    if (!dec_cell_ok(desc->cell)) return fail(GSX_ERR_INVALID_ARG, "%s: the cell edge %g is not finite and above 0, or its float32 reciprocal is 0 or inf", fn, (double)desc->cell);
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u) return fail(GSX_ERR_INVALID_ARG, "%s: a reserved word is not 0", fn);
    if (dst_key && !strcmp(src_key, dst_key)) return fail(GSX_ERR_INVALID_ARG, "%s: dst_key equals src_key '%s'", fn, src_key);
    Model* m = nullptr;
    if ((st = neighbor_model(v, fn, src_key, &m))) return st;  // behind the frames in flight on the lanes
    if (dst_key && v->models.count(dst_key)) return fail(GSX_ERR_INVALID_ARG, "%s: model '%s' exists", fn, dst_key);
    const uint64_t n = m->n;
    *out = gsx_decimate_stats_t{};
    out->grid_bits = desc->grid_bits ? desc->grid_bits : nb_auto_bits(n);
    if (out_map)
        for (uint64_t i = 0; i < n; ++i) out_map[i] = kDecNoCell;
    if (n == 0) return GSX_OK;

    DecimateJob job;
    if ((st = decimate_job(v, m, out->grid_bits, &job))) return st;
    DecimateCount c{};
    if ((st = count_cells(v, m, model_filter(m, desc->filter, (desc->flags & GSX_EXTRACT_INVERT) != 0), desc->cell, job, &c))) return st;
    out->count = c.count;
    out->n_nonfinite = c.n_nonfinite;
    out->cells = c.cells;
    out->singletons = c.singletons;
    out->largest_cell = c.largest_cell;
    if (out_map) HIPCHK(gsx::op::Memcpy(out_map, job.map, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (!dst_key || c.cells == 0) return GSX_OK;  // count only, or nothing participates: no model

    Model* d = nullptr;
    // (every plane of every Gaussian of dst is written below: no zero fill)
    if ((st = model_create(v, dst_key, c.cells, m->sh_kind, m->cov_kind, false, &d))) return st;
    const ExtractPlanes src = extract_planes(m, false), dst = extract_planes(d, false);
    // every representative as stored bits (a one-member cell is done with that), then the cells of two members and more over them
    hipError_t e = launch_extract_scatter(v->stream, (int)m->sh_kind, (int)m->cov_kind, n, c.cells, 0, job.keep, job.keep_bases, src, dst);
    if (e == hipSuccess && c.singletons != c.cells) e = launch_decimate_merge(v->stream, (int)m->sh_kind, (int)m->cov_kind, n, c.cells, job, src, dst);
    if (e != hipSuccess) {  // no dst left behind
        (void)gsx::op::StreamSynchronize(v->stream);
        v->models.erase(dst_key);
        return fail(e == hipErrorOutOfMemory ? GSX_ERR_OOM : GSX_ERR_HIP, "%s: the launch failed: %s", fn, hipGetErrorString(e));
    }
    d->mt = m->mt;
    return GSX_OK;
}

gsx_status gsx_model_decimate_edge(gsx_viewer* v, const char* key, uint32_t filter, uint32_t flags, uint64_t target_cells, float* out_cell,
                                   uint64_t* out_cells) {
    static const char* fn = "gsx_model_decimate_edge";
    if (!v || !key || !out_cell || !out_cells) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    gsx_status st = check_filter(fn, filter, flags, 0u);
    if (st) return st;
    if (target_cells == 0) return fail(GSX_ERR_INVALID_ARG, "%s: target_cells is 0", fn);
    Model* m = nullptr;
    if ((st = neighbor_model(v, fn, key, &m))) return st;
    *out_cell = 0.0f;
    *out_cells = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    DecimateJob job;
    if ((st = decimate_job(v, m, nb_auto_bits(n), &job))) return st;
    const ModelFilter f = model_filter(m, filter, (flags & GSX_EXTRACT_INVERT) != 0);
    // the participants' extent: the grid's reduce alone (count, origin and maximum in its result block)
    HIPCHK(gsx::op::MemsetAsync(job.nb.result, 0, 4 * kNbResultWords, v->stream));
    HIPCHK(launch_neighbors_reduce(v->stream, n, f, extract_planes(m, false).pc, job.nb));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t words[kNbResultWords];
    HIPCHK(gsx::op::Memcpy(words, job.nb.result, sizeof words, hipMemcpyDeviceToHost));
    if (words[kNbCount] == 0u) return GSX_OK;  // nothing participates: edge 0, 0 cells
    float extent = 0.0f;
    for (int a = 0; a < 3; ++a) extent = fmaxf(extent, nb_from_bits(words[kNbMax + a]) - nb_from_bits(words[kNbOrigin + a]));
    const auto count = [&](float edge, uint64_t* cells) {
        DecimateCount c{};
        const gsx_status e = count_cells(v, m, f, edge, job, &c);
        *cells = c.cells;
        return (int)e;
    };
    return (gsx_status)dec_find_edge(extent, target_cells, count, out_cell, out_cells);
}

}  // extern "C"
