// gsx_api_knn.cpp — C ABI of the nearest neighbours (spec/RENDER_SPEC.md section 20; kernels_knn.hip): gsx_model_knn and
// gsx_model_select_knn.  The filter is model_filter's, the grid section 18's (neighbors_host.h), rebuilt once a round at the round's
// radius, the rules knn_math.h's, the workspace the model operations' (v->extract_ws): the grid's regions, then [the kNN's words, 128 B
// | its partials, 32 B a workgroup | the box, its partials and histogram | the scores, 4 B a Gaussian | two lists, 16 B a Gaussian
// each | the rows, 4 k B a Gaussian, only when the caller wants them].  The host looks at the device once for the box
// (participants_box) and once a round for the unresolved count; the rounds' schedule is radius_search.h's, its uncapped case.
#include "gsx_state.h"
#include "knn_math.h"
#include "neighbors_host.h"
#include "radius_search.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_knn_desc) == 32 && sizeof(gsx_knn_stats_t) == 72 && sizeof(gsx_knn_select_desc) == 48, "spec section 20's layouts");
static_assert(GSX_KNN_MAX_K == kKnnMaxK, "knn_math.h restates the bound on k");
static_assert(GSX_KNN_SCORE_KTH == kKnnScoreKth && GSX_KNN_SCORE_MEAN == kKnnScoreMean, "the kernels' scores");
static_assert(GSX_KNN_SELECT_RANGE == kKnnSelectRange && GSX_KNN_SELECT_OUTLIERS == kKnnSelectOutliers, "the kernels' modes");

// The workspace of a model of n Gaussians under a table of 2^bits buckets, with or without rows of k; returns its bytes.
size_t knn_ws(char* ws, uint64_t n, uint32_t bits, uint32_t k, bool rows, KnnJob* job) {
    WsCursor c{ws, neighbor_ws(ws, n, bits, &job->nb)};
    job->words = c.take<uint32_t>(4 * kKnnWords);
    job->partials = c.take<uint32_t>(4 * kKnnPartialWords * (size_t)extract_groups(n));
    job->box = take_box(c);
    job->scores = c.take<float>(4 * (size_t)n);
    job->list[0] = c.take<uint4>(16 * (size_t)n);
    job->list[1] = c.take<uint4>(16 * (size_t)n);
    job->rows = rows ? c.take<float>(4 * (size_t)n * k) : nullptr;
    return c.at;
}

// what both calls check about (filter, flags, k, score, radius_hint, grid_bits, max_rounds)
gsx_status check_knn(const char* fn, uint32_t filter, uint32_t flags, uint32_t k, uint32_t score, float radius_hint, uint32_t grid_bits, uint32_t max_rounds) {
    if (filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, filter);
    if (flags) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (none are defined)", fn, flags);
    if (k < 1u || k > kKnnMaxK) return fail(GSX_ERR_INVALID_ARG, "%s: k %u is not in 1 .. %u", fn, k, kKnnMaxK);
    if (score > (uint32_t)GSX_KNN_SCORE_MEAN) return fail(GSX_ERR_INVALID_ARG, "%s: unknown score %u", fn, score);
    if (!(radius_hint >= 0.0f) || (radius_hint > 0.0f && !nb_radius_ok(radius_hint)))
        return fail(GSX_ERR_INVALID_ARG, "%s: the radius hint %g is negative or NaN, or not finite, or its float32 square is 0 or inf", fn, (double)radius_hint);
    if (grid_bits > kNbMaxBits) return fail(GSX_ERR_INVALID_ARG, "%s: grid_bits %u is above %u", fn, grid_bits, kNbMaxBits);
    if (max_rounds > kKnnMaxRounds) return fail(GSX_ERR_INVALID_ARG, "%s: max_rounds %u is above %u", fn, max_rounds, kKnnMaxRounds);
    return GSX_OK;
}

// The workspace (grown if need be: the only step that can fail for memory) and the job of a call; n > 0.
gsx_status knn_job(gsx_viewer* v, const Model* m, uint32_t k, uint32_t score, uint32_t grid_bits, bool rows, KnnJob* job) {
    const uint32_t bits = grid_bits ? grid_bits : nb_auto_bits(m->n);
    const gsx_status st = place_job(v, job, [&](char* ws, KnnJob* j) { return knn_ws(ws, m->n, bits, k, rows, j); });
    if (st) return st;
    job->nb.bits = bits;
    job->nb.max_count = kNbMaxCount;
    job->k = k;
    job->score = score;
    return GSX_OK;
}

// The whole search and the statistics, enqueued and, between rounds, waited for: the scores (and rows) and the kNN's words are in the
// workspace when the stream reaches its end, and so are the participant bits of the last grid.
gsx_status run_knn(gsx_viewer* v, const Model* m, const ModelFilter& f, KnnJob& job, float radius_hint, uint32_t max_rounds, gsx_knn_stats_t* stats) {
    const uint64_t n = m->n;
    HIPCHK(gsx::op::MemsetAsync(job.words, 0, 4 * kKnnWords, v->stream));
    RadiusSearch s{{}, {}, 0u, radius_hint, job.k, 0.0f, max_rounds};  // (uncapped)
    gsx_status st = participants_box(v, m, f, job.box, [&] { return launch_knn_fill(v->stream, n, job); }, &s, &stats->n_nonfinite);
    if (st) return st;
    stats->count = s.P;
    const uint4* src = job.nb.records;  // the first list: the grid's records
    // the participant bits, the table and the records at radius r (also without participants: the select reads the participant bits)
    const auto grid = [&](float r, bool) { return enqueue_grid_at(v, m, f, job.nb, r); };
    const auto round = [&](uint32_t i, uint32_t U, bool, uint32_t* left) -> gsx_status {
        const uint32_t to = i & 1u;
        HIPCHK(gsx::op::MemsetAsync(job.words + kKnnList + to, 0, 4, v->stream));
        HIPCHK(launch_knn_query(v->stream, n, src, U, to, job));
        HIPCHK(gsx::op::StreamSynchronize(v->stream));  // the one look a round: how many are left
        HIPCHK(gsx::op::Memcpy(left, job.words + kKnnList + to, 4, hipMemcpyDeviceToHost));
        src = job.list[to];
        return GSX_OK;
    };
    const auto brute = [&](uint32_t U) -> gsx_status {
        HIPCHK(launch_knn_brute(v->stream, n, src, U, s.P, job));
        return GSX_OK;
    };
    if ((st = radius_search<gsx_status>(s, s.P, grid, round, brute))) return st;
    stats->first_radius = s.first_radius;
    stats->rounds = s.rounds;
    stats->n_brute = s.n_brute;
    HIPCHK(launch_knn_stats(v->stream, n, job));
    return GSX_OK;
}

// the words of a finished call into the caller's stats (the counts are there already)
void read_stats(const uint32_t* w, gsx_knn_stats_t* stats) {
    stats->n_scored = w[kKnnScored];
    stats->score_min = nb_from_bits(w[kKnnScoreMin]);
    stats->score_max = nb_from_bits(w[kKnnScoreMax]);
    stats->threshold = nb_from_bits(w[kKnnThreshold]);
    __builtin_memcpy(&stats->mean, w + kKnnMean, 8);
    __builtin_memcpy(&stats->std, w + kKnnStd, 8);
}

}  // namespace

extern "C" {

void gsx_knn_desc_default(gsx_knn_desc* d) {
    if (!d) return;
    *d = gsx_knn_desc{};
    d->k = 3u;
    d->score = GSX_KNN_SCORE_MEAN;
}

gsx_status gsx_model_knn(gsx_viewer* v, const char* key, const gsx_knn_desc* desc, float* out_d2, float* out_score, gsx_knn_stats_t* out) {
    if (!v || !key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_knn: null argument");
    gsx_status st = check_knn("gsx_model_knn", desc->filter, desc->flags, desc->k, desc->score, desc->radius_hint, desc->grid_bits, desc->max_rounds);
    if (st) return st;
    if (desc->reserved != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_knn: reserved is %u, not 0", desc->reserved);
    Model* m = nullptr;
    if ((st = neighbor_model(v, "gsx_model_knn", key, &m))) return st;
    *out = gsx_knn_stats_t{};
    out->grid_bits = desc->grid_bits ? desc->grid_bits : nb_auto_bits(m->n);
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    KnnJob job;
    if ((st = knn_job(v, m, desc->k, desc->score, desc->grid_bits, out_d2 != nullptr, &job))) return st;
    job.mode = GSX_KNN_SELECT_RANGE;  // (no threshold)
    if ((st = run_knn(v, m, model_filter(m, desc->filter, false), job, desc->radius_hint, desc->max_rounds, out))) return st;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t host[kKnnWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, out);
    if (out_d2) HIPCHK(gsx::op::Memcpy(out_d2, job.rows, 4 * (size_t)n * desc->k, hipMemcpyDeviceToHost));
    if (out_score) HIPCHK(gsx::op::Memcpy(out_score, job.scores, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_model_select_knn(gsx_viewer* v, const char* key, const gsx_knn_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected,
                                gsx_knn_stats_t* out_stats) {
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_knn: null argument");
    gsx_status st = check_knn("gsx_model_select_knn", desc->filter, desc->flags, desc->k, desc->score, desc->radius_hint, desc->grid_bits, desc->max_rounds);
    if (st) return st;
    if ((st = check_selection_op("gsx_model_select_knn", desc->selection_op))) return st;
    if (desc->mode > (uint32_t)GSX_KNN_SELECT_OUTLIERS) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_knn: unknown mode %u", desc->mode);
    if (desc->mode == (uint32_t)GSX_KNN_SELECT_RANGE ? !(desc->lo <= desc->hi && desc->std_ratio == 0.0f)  // (a NaN bound compares false)
                                                     : !(nb_finite(desc->std_ratio) && desc->lo == 0.0f && desc->hi == 0.0f))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_knn: bounds [%g, %g], std_ratio %g in mode %u (range: lo <= hi, neither NaN, std_ratio 0; outliers: a finite std_ratio, lo and hi 0)",
                    (double)desc->lo, (double)desc->hi, (double)desc->std_ratio, desc->mode);
    Model* m = nullptr;
    if ((st = neighbor_model(v, "gsx_model_select_knn", key, &m))) return st;
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    gsx_knn_stats_t stats{};
    stats.grid_bits = desc->grid_bits ? desc->grid_bits : nb_auto_bits(m->n);
    if (out_stats) *out_stats = stats;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    KnnJob job;
    if ((st = knn_job(v, m, desc->k, desc->score, desc->grid_bits, false, &job))) return st;  // (before anything of the model changes)
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    if ((st = select_begin(v, m, desc->selection_op, job.nb.partials, &job.nb.sel))) return st;
    job.mode = desc->mode;
    job.lo = desc->lo;
    job.hi = desc->hi;
    job.std_ratio = desc->std_ratio;
    if ((st = run_knn(v, m, f, job, desc->radius_hint, desc->max_rounds, &stats))) return st;
    HIPCHK(launch_knn_select(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(m);
    uint32_t host[kKnnWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, &stats);
    if (out_hit) *out_hit = host[kKnnHit];
    if (out_selected) *out_selected = host[kKnnSelected];
    if (out_stats) *out_stats = stats;
    return GSX_OK;
}

}  // extern "C"
