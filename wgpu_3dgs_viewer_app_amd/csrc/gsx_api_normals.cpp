// gsx_api_normals.cpp — C ABI of the model normals (spec/RENDER_SPEC.md section 26; kernels_normals.hip): gsx_model_normals and
// gsx_model_select_normals, and of section 27's kept normals: gsx_model_normals_keep, _kept and _reset (Model::normals).  The filter is model_filter's, the grid section 18's (neighbors_host.h), rebuilt once a round at the
// round's radius, the rules normals_math.h's, the workspace the model operations' (v->extract_ws): the grid's regions, then [the
// normals' words, 128 B | its partials, 32 B a workgroup | the box, its partials and histogram | the normals, 12 B a Gaussian | the
// variations, 4 B a Gaussian | two lists, 16 B a Gaussian each | the indices, 4 k B a Gaussian, only when the caller wants them].  The
// host looks at the device once for the box (participants_box) and once a round for the unresolved count; the rounds' schedule is
// radius_search.h's, its uncapped case: this file supplies the grid, a round and the fallback and decides nothing about them.
#include "gsx_state.h"
#include "neighbors_host.h"
#include "normals_math.h"
#include "radius_search.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_normals_desc) == 48 && sizeof(gsx_normals_stats_t) == 64 && sizeof(gsx_normals_select_desc) == 80, "spec section 26's layouts");
static_assert(sizeof(gsx_normals_kept_t) == 48, "spec section 27's layout");
static_assert(GSX_NORMALS_MIN_K == kNormalsMinK && GSX_NORMALS_MAX_K == kNormalsMaxK && GSX_NORMALS_MAX_K == kKnnMaxK, "normals_math.h restates the bounds on k");
static_assert(GSX_NORMALS_ORIENT_CANONICAL == kNormalsOrientCanonical && GSX_NORMALS_ORIENT_TOWARD == kNormalsOrientToward, "the kernels' orients");
static_assert(GSX_NORMALS_SELECT_VARIATION == kNormalsSelectVariation && GSX_NORMALS_SELECT_FACING == kNormalsSelectFacing, "the kernels' modes");
static_assert(GSX_NORMALS_ABS == kNormalsAbs && GSX_NORMALS_NONE == kNormalsNone, "the kernels' flag and their 'none'");

// The workspace of a model of n Gaussians under a table of 2^bits buckets, with or without the indices of k; returns its bytes.
size_t normals_ws(char* ws, uint64_t n, uint32_t bits, uint32_t k, bool indices, NormalsJob* job) {
    WsCursor c{ws, neighbor_ws(ws, n, bits, &job->nb)};
    job->words = c.take<uint32_t>(4 * kNormalsWords);
    job->partials = c.take<uint32_t>(4 * kNormalsPartialWords * (size_t)extract_groups(n));
    job->box = take_box(c);
    job->normals = c.take<float>(12 * (size_t)n);
    job->variation = c.take<float>(4 * (size_t)n);
    job->list[0] = c.take<uint4>(16 * (size_t)n);
    job->list[1] = c.take<uint4>(16 * (size_t)n);
    job->indices = indices ? c.take<uint32_t>(4 * (size_t)n * k) : nullptr;
    return c.at;
}

// what both calls check about (filter, k, orient, toward, radius_hint, grid_bits, max_rounds)
gsx_status check_normals(const char* fn, uint32_t filter, uint32_t k, uint32_t orient, const float toward[3], float radius_hint, uint32_t grid_bits, uint32_t max_rounds) {
    if (filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, filter);
    if (k < kNormalsMinK || k > kNormalsMaxK) return fail(GSX_ERR_INVALID_ARG, "%s: k %u is not in %u .. %u", fn, k, kNormalsMinK, kNormalsMaxK);
    if (orient > kNormalsOrientToward) return fail(GSX_ERR_INVALID_ARG, "%s: unknown orient %u", fn, orient);
    if (orient == kNormalsOrientToward && !(nb_finite(toward[0]) && nb_finite(toward[1]) && nb_finite(toward[2])))
        return fail(GSX_ERR_INVALID_ARG, "%s: toward (%g, %g, %g) is not finite", fn, (double)toward[0], (double)toward[1], (double)toward[2]);
    if (!(radius_hint >= 0.0f) || (radius_hint > 0.0f && !nb_radius_ok(radius_hint)))
        return fail(GSX_ERR_INVALID_ARG, "%s: the radius hint %g is negative or NaN, or not finite, or its float32 square is 0 or inf", fn, (double)radius_hint);
    if (grid_bits > kNbMaxBits) return fail(GSX_ERR_INVALID_ARG, "%s: grid_bits %u is above %u", fn, grid_bits, kNbMaxBits);
    if (max_rounds > kKnnMaxRounds) return fail(GSX_ERR_INVALID_ARG, "%s: max_rounds %u is above %u", fn, max_rounds, kKnnMaxRounds);
    return GSX_OK;
}

// The workspace (grown if need be: the only step that can fail for memory) and the job of a call; n > 0.
gsx_status normals_job(gsx_viewer* v, const Model* m, uint32_t k, uint32_t orient, const float toward[3], uint32_t grid_bits, bool indices, NormalsJob* job) {
    const uint32_t bits = grid_bits ? grid_bits : nb_auto_bits(m->n);
    const gsx_status st = place_job(v, job, [&](char* ws, NormalsJob* j) { return normals_ws(ws, m->n, bits, k, indices, j); });
    if (st) return st;
    job->nb.bits = bits;
    job->nb.max_count = kNbMaxCount;
    job->k = k;
    job->orient = orient;
    for (int a = 0; a < 3; ++a) job->toward[a] = orient == kNormalsOrientToward ? toward[a] : 0.0f;
    job->pc = extract_planes(m, false).pc;
    return GSX_OK;
}

// The whole search with its fits and the statistics, enqueued and, between rounds, waited for: the normals, the variations (and the
// indices) and the words are in the workspace when the stream reaches its end, and so are the participant bits of the last grid.
gsx_status run_normals(gsx_viewer* v, const Model* m, const ModelFilter& f, NormalsJob& job, float radius_hint, uint32_t max_rounds, gsx_normals_stats_t* stats) {
    const uint64_t n = m->n;
    HIPCHK(gsx::op::MemsetAsync(job.words, 0, 4 * kNormalsWords, v->stream));
    RadiusSearch s{{}, {}, 0u, radius_hint, job.k, 0.0f, max_rounds};  // (uncapped)
    gsx_status st = participants_box(v, m, f, job.box, [&] { return launch_normals_fill(v->stream, n, job); }, &s, &stats->n_nonfinite);
    if (st) return st;
    stats->count = s.P;
    const uint4* src = job.nb.records;  // the first list: the grid's records
    const auto grid = [&](float r, bool) { return enqueue_grid_at(v, m, f, job.nb, r); };
    const auto round = [&](uint32_t i, uint32_t U, bool, uint32_t* left) -> gsx_status {
        const uint32_t to = i & 1u;
        HIPCHK(gsx::op::MemsetAsync(job.words + kNormalsList + to, 0, 4, v->stream));
        HIPCHK(launch_normals_query(v->stream, n, src, U, to, job));
        HIPCHK(gsx::op::StreamSynchronize(v->stream));  // the one look a round: how many are left
        HIPCHK(gsx::op::Memcpy(left, job.words + kNormalsList + to, 4, hipMemcpyDeviceToHost));
        src = job.list[to];
        return GSX_OK;
    };
    const auto brute = [&](uint32_t U) -> gsx_status {
        HIPCHK(launch_normals_brute(v->stream, n, src, U, s.P, job));
        return GSX_OK;
    };
    if ((st = radius_search<gsx_status>(s, s.P, grid, round, brute))) return st;
    stats->first_radius = s.first_radius;
    stats->rounds = s.rounds;
    stats->n_brute = s.n_brute;
    HIPCHK(launch_normals_stats(v->stream, n, job));
    return GSX_OK;
}

// the words of a finished call into the caller's stats (the counts are there already)
void read_stats(const uint32_t* w, gsx_normals_stats_t* stats) {
    stats->n_fitted = w[kNormalsFitted];
    stats->variation_min = nb_from_bits(w[kNormalsVarMin]);
    stats->variation_max = nb_from_bits(w[kNormalsVarMax]);
    __builtin_memcpy(&stats->mean, w + kNormalsMean, 8);
}

// the model takes the fresh plane; the older one, if any, is freed with `fresh`
void adopt_normals(Model* m, DevBuf& fresh, const gsx_normals_kept_t& kept) {
    std::swap(m->normals.p, fresh.p);
    std::swap(m->normals.bytes, fresh.bytes);
    std::swap(m->normals.borrowed, fresh.borrowed);
    m->normals_kept = kept;
}

// gsx_model_normals and gsx_model_normals_keep: one computation.  keep: the normals and the variations stay with the model, in a buffer
// allocated before anything runs and put in the older plane's place only when the stream has reached its end.
gsx_status normals_call(gsx_viewer* v, const char* fn, const char* key, const gsx_normals_desc* desc, float* out_normal, float* out_variation, uint32_t* out_index,
                        gsx_normals_stats_t* out, bool keep) {
    if (!v || !key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (desc->flags) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (none are defined)", fn, desc->flags);
    gsx_status st = check_normals(fn, desc->filter, desc->k, desc->orient, desc->toward, desc->radius_hint, desc->grid_bits, desc->max_rounds);
    if (st) return st;
    if (desc->reserved != 0u || desc->reserved2 != 0u) return fail(GSX_ERR_INVALID_ARG, "%s: the reserved words are %u, %u, not 0", fn, desc->reserved, desc->reserved2);
    Model* m = nullptr;
    if ((st = neighbor_model(v, fn, key, &m))) return st;
    *out = gsx_normals_stats_t{};
    out->grid_bits = desc->grid_bits ? desc->grid_bits : nb_auto_bits(m->n);
    const uint64_t n = m->n;
    gsx_normals_kept_t kept{};
    kept.present = 1u;
    kept.k = desc->k;
    kept.orient = desc->orient;
    kept.filter = desc->filter;
    for (int a = 0; a < 3; ++a) kept.toward[a] = desc->orient == kNormalsOrientToward ? desc->toward[a] : 0.0f;
    kept.count = n;
    DevBuf fresh;
    if (n == 0) {
        if (keep) {
            HIPCHK(fresh.ensure(16));
            adopt_normals(m, fresh, kept);
        }
        return GSX_OK;
    }
    NormalsJob job;
    if ((st = normals_job(v, m, desc->k, desc->orient, desc->toward, desc->grid_bits, out_index != nullptr, &job))) return st;
    if (keep) HIPCHK(fresh.ensure(16 * (size_t)n));
    if ((st = run_normals(v, m, model_filter(m, desc->filter, false), job, desc->radius_hint, desc->max_rounds, out))) return st;
    if (keep) {
        HIPCHK(gsx::op::MemcpyAsync(fresh.p, job.normals, 12 * (size_t)n, hipMemcpyDeviceToDevice, v->stream));
        HIPCHK(gsx::op::MemcpyAsync(fresh.as<float>() + 3 * (size_t)n, job.variation, 4 * (size_t)n, hipMemcpyDeviceToDevice, v->stream));
    }
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t host[kNormalsWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, out);
    if (out_normal) HIPCHK(gsx::op::Memcpy(out_normal, job.normals, 12 * (size_t)n, hipMemcpyDeviceToHost));
    if (out_variation) HIPCHK(gsx::op::Memcpy(out_variation, job.variation, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (out_index) HIPCHK(gsx::op::Memcpy(out_index, job.indices, 4 * (size_t)n * desc->k, hipMemcpyDeviceToHost));
    if (keep) {
        kept.n_fitted = out->n_fitted;
        adopt_normals(m, fresh, kept);
    }
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_normals_desc_default(gsx_normals_desc* d) {
    if (!d) return;
    *d = gsx_normals_desc{};
    d->k = 8u;
    d->orient = GSX_NORMALS_ORIENT_CANONICAL;
}

gsx_status gsx_model_normals(gsx_viewer* v, const char* key, const gsx_normals_desc* desc, float* out_normal, float* out_variation, uint32_t* out_index,
                             gsx_normals_stats_t* out) {
    return normals_call(v, "gsx_model_normals", key, desc, out_normal, out_variation, out_index, out, false);
}

gsx_status gsx_model_normals_keep(gsx_viewer* v, const char* key, const gsx_normals_desc* desc, gsx_normals_stats_t* out) {
    return normals_call(v, "gsx_model_normals_keep", key, desc, nullptr, nullptr, nullptr, out, true);
}

gsx_status gsx_model_normals_kept(gsx_viewer* v, const char* key, gsx_normals_kept_t* out, float* out_normal, float* out_variation) {
    if (!v || !key || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_normals_kept: null argument");
    Model* m = nullptr;
    const gsx_status st = neighbor_model(v, "gsx_model_normals_kept", key, &m);
    if (st) return st;
    *out = m->normals_kept;  // (zeros without a plane)
    if (!m->normals.p) return GSX_OK;
    const size_t n = (size_t)m->normals_kept.count;
    if (n == 0) return GSX_OK;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    if (out_normal) HIPCHK(gsx::op::Memcpy(out_normal, m->normals.p, 12 * n, hipMemcpyDeviceToHost));
    if (out_variation) HIPCHK(gsx::op::Memcpy(out_variation, m->normals.as<float>() + 3 * n, 4 * n, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_model_normals_reset(gsx_viewer* v, const char* key) {
    if (!v || !key) return fail(GSX_ERR_INVALID_ARG, "gsx_model_normals_reset: null argument");
    Model* m = nullptr;
    const gsx_status st = neighbor_model(v, "gsx_model_normals_reset", key, &m);
    if (st) return st;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));  // (nothing enqueued reads the plane any more)
    drop_normals(m);
    return GSX_OK;
}

gsx_status gsx_model_select_normals(gsx_viewer* v, const char* key, const gsx_normals_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected,
                                    gsx_normals_stats_t* out_stats) {
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_normals: null argument");
    if (desc->flags & ~kNormalsAbs) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_normals: unknown flag bits 0x%x", desc->flags);
    gsx_status st = check_normals("gsx_model_select_normals", desc->filter, desc->k, desc->orient, desc->toward, desc->radius_hint, desc->grid_bits, desc->max_rounds);
    if (st) return st;
    if ((st = check_selection_op("gsx_model_select_normals", desc->selection_op))) return st;
    if (desc->mode > kNormalsSelectFacing) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_normals: unknown mode %u", desc->mode);
    if (!(desc->lo <= desc->hi))  // (a NaN bound compares false)
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_normals: bounds [%g, %g] (lo <= hi, neither NaN)", (double)desc->lo, (double)desc->hi);
    float dir[3] = {0.0f, 0.0f, 0.0f};
    if (desc->mode == kNormalsSelectFacing && !nm_direction(desc->dir, dir))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_normals: dir (%g, %g, %g) is zero or not finite", (double)desc->dir[0], (double)desc->dir[1], (double)desc->dir[2]);
    if (desc->reserved != 0u || desc->reserved2[0] != 0u || desc->reserved2[1] != 0u)
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_normals: the reserved words are %u, %u, %u, not 0", desc->reserved, desc->reserved2[0], desc->reserved2[1]);
    Model* m = nullptr;
    if ((st = neighbor_model(v, "gsx_model_select_normals", key, &m))) return st;
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    gsx_normals_stats_t stats{};
    stats.grid_bits = desc->grid_bits ? desc->grid_bits : nb_auto_bits(m->n);
    if (out_stats) *out_stats = stats;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    NormalsJob job;
    if ((st = normals_job(v, m, desc->k, desc->orient, desc->toward, desc->grid_bits, false, &job))) return st;  // (before anything of the model changes)
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    if ((st = select_begin(v, m, desc->selection_op, job.nb.partials, &job.nb.sel))) return st;
    job.mode = desc->mode;
    job.flags = desc->flags;
    job.lo = desc->lo;
    job.hi = desc->hi;
    for (int a = 0; a < 3; ++a) job.dir[a] = dir[a];
    if ((st = run_normals(v, m, f, job, desc->radius_hint, desc->max_rounds, &stats))) return st;
    HIPCHK(launch_normals_select(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(m);
    uint32_t host[kNormalsWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, &stats);
    if (out_hit) *out_hit = host[kNormalsHit];
    if (out_selected) *out_selected = host[kNormalsSelected];
    if (out_stats) *out_stats = stats;
    return GSX_OK;
}

}  // extern "C"
