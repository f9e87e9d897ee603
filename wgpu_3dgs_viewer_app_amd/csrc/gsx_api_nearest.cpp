// gsx_api_nearest.cpp — C ABI of the nearest search across models (spec/RENDER_SPEC.md section 23; kernels_nearest.hip):
// gsx_model_nearest, gsx_model_select_nearest and gsx_model_align_step, and section 27's gsx_model_align_plane_step (the solve
// align_plane_math.h's, its sums and partials behind the workspace below, for that call alone).  The filters are model_filter's, the grid section 18's
// (neighbors_host.h) over the TARGETS, rebuilt once a round at the round's radius, the rules nearest_math.h's and knn_math.h's, the
// solve align_math.h's, the workspace the model operations' (v->extract_ws): the grid's regions for the targets, then [the words, 128
// B | the align sums, 256 B | the partials, 128 B a workgroup of the source | the box, its partials and histogram | the select's
// partials | the source's participant and transfer bits | index and d2, 4 B a source Gaussian each | two lists, 16 B a source
// Gaussian each].  The host looks at the device once for the box (participants_box) and the first list's length and once a round
// for the unresolved count; the rounds' schedule is radius_search.h's.
#include "gsx_state.h"
#include "align_math.h"
#include "align_plane_math.h"
#include "nearest_math.h"
#include "neighbors_host.h"
#include "radius_search.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_nearest_desc) == 80 && sizeof(gsx_nearest_stats_t) == 136 && sizeof(gsx_nearest_select_desc) == 96, "spec section 23's layouts");
static_assert(sizeof(gsx_align_desc) == 88 && sizeof(gsx_align_step_t) == 272, "spec section 23's layouts");
static_assert(sizeof(gsx_align_plane_desc) == 96 && sizeof(gsx_align_plane_step_t) == 568, "spec section 27's layouts");
static_assert(GSX_NEAREST_NONE == kNearestNone && GSX_NEAREST_MODEL_TRANSFORMS == kNearestModelTransforms, "nearest_math.h restates them");
static_assert(GSX_NEAREST_SELECT_RANGE == kNearestSelectRange && GSX_NEAREST_SELECT_TRANSFER == kNearestSelectTransfer, "the kernels' modes");

// The workspace of a source of n Gaussians against targets of n_dst under a table of 2^bits buckets; returns its bytes.
size_t nearest_ws(char* ws, uint64_t n, uint64_t n_dst, uint32_t bits, NearestJob* job) {
    WsCursor c{ws, neighbor_ws(ws, n_dst, bits, &job->nb)};
    const size_t groups = (size_t)extract_groups(n), bit_words = (size_t)((n + 31u) / 32u);
    job->words = c.take<uint32_t>(4 * kNearestWords);
    job->align = c.take<double>(8 * kNearestAlignDoubles);
    job->partials = c.take<double>(8 * kNearestPartialDoubles * groups);
    job->box = take_box(c);
    job->sel.partials = c.take<uint32_t>(4 * kSelectPartialWords * groups);
    job->participants = c.take<uint32_t>(4 * bit_words);
    job->transfer = c.take<uint32_t>(4 * bit_words);
    job->out_index = c.take<uint32_t>(4 * (size_t)n);
    job->out_d2 = c.take<float>(4 * (size_t)n);
    job->list[0] = c.take<uint4>(16 * (size_t)n);
    job->list[1] = c.take<uint4>(16 * (size_t)n);
    return c.at;
}

// what the three calls check about a gsx_nearest_desc
gsx_status check_nearest(const char* fn, const gsx_nearest_desc& d) {
    if ((d.src_filter | d.dst_filter) & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x / 0x%x", fn, d.src_filter, d.dst_filter);
    if (d.flags & ~(uint32_t)GSX_NEAREST_MODEL_TRANSFORMS) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", fn, d.flags);
    if (!nearest_max_ok(d.max_distance))
        return fail(GSX_ERR_INVALID_ARG, "%s: max_distance %g is not 0 (unlimited) or finite and above 0 with a float32 square that is neither 0 nor inf", fn, (double)d.max_distance);
    if (!(d.radius_hint >= 0.0f) || (d.radius_hint > 0.0f && !nb_radius_ok(d.radius_hint)))
        return fail(GSX_ERR_INVALID_ARG, "%s: the radius hint %g is negative or NaN, or not finite, or its float32 square is 0 or inf", fn, (double)d.radius_hint);
    if (d.grid_bits > kNbMaxBits) return fail(GSX_ERR_INVALID_ARG, "%s: grid_bits %u is above %u", fn, d.grid_bits, kNbMaxBits);
    if (d.max_rounds > kKnnMaxRounds) return fail(GSX_ERR_INVALID_ARG, "%s: max_rounds %u is above %u", fn, d.max_rounds, kKnnMaxRounds);
    if (d.reserved != 0u) return fail(GSX_ERR_INVALID_ARG, "%s: reserved is %u, not 0", fn, d.reserved);
    if (!(d.flags & GSX_NEAREST_MODEL_TRANSFORMS))
        for (int k = 0; k < 12; ++k)
            if (!nb_finite(d.xform[k])) return fail(GSX_ERR_INVALID_ARG, "%s: xform[%d] is not finite", fn, k);
    return GSX_OK;
}

// bind, find both models, refuse what gsx_model_knn refuses, and the matrix the call uses
gsx_status nearest_models(gsx_viewer* v, const char* fn, const char* src_key, const char* dst_key, const gsx_nearest_desc& d, Model** src, Model** dst,
                          float xform[12]) {
    gsx_status st = neighbor_model(v, fn, src_key, src);
    if (st) return st;
    if ((st = neighbor_model(v, fn, dst_key, dst))) return st;
    if (d.flags & GSX_NEAREST_MODEL_TRANSFORMS) {
        const ModelTransform &ms = (*src)->mt, &md = (*dst)->mt;
        if (!merge_is_valid(ms.pos, ms.quat, ms.scale) || !merge_is_valid(md.pos, md.quat, md.scale))
            return fail(GSX_ERR_INVALID_ARG, "%s: a model transform has a component that is not finite, or a zero quaternion", fn);
        for (int a = 0; a < 3; ++a)
            if (md.scale[a] == 0.0f) return fail(GSX_ERR_INVALID_ARG, "%s: the scale of '%s' has a component of 0: its transform has no inverse", fn, dst_key);
        nearest_model_matrix(ms.pos, ms.quat, ms.scale, md.pos, md.quat, md.scale, xform);
        for (int k = 0; k < 12; ++k)
            if (!nb_finite(xform[k])) return fail(GSX_ERR_INVALID_ARG, "%s: the matrix between the two model transforms is not finite in float32", fn);
    } else {
        for (int k = 0; k < 12; ++k) xform[k] = d.xform[k];
    }
    return GSX_OK;
}

// The workspace (grown if need be: the only step that can fail for memory) and the job of a call; the source has n > 0 Gaussians.
// plane (nullable): the point-to-plane step's sums and partials, behind everything else and only for that call.
gsx_status nearest_job(gsx_viewer* v, const Model* src, const Model* dst, const gsx_nearest_desc& d, const float xform[12], NearestJob* job,
                       AlignPlaneJob* plane = nullptr) {
    const uint32_t bits = d.grid_bits ? d.grid_bits : nb_auto_bits(dst->n);
    const gsx_status st = place_job(v, job, [&](char* ws, NearestJob* j) {
        WsCursor c{ws, nearest_ws(ws, src->n, dst->n, bits, j)};
        if (plane) {
            plane->sums = c.take<double>(8 * kAlignPlaneDoubles);
            plane->partials = c.take<double>(8 * kAlignPlanePartialDoubles * (size_t)extract_groups(src->n));
        }
        return c.at;
    });
    if (st) return st;
    job->nb.bits = bits;
    job->nb.max_count = kNbMaxCount;
    for (int k = 0; k < 12; ++k) job->xform[k] = xform[k];
    job->cap2 = nearest_cap2(d.max_distance);
    job->n_dst = dst->n;
    job->dst_pc = dst->n ? extract_planes(dst, false).pc : nullptr;
    return GSX_OK;
}

// The whole search and the statistics, enqueued and, between rounds, waited for: index, d2 and the words are in the workspace when
// the stream reaches its end, and so are the source's participant bits.
gsx_status run_nearest(gsx_viewer* v, const Model* src, const Model* dst, const ModelFilter& fs, const ModelFilter& fd, NearestJob& job,
                       const gsx_nearest_desc& d, gsx_nearest_stats_t* stats) {
    const uint64_t n = src->n;
    HIPCHK(gsx::op::MemsetAsync(job.words, 0, 4 * kNearestWords, v->stream));
    HIPCHK(gsx::op::MemsetAsync(job.align, 0, 8 * kNearestAlignDoubles, v->stream));
    RadiusSearch s{{}, {}, 0u, d.radius_hint, 1u, d.max_distance, d.max_rounds};  // (the participants are the targets)
    gsx_status st = participants_box(v, dst, fd, job.box, [&] { return launch_nearest_map(v->stream, n, fs, extract_planes(src, false).pc, job); }, &s,
                                     &stats->targets_nonfinite);
    if (st) return st;
    uint32_t head[4];
    HIPCHK(gsx::op::Memcpy(head, job.words, sizeof head, hipMemcpyDeviceToHost));
    const uint32_t Q = head[kNearestList + 1u];
    stats->count = Q;
    stats->n_nonfinite = head[kNearestNonfinite];
    stats->targets = s.P;
    const uint4* list = job.list[1];  // the first list: k_nearest_map's
    // the targets' table and records at radius r (the fallback reads its records)
    const auto grid = [&](float r, bool final_round) {
        job.final_round = final_round ? 1u : 0u;
        return enqueue_grid_at(v, dst, fd, job.nb, r);
    };
    const auto round = [&](uint32_t i, uint32_t U, bool final_round, uint32_t* left) -> gsx_status {
        const uint32_t to = i & 1u;
        HIPCHK(gsx::op::MemsetAsync(job.words + kNearestList + to, 0, 4, v->stream));
        HIPCHK(launch_nearest_query(v->stream, n, list, U, to, job));
        if (final_round) return GSX_OK;  // what it did not find has no target within max_distance: nothing to wait for
        HIPCHK(gsx::op::StreamSynchronize(v->stream));  // the one look a round: how many are left
        HIPCHK(gsx::op::Memcpy(left, job.words + kNearestList + to, 4, hipMemcpyDeviceToHost));
        list = job.list[to];
        return GSX_OK;
    };
    const auto brute = [&](uint32_t U) -> gsx_status {
        HIPCHK(launch_nearest_brute(v->stream, n, list, U, s.P, job));
        return GSX_OK;
    };
    if (s.P && Q) {  // (without queries or targets there is no search, and first_radius stays 0)
        if ((st = radius_search<gsx_status>(s, Q, grid, round, brute))) return st;
        stats->first_radius = s.first_radius;
    }
    stats->rounds = s.rounds;
    stats->n_brute = s.n_brute;
    HIPCHK(launch_nearest_stats(v->stream, n, job));
    return GSX_OK;
}

// the words of a finished call into the caller's stats (the counts are there already)
void read_stats(const uint32_t* w, gsx_nearest_stats_t* stats) {
    double sum, sum2;
    __builtin_memcpy(&sum, w + kNearestSum, 8);
    __builtin_memcpy(&sum2, w + kNearestSum2, 8);
    stats->n_found = w[kNearestFound];
    stats->d_min = nb_from_bits(w[kNearestMin]);
    stats->d_max = nb_from_bits(w[kNearestMax]);
    stats->mean = stats->n_found ? sum / (double)stats->n_found : 0.0;
    stats->rms = stats->n_found ? sqrt(sum2 / (double)stats->n_found) : 0.0;
}

// the stats of a call before anything ran: zeros, the table and the matrix
gsx_nearest_stats_t fresh_stats(const Model* dst, const gsx_nearest_desc& d, const float xform[12]) {
    gsx_nearest_stats_t s{};
    s.grid_bits = d.grid_bits ? d.grid_bits : nb_auto_bits(dst->n);
    for (int k = 0; k < 12; ++k) s.xform[k] = xform[k];
    return s;
}

}  // namespace

extern "C" {

void gsx_nearest_desc_default(gsx_nearest_desc* d) {
    if (!d) return;
    *d = gsx_nearest_desc{};
    d->xform[0] = d->xform[5] = d->xform[10] = 1.0f;
}

gsx_status gsx_model_nearest(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_nearest_desc* desc, uint32_t* out_index, float* out_d2,
                             gsx_nearest_stats_t* out) {
    if (!v || !src_key || !dst_key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_nearest: null argument");
    gsx_status st = check_nearest("gsx_model_nearest", *desc);
    if (st) return st;
    Model *src = nullptr, *dst = nullptr;
    float xform[12];
    if ((st = nearest_models(v, "gsx_model_nearest", src_key, dst_key, *desc, &src, &dst, xform))) return st;
    *out = fresh_stats(dst, *desc, xform);
    const uint64_t n = src->n;
    if (n == 0) return GSX_OK;
    NearestJob job;
    if ((st = nearest_job(v, src, dst, *desc, xform, &job))) return st;
    if ((st = run_nearest(v, src, dst, model_filter(src, desc->src_filter, false), model_filter(dst, desc->dst_filter, false), job, *desc, out))) return st;
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t host[kNearestWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, out);
    if (out_index) HIPCHK(gsx::op::Memcpy(out_index, job.out_index, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (out_d2) HIPCHK(gsx::op::Memcpy(out_d2, job.out_d2, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_model_select_nearest(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_nearest_select_desc* desc, uint64_t* out_hit,
                                    uint64_t* out_selected, gsx_nearest_stats_t* out_stats) {
    if (!v || !src_key || !dst_key || !desc) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_nearest: null argument");
    gsx_status st = check_nearest("gsx_model_select_nearest", desc->nearest);
    if (st) return st;
    if ((st = check_selection_op("gsx_model_select_nearest", desc->selection_op))) return st;
    if (desc->mode > (uint32_t)GSX_NEAREST_SELECT_TRANSFER) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_nearest: unknown mode %u", desc->mode);
    if (desc->mode == (uint32_t)GSX_NEAREST_SELECT_RANGE ? !(desc->lo <= desc->hi) : !(desc->lo == 0.0f && desc->hi == 0.0f))  // (a NaN bound compares false)
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_nearest: bounds [%g, %g] in mode %u (range: lo <= hi, neither NaN; transfer: both 0)", (double)desc->lo,
                    (double)desc->hi, desc->mode);
    Model *src = nullptr, *dst = nullptr;
    float xform[12];
    if ((st = nearest_models(v, "gsx_model_select_nearest", src_key, dst_key, desc->nearest, &src, &dst, xform))) return st;
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    gsx_nearest_stats_t stats = fresh_stats(dst, desc->nearest, xform);
    if (out_stats) *out_stats = stats;
    const uint64_t n = src->n;
    if (n == 0) return GSX_OK;
    NearestJob job;
    if ((st = nearest_job(v, src, dst, desc->nearest, xform, &job))) return st;  // (before anything of the model changes)
    // (before has_selection changes: none selected = none pass, and no target is selected)
    const ModelFilter fs = model_filter(src, desc->nearest.src_filter, false), fd = model_filter(dst, desc->nearest.dst_filter, false);
    const bool dst_selected = dst->has_selection;
    uint32_t* sel_partials = job.sel.partials;
    if ((st = select_begin(v, src, desc->selection_op, sel_partials, &job.sel))) return st;
    job.dst_selection = dst_selected ? dst->selection.as<uint32_t>() : nullptr;
    job.mode = desc->mode;
    job.lo = desc->lo;
    job.hi = desc->hi;
    if ((st = run_nearest(v, src, dst, fs, fd, job, desc->nearest, &stats))) return st;
    if (desc->mode == (uint32_t)GSX_NEAREST_SELECT_TRANSFER) HIPCHK(launch_nearest_transfer(v->stream, n, job));
    HIPCHK(launch_nearest_select(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(src);
    uint32_t host[kNearestWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, &stats);
    if (out_hit) *out_hit = host[kNearestHit];
    if (out_selected) *out_selected = host[kNearestSelected];
    if (out_stats) *out_stats = stats;
    return GSX_OK;
}

gsx_status gsx_model_align_step(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_align_desc* desc, gsx_align_step_t* out) {
    if (!v || !src_key || !dst_key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_align_step: null argument");
    gsx_status st = check_nearest("gsx_model_align_step", desc->nearest);
    if (st) return st;
    if (desc->flags & ~(uint32_t)GSX_ALIGN_SCALE) return fail(GSX_ERR_INVALID_ARG, "gsx_model_align_step: unknown flag bits 0x%x", desc->flags);
    if (desc->reserved != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_align_step: reserved is %u, not 0", desc->reserved);
    Model *src = nullptr, *dst = nullptr;
    float xform[12];
    if ((st = nearest_models(v, "gsx_model_align_step", src_key, dst_key, desc->nearest, &src, &dst, xform))) return st;
    *out = gsx_align_step_t{};
    out->quat[3] = 1.0;
    out->scale = 1.0;
    out->degenerate = 1u;
    for (int k = 0; k < 12; ++k) out->xform_next[k] = xform[k];
    out->nearest = fresh_stats(dst, desc->nearest, xform);
    const uint64_t n = src->n;
    if (n == 0) return GSX_OK;
    NearestJob job;
    if ((st = nearest_job(v, src, dst, desc->nearest, xform, &job))) return st;
    if ((st = run_nearest(v, src, dst, model_filter(src, desc->nearest.src_filter, false), model_filter(dst, desc->nearest.dst_filter, false), job, desc->nearest,
                          &out->nearest)))
        return st;
    HIPCHK(launch_nearest_align(v->stream, n, extract_planes(src, false).pc, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t host[kNearestWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, &out->nearest);
    double a[kNearestAlignDoubles];
    HIPCHK(gsx::op::Memcpy(a, job.align, sizeof a, hipMemcpyDeviceToHost));
    AlignSums sums;
    sums.n = a[0];
    for (int k = 0; k < 3; ++k) {
        sums.sum_q[k] = a[1 + k];
        sums.sum_t[k] = a[4 + k];
    }
    for (int k = 0; k < 9; ++k) sums.H[k] = a[8 + k];
    sums.spread_q = a[17];
    sums.spread_t = a[18];
    sums.sum_d2 = a[19];
    out->n_pairs = (uint64_t)sums.n;
    out->rms_before = sums.n > 0.0 ? sqrt(sums.sum_d2 / sums.n) : 0.0;
    const AlignDelta delta = align_solve(sums, (desc->flags & GSX_ALIGN_SCALE) != 0u);
    out->degenerate = delta.degenerate ? 1u : 0u;
    if (delta.degenerate) return GSX_OK;  // (the identity and xform_next = xform are in place)
    for (int k = 0; k < 3; ++k) out->pos[k] = delta.pos[k];
    for (int k = 0; k < 4; ++k) out->quat[k] = delta.quat[k];
    out->scale = delta.scale;
    align_compose(delta, xform, out->xform_next);
    return GSX_OK;
}

gsx_status gsx_model_align_plane_step(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_align_plane_desc* desc, gsx_align_plane_step_t* out) {
    const char* fn = "gsx_model_align_plane_step";
    if (!v || !src_key || !dst_key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    gsx_status st = check_nearest(fn, desc->nearest);
    if (st) return st;
    if (desc->flags) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (none are defined)", fn, desc->flags);
    if (!(desc->max_variation >= 0.0f)) return fail(GSX_ERR_INVALID_ARG, "%s: max_variation %g is negative or NaN (0: no limit)", fn, (double)desc->max_variation);
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u)
        return fail(GSX_ERR_INVALID_ARG, "%s: the reserved words are %u, %u, not 0", fn, desc->reserved[0], desc->reserved[1]);
    Model *src = nullptr, *dst = nullptr;
    float xform[12];
    if ((st = nearest_models(v, fn, src_key, dst_key, desc->nearest, &src, &dst, xform))) return st;
    if (!dst->normals.p || dst->normals_kept.count != dst->n)
        return fail(GSX_ERR_INVALID_ARG, "%s: model '%s' has no kept normals (gsx_model_normals_keep first; an upload, an import, a transform or a pod kind change drops them)",
                    fn, dst_key);
    *out = gsx_align_plane_step_t{};
    out->quat[3] = 1.0;
    out->degenerate = 1u;
    for (int k = 0; k < 12; ++k) out->xform_next[k] = xform[k];
    out->nearest = fresh_stats(dst, desc->nearest, xform);
    const uint64_t n = src->n;
    if (n == 0) return GSX_OK;
    NearestJob job;
    AlignPlaneJob plane{};
    if ((st = nearest_job(v, src, dst, desc->nearest, xform, &job, &plane))) return st;
    plane.normals = dst->normals.as<float>();
    plane.variation = plane.normals + 3 * (size_t)dst->n;
    plane.max_variation = desc->max_variation;
    if ((st = run_nearest(v, src, dst, model_filter(src, desc->nearest.src_filter, false), model_filter(dst, desc->nearest.dst_filter, false), job, desc->nearest,
                          &out->nearest)))
        return st;
    HIPCHK(gsx::op::MemsetAsync(plane.sums, 0, 8 * kAlignPlaneDoubles, v->stream));
    HIPCHK(launch_nearest_align_plane(v->stream, n, extract_planes(src, false).pc, job, plane));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t host[kNearestWords];
    HIPCHK(gsx::op::Memcpy(host, job.words, sizeof host, hipMemcpyDeviceToHost));
    read_stats(host, &out->nearest);
    double a[kAlignPlaneDoubles];
    HIPCHK(gsx::op::Memcpy(a, plane.sums, sizeof a, hipMemcpyDeviceToHost));
    AlignPlaneSums sums;
    sums.n = a[0];
    for (int k = 0; k < 3; ++k) sums.centre[k] = align_plane_centre(a[1 + k], sums.n);
    for (uint32_t k = 0; k < kAlignPlaneTri; ++k) sums.A[k] = a[8 + k];
    for (int k = 0; k < 6; ++k) sums.b[k] = a[29 + k];
    sums.sum_e2 = a[35];
    sums.sum_d2 = a[36];
    out->n_pairs = (uint64_t)sums.n;
    out->n_unfitted = (uint64_t)a[4];
    out->rms_before = sums.n > 0.0 ? sqrt(sums.sum_d2 / sums.n) : 0.0;
    out->rms_plane_before = sums.n > 0.0 ? sqrt(sums.sum_e2 / sums.n) : 0.0;
    for (uint32_t k = 0; k < kAlignPlaneTri; ++k) out->normal_matrix[k] = sums.A[k];
    for (int k = 0; k < 6; ++k) out->rhs[k] = sums.b[k];
    const AlignPlaneDelta d = align_plane_solve(sums);
    for (int k = 0; k < 6; ++k) out->eigenvalues[k] = d.eigenvalues[k];
    for (int k = 0; k < 3; ++k) out->centre[k] = d.centre[k];
    out->rank = d.rank;
    out->degenerate = d.delta.degenerate ? 1u : 0u;
    if (d.delta.degenerate) return GSX_OK;  // (the identity and xform_next = xform are in place)
    for (int k = 0; k < 3; ++k) out->pos[k] = d.delta.pos[k];
    for (int k = 0; k < 4; ++k) out->quat[k] = d.delta.quat[k];
    align_compose(d.delta, xform, out->xform_next);
    return GSX_OK;
}

}  // extern "C"
