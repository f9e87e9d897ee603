// gsx_api_plane.cpp — C ABI of the model plane (spec/RENDER_SPEC.md section 28; kernels_plane.hip): gsx_model_fit_plane,
// gsx_model_select_plane and the host-only gsx_plane_level.  The filter is model_filter's, the rules plane_math.h's, the workspace the
// model operations' (v->extract_ws): [the words, 128 B | the planes, 16 KiB | valid, 4 KiB | the counts, 4 KiB | the sums, 128 B | the
// select's partials, 64 KiB | the participant bits, 1 bit a Gaussian | the moments' partials, 64 B a workgroup].  The host looks at
// the device once for the counts and once a moments pass; the solve between the passes is plane_math.h's, in double.
#include "gsx_state.h"
#include "neighbors_host.h"
#include "plane_math.h"

using namespace gsx;

namespace {

static_assert(sizeof(gsx_plane_t) == 16 && sizeof(gsx_plane_fit_desc) == 64 && sizeof(gsx_plane_fit_t) == 208 && sizeof(gsx_plane_select_desc) == 48, "spec section 28's layouts");
static_assert(sizeof(Plane) == sizeof(gsx_plane_t) && sizeof(float4) == sizeof(gsx_plane_t), "a plane is four floats everywhere");
static_assert(GSX_PLANE_MAX_CANDIDATES == kPlaneMaxCandidates && GSX_PLANE_MAX_REFINE == kPlaneMaxRefine && GSX_PLANE_NONE == kPlaneNone, "plane_math.h restates the limits");
static_assert(GSX_PLANE_SAMPLE_TRIPLES == kPlaneSampleTriples && GSX_PLANE_SAMPLE_NORMALS == kPlaneSampleNormals && GSX_PLANE_SAMPLE_CALLER == kPlaneSampleCaller, "the kernels' samples");

// The workspace of a model of n Gaussians; returns its bytes.
size_t plane_ws(char* ws, uint64_t n, PlaneJob* job) {
    WsCursor c{ws, 0};
    job->words = c.take<uint32_t>(4 * kPlaneWords);
    job->planes = c.take<float4>(16 * kPlaneMaxCandidates);
    job->valid = c.take<uint32_t>(4 * kPlaneMaxCandidates);
    job->counts = c.take<uint32_t>(4 * kPlaneMaxCandidates);
    job->sums = c.take<double>(8 * kPlaneSumDoubles);
    job->sel.partials = c.take<uint32_t>(4 * kSelectPartialWords * (size_t)kPropMaxGroups);
    job->participants = c.take<uint32_t>(4 * (size_t)((n + 31u) / 32u));
    job->partials = c.take<double>(8 * kPlanePartialDoubles * (size_t)extract_groups(n));
    return c.at;
}

bool has_kept_normals(const Model* m) { return m->normals.p && m->normals_kept.count == m->n; }

gsx_status no_kept_normals(const char* fn, const char* key, const char* why) {
    return fail(GSX_ERR_INVALID_ARG, "%s: %s, and model '%s' has no kept normals (gsx_model_normals_keep first; an upload, an import, a transform or a pod kind change drops them)", fn,
                why, key);
}

// The job of a call in the workspace (grown if need be: the only step that can fail for memory); n > 0.
gsx_status plane_job(gsx_viewer* v, const Model* m, float min_cos, bool normals, PlaneJob* job) {
    const gsx_status st = place_job(v, job, [&](char* ws, PlaneJob* j) { return plane_ws(ws, m->n, j); });
    if (st) return st;
    job->pc = extract_planes(m, false).pc;
    if (normals) {
        job->normals = m->normals.as<float>();
        job->variation = job->normals + 3 * (size_t)m->n;
    }
    job->min_cos = min_cos;
    return GSX_OK;
}

float4 as_float4(const Plane& pl) { return make_float4(pl.n[0], pl.n[1], pl.n[2], pl.offset); }
gsx_plane_t as_public(const Plane& pl) { return gsx_plane_t{{pl.n[0], pl.n[1], pl.n[2]}, pl.offset}; }

// One moments pass over the inliers of `pl`, waited for: its sums into `s`.
gsx_status moments_pass(gsx_viewer* v, uint64_t n, uint32_t pass, const Plane& pl, const PlaneJob& job, PlaneSums* s) {
    HIPCHK(launch_plane_moments(v->stream, n, pass, as_float4(pl), job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    double a[kPlaneSumDoubles];
    HIPCHK(gsx::op::Memcpy(a, job.sums, sizeof a, hipMemcpyDeviceToHost));
    if (pass == 0u) {
        s->count = a[0];
        for (int k = 0; k < 3; ++k) s->sum_p[k] = a[1 + k];
        s->sum_r2 = a[4];
    } else {
        for (int k = 0; k < 6; ++k) s->scatter[k] = a[8 + k];
    }
    return GSX_OK;
}

}  // namespace

extern "C" {

void gsx_plane_fit_desc_default(gsx_plane_fit_desc* d) {
    if (!d) return;
    *d = gsx_plane_fit_desc{};
    d->sample = GSX_PLANE_SAMPLE_TRIPLES;
    d->n_candidates = 256u;
    d->refine_iters = 2u;
    d->orient = GSX_NORMALS_ORIENT_CANONICAL;
}

void gsx_plane_select_desc_default(gsx_plane_select_desc* d) {
    if (!d) return;
    *d = gsx_plane_select_desc{};
    d->plane.normal[2] = 1.0f;
    d->selection_op = GSX_SELECTION_SET;
}

gsx_status gsx_model_fit_plane(gsx_viewer* v, const char* key, const gsx_plane_fit_desc* desc, const gsx_plane_t* candidates, gsx_plane_t* out_candidates,
                               uint32_t* out_counts, gsx_plane_fit_t* out) {
    const char* fn = "gsx_model_fit_plane";
    if (!v || !key || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, desc->filter);
    if (desc->flags & ~(uint32_t)GSX_EXTRACT_INVERT) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", fn, desc->flags);
    if (desc->sample > kPlaneSampleCaller) return fail(GSX_ERR_INVALID_ARG, "%s: unknown sample %u", fn, desc->sample);
    if (desc->n_candidates < 1u || desc->n_candidates > kPlaneMaxCandidates)
        return fail(GSX_ERR_INVALID_ARG, "%s: n_candidates %u is not in 1 .. %u", fn, desc->n_candidates, kPlaneMaxCandidates);
    if (!(nb_finite(desc->tolerance) && desc->tolerance >= 0.0f)) return fail(GSX_ERR_INVALID_ARG, "%s: the tolerance %g is negative or not finite", fn, (double)desc->tolerance);
    if (!(desc->min_cos >= 0.0f && desc->min_cos <= 1.0f)) return fail(GSX_ERR_INVALID_ARG, "%s: min_cos %g is not in [0, 1] (0: off)", fn, (double)desc->min_cos);
    if (desc->refine_iters > kPlaneMaxRefine) return fail(GSX_ERR_INVALID_ARG, "%s: refine_iters %u is above %u", fn, desc->refine_iters, kPlaneMaxRefine);
    if (desc->orient > kNormalsOrientToward) return fail(GSX_ERR_INVALID_ARG, "%s: unknown orient %u", fn, desc->orient);
    if (desc->orient == kNormalsOrientToward && !pl_finite3(desc->toward[0], desc->toward[1], desc->toward[2]))
        return fail(GSX_ERR_INVALID_ARG, "%s: toward (%g, %g, %g) is not finite", fn, (double)desc->toward[0], (double)desc->toward[1], (double)desc->toward[2]);
    if (desc->sample == kPlaneSampleCaller && !candidates) return fail(GSX_ERR_INVALID_ARG, "%s: GSX_PLANE_SAMPLE_CALLER without candidates", fn);
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u || desc->reserved[2] != 0u)
        return fail(GSX_ERR_INVALID_ARG, "%s: the reserved words are %u, %u, %u, not 0", fn, desc->reserved[0], desc->reserved[1], desc->reserved[2]);
    Model* m = nullptr;
    gsx_status st = neighbor_model(v, fn, key, &m);
    if (st) return st;
    const bool normals = desc->min_cos > 0.0f || desc->sample == kPlaneSampleNormals;
    if (normals && !has_kept_normals(m)) return no_kept_normals(fn, key, desc->min_cos > 0.0f ? "min_cos is above 0" : "the sample is GSX_PLANE_SAMPLE_NORMALS");
    const uint32_t H = desc->n_candidates;
    *out = gsx_plane_fit_t{};
    out->winner = kPlaneNone;
    out->degenerate = 1u;
    if (out_candidates) for (uint32_t h = 0; h < H; ++h) out_candidates[h] = gsx_plane_t{};
    if (out_counts) for (uint32_t h = 0; h < H; ++h) out_counts[h] = 0u;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    PlaneJob job;
    if ((st = plane_job(v, m, desc->min_cos, normals, &job))) return st;
    job.tolerance = desc->tolerance;
    job.sample = desc->sample;
    job.n_candidates = H;
    job.seed = desc->seed;
    const ModelFilter f = model_filter(m, desc->filter, (desc->flags & GSX_EXTRACT_INVERT) != 0u);
    HIPCHK(gsx::op::MemsetAsync(job.words, 0, 4 * kPlaneWords, v->stream));
    HIPCHK(gsx::op::MemsetAsync(job.counts, 0, 4 * kPlaneMaxCandidates, v->stream));
    if (desc->sample == kPlaneSampleCaller) HIPCHK(gsx::op::MemcpyAsync(job.planes, candidates, 16 * (size_t)H, hipMemcpyHostToDevice, v->stream));
    HIPCHK(launch_plane_participants(v->stream, n, f, job));
    HIPCHK(launch_plane_candidates(v->stream, n, job));
    HIPCHK(launch_plane_score(v->stream, n, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    uint32_t words[kPlaneWords];
    HIPCHK(gsx::op::Memcpy(words, job.words, sizeof words, hipMemcpyDeviceToHost));
    std::vector<Plane> planes(H);
    std::vector<uint32_t> valid(H), counts(H);
    HIPCHK(gsx::op::Memcpy(planes.data(), job.planes, 16 * (size_t)H, hipMemcpyDeviceToHost));
    HIPCHK(gsx::op::Memcpy(valid.data(), job.valid, 4 * (size_t)H, hipMemcpyDeviceToHost));
    HIPCHK(gsx::op::Memcpy(counts.data(), job.counts, 4 * (size_t)H, hipMemcpyDeviceToHost));
    out->count = words[kPlaneCount];
    out->n_nonfinite = words[kPlaneNonfinite];
    for (uint32_t h = 0; h < H; ++h) {
        if (!valid[h]) planes[h] = Plane{{0.0f, 0.0f, 0.0f}, 0.0f};  // (as it is reported; it was scored with a NaN offset: 0 inliers)
        else out->n_valid += 1u;
        if (out_candidates) out_candidates[h] = as_public(planes[h]);
        if (out_counts) out_counts[h] = counts[h];
    }
    const uint32_t winner = pl_winner(counts.data(), valid.data(), H);
    out->winner = winner;
    if (winner == kPlaneNone) return GSX_OK;
    out->candidate_inliers = counts[winner];
    if (counts[winner] < kPlaneMinInliers) return GSX_OK;
    out->degenerate = 0u;
    Plane plane = planes[winner];
    out->candidate = as_public(plane);
    out->plane = out->candidate;
    out->n_inliers = counts[winner];
    if (desc->refine_iters == 0u) return GSX_OK;
    // Refinement: `plane` has out->n_inliers inliers, summed in `sums` (pass 0).  A round: the scatter about their centre, the fit, the
    // fit's own pass 0 (its recount, its sum p for the next round, its sum r^2).  Fewer inliers, or no fit: the plane before stays.
    PlaneSums sums;
    if ((st = moments_pass(v, n, 0u, plane, job, &sums))) return st;
    for (uint32_t round = 0; round < desc->refine_iters; ++round) {
        if ((st = moments_pass(v, n, 1u, plane, job, &sums))) return st;
        const PlaneFit fit = pl_solve(sums, desc->orient, desc->toward);
        if (!fit.ok) break;
        PlaneSums next;
        if ((st = moments_pass(v, n, 0u, fit.plane, job, &next))) return st;
        if (next.count < (double)out->n_inliers) break;
        out->plane = as_public(fit.plane);
        out->n_inliers = (uint64_t)next.count;
        out->refine_done = round + 1u;
        for (int k = 0; k < 3; ++k) {
            out->centroid[k] = fit.centre[k];
            out->eigenvalues[k] = fit.eigenvalues[k];
            out->sums[k] = sums.sum_p[k];
        }
        for (int k = 0; k < 6; ++k) out->sums[3 + k] = sums.scatter[k];
        out->sums[9] = next.sum_r2;
        out->rms = next.count > 0.0 ? sqrt(next.sum_r2 / next.count) : 0.0;
        plane = fit.plane;
        sums = next;
    }
    return GSX_OK;
}

gsx_status gsx_model_select_plane(gsx_viewer* v, const char* key, const gsx_plane_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected) {
    const char* fn = "gsx_model_select_plane";
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "%s: null argument", fn);
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, desc->filter);
    gsx_status st = check_selection_op(fn, desc->selection_op);
    if (st) return st;
    const Plane pl{{desc->plane.normal[0], desc->plane.normal[1], desc->plane.normal[2]}, desc->plane.offset};
    if (!pl_caller_ok(pl))
        return fail(GSX_ERR_INVALID_ARG, "%s: the plane (%g, %g, %g; %g) has a component that is not finite, or a zero normal", fn, (double)pl.n[0], (double)pl.n[1], (double)pl.n[2],
                    (double)pl.offset);
    if (!(desc->lo <= desc->hi))  // (a NaN bound compares false)
        return fail(GSX_ERR_INVALID_ARG, "%s: bounds [%g, %g] (lo <= hi, neither NaN)", fn, (double)desc->lo, (double)desc->hi);
    if (!(desc->min_cos >= 0.0f && desc->min_cos <= 1.0f)) return fail(GSX_ERR_INVALID_ARG, "%s: min_cos %g is not in [0, 1] (0: off)", fn, (double)desc->min_cos);
    if (desc->reserved[0] != 0u || desc->reserved[1] != 0u || desc->reserved[2] != 0u)
        return fail(GSX_ERR_INVALID_ARG, "%s: the reserved words are %u, %u, %u, not 0", fn, desc->reserved[0], desc->reserved[1], desc->reserved[2]);
    Model* m = nullptr;
    if ((st = neighbor_model(v, fn, key, &m))) return st;
    if (desc->min_cos > 0.0f && !has_kept_normals(m)) return no_kept_normals(fn, key, "min_cos is above 0");
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    PlaneJob job;
    if ((st = plane_job(v, m, desc->min_cos, desc->min_cos > 0.0f, &job))) return st;  // (before anything of the model changes)
    job.lo = desc->lo;
    job.hi = desc->hi;
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    if ((st = select_begin(v, m, desc->selection_op, job.sel.partials, &job.sel))) return st;
    HIPCHK(launch_plane_select(v->stream, n, f, as_float4(pl), job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(m);
    uint32_t words[kPlaneWords];
    HIPCHK(gsx::op::Memcpy(words, job.words, sizeof words, hipMemcpyDeviceToHost));
    if (out_hit) *out_hit = words[kPlaneHit];
    if (out_selected) *out_selected = words[kPlaneSelected];
    return GSX_OK;
}

gsx_status gsx_plane_level(const gsx_plane_t* plane, const float up[3], float quat_xyzw[4], float pos[3]) {
    if (!plane || !up || !quat_xyzw || !pos) return fail(GSX_ERR_INVALID_ARG, "gsx_plane_level: null argument");
    double q[4], p[3];
    if (!pl_level(Plane{{plane->normal[0], plane->normal[1], plane->normal[2]}, plane->offset}, up, q, p))
        return fail(GSX_ERR_INVALID_ARG, "gsx_plane_level: the plane or up has a component that is not finite, or the normal or up is zero");
    for (int k = 0; k < 4; ++k) quat_xyzw[k] = (float)q[k];
    for (int k = 0; k < 3; ++k) pos[k] = (float)p[k];
    return GSX_OK;
}

}  // extern "C"
