// neighbors_host.h — the host side that the neighbour counts (gsx_api_neighbors.cpp, spec section 18) and the clusters
// (gsx_api_clusters.cpp, section 19) share: the grid's workspace inside the model operations' (v->extract_ws), what both check about
// a desc, how both bind and find their model, and the four passes that build the grid.  The workspace:
// [result block, 128 B | 4096 histogram words | the scan's total | the workgroups' partials | the participant bits | the bucket table |
//  the scan's block sums and bases | the counts, 4 B a Gaussian | the records, 16 B a Gaussian]; a caller's own regions follow.
// Every operation on the grid (the nearest neighbours, the nearest across models and decimate too) places its job with place_job; the
// two searches by rounds (radius_search.h) take their participants' box from participants_box.
#pragma once
#include "gsx_state.h"
#include "bounds_math.h"
#include "radius_search.h"
#include "neighbors_math.h"

namespace gsx {

constexpr size_t kNbWsHist = 4 * kNbResultWords;                   // 128
constexpr size_t kNbWsTotal = kNbWsHist + 4 * (kNbMaxCount + 1u);  // 16 512
constexpr size_t kNbWsPartials = kNbWsTotal + 128;
static_assert(kNbWsHist == 128 && kNbWsPartials % 128 == 0, "the workspace regions are whole 128-byte lines");

// The regions of a workspace one after the other, whole 128-byte lines each, from `at` bytes behind `ws` (nullptr where only the
// size is asked for: the addresses are integers until the end).
struct WsCursor {
    char* ws;
    size_t at;
    template <class T>
    T* take(size_t bytes) {
        const size_t here = at;
        at += extract_pad128(bytes);
        return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(ws) + here);
    }
};

// The workspace of a model of n Gaussians under a table of 2^bits buckets; returns its bytes.
inline size_t neighbor_ws(char* ws, uint64_t n, uint32_t bits, NeighborJob* job) {
    const size_t words = size_t(1) << bits, blocks = (words + kNbScanBlock - 1u) / kNbScanBlock;
    WsCursor c{ws, 0};
    job->result = c.take<uint32_t>(kNbWsHist);
    job->hist = c.take<uint32_t>(kNbWsTotal - kNbWsHist);
    job->scan_total = c.take<uint64_t>(kNbWsPartials - kNbWsTotal);
    job->partials = c.take<uint32_t>(4 * kNbPartialWords * (size_t)extract_groups(n));
    job->participants = c.take<uint32_t>(4 * (size_t)((n + 31u) / 32u));
    job->table = c.take<uint32_t>(4 * words);
    job->scan_sums = c.take<uint32_t>(4 * blocks);
    job->scan_bases = c.take<uint32_t>(4 * blocks);
    job->counts = c.take<uint32_t>(4 * (size_t)n);
    job->records = c.take<uint4>(16 * (size_t)n);
    return c.at;
}

// A call's job in the workspace, grown if need be (the only step that can fail for memory): layout(ws, job) places the job's regions
// behind ws (nullptr: only the size is asked for) and returns their bytes.
template <class Job, class Layout>
inline gsx_status place_job(gsx_viewer* v, Job* job, Layout layout) {
    Job sized{};
    HIPCHK(v->extract_ws.ensure(layout(nullptr, &sized)));
    *job = Job{};
    layout(v->extract_ws.as<char>(), job);
    return GSX_OK;
}

// The box's three regions (gsx_internal.h: BoxWs), in this order.
inline BoxWs take_box(WsCursor& c) {
    BoxWs b;
    b.box = c.take<gsx_model_bounds_t>(sizeof(gsx_model_bounds_t));
    b.partials = c.take<BoundsPartial>(sizeof(BoundsPartial) * kBoundsMaxGroups);
    b.hist = c.take<uint32_t>(4 * 3u * kBoundsBins);
    return b;
}

// The participants' count and the extents of their box and of their box trimmed at kKnnTrimPermille, into the search that takes its
// radii from them (radius_search.h), and how many pass the filter without a finite position: gsx_model_bounds' passes, whose
// participants are the grid's (the filter and three finite coordinates), then `also()`, what the caller wants on the stream behind
// them before the search starts (its fill or map pass), then the one wait for all of it.
template <class Also>
inline gsx_status participants_box(gsx_viewer* v, const Model* m, const ModelFilter& f, const BoxWs& ws, Also also, RadiusSearch* s, uint64_t* n_nonfinite) {
    const uint64_t looked_at = f.select_none ? 0 : m->n;  // (selected Gaussians of a model without a selection: none)
    if (looked_at) HIPCHK(launch_bounds_reduce(v->stream, m->pc.as<float4>(), m->n, f, ws.partials));
    HIPCHK(launch_bounds_finish(v->stream, ws.partials, looked_at ? bounds_reduce_groups(m->n) : 0u, looked_at != 0, ws.box, ws.hist));
    if (looked_at) HIPCHK(launch_bounds_trim(v->stream, m->pc.as<float4>(), m->n, f, kKnnTrimPermille, ws.box, ws.hist));
    HIPCHK(also());
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    gsx_model_bounds_t box;
    HIPCHK(gsx::op::Memcpy(&box, ws.box, sizeof box, hipMemcpyDeviceToHost));
    s->P = (uint32_t)box.count;
    *n_nonfinite = box.n_nonfinite;
    for (int a = 0; a < 3; ++a) {
        s->ext[a] = (double)box.max[a] - (double)box.min[a];
        s->trimmed[a] = (double)box.trim_max[a] - (double)box.trim_min[a];
    }
    return GSX_OK;
}

// what the calls check about (filter, flags, radius, max_count, grid_bits)
inline gsx_status check_desc(const char* fn, uint32_t filter, uint32_t flags, float radius, uint32_t max_count, uint32_t grid_bits) {
    if (filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "%s: unknown filter bits 0x%x", fn, filter);
    if (flags) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (none are defined)", fn, flags);
    if (!nb_radius_ok(radius)) return fail(GSX_ERR_INVALID_ARG, "%s: the radius %g is not finite and above 0, or its float32 square is 0 or inf", fn, (double)radius);
    if (max_count < 1u || max_count > kNbMaxCount) return fail(GSX_ERR_INVALID_ARG, "%s: max_count %u is not in 1 .. %u", fn, max_count, kNbMaxCount);
    if (grid_bits > kNbMaxBits) return fail(GSX_ERR_INVALID_ARG, "%s: grid_bits %u is above %u", fn, grid_bits, kNbMaxBits);
    return GSX_OK;
}

// bind, find, refuse what gsx_model_extract refuses
inline gsx_status neighbor_model(gsx_viewer* v, const char* fn, const char* key, Model** out) {
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes
    if (st) return st;
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "%s: no model '%s'", fn, key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "%s: the viewer has a communicator (call it before gsx_viewer_comm_init, or on one GPU)", fn);
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "%s: model '%s' is a shard of a multi-GPU frame", fn, key);
    *out = m;
    return GSX_OK;
}

// The grid's passes, enqueued: the participant bits, the table (bucket ends) and the records in bucket order are in the workspace
// when the stream reaches its end; the counts are 0.
inline gsx_status enqueue_grid(gsx_viewer* v, const Model* m, const ModelFilter& f, const NeighborJob& job) {
    const uint4* pc = extract_planes(m, false).pc;
    HIPCHK(gsx::op::MemsetAsync(job.result, 0, kNbWsTotal + 8, v->stream));  // the result block, the bins, the scan's total
    HIPCHK(gsx::op::MemsetAsync(job.table, 0, 4 * (size_t(1) << job.bits), v->stream));
    HIPCHK(launch_neighbors_reduce(v->stream, m->n, f, pc, job));
    HIPCHK(launch_neighbors_cell(v->stream, m->n, f, pc, job));
    HIPCHK(launch_neighbors_scan(v->stream, job));
    HIPCHK(launch_neighbors_scatter(v->stream, m->n, pc, job));
    return GSX_OK;
}
// the same at the radius of a search's round
inline gsx_status enqueue_grid_at(gsx_viewer* v, const Model* m, const ModelFilter& f, NeighborJob& job, float radius) {
    const NbGrid g = nb_grid(radius);
    job.r2 = g.r2;
    job.inv_h = g.inv_h;
    return enqueue_grid(v, m, f, job);
}

}  // namespace gsx
