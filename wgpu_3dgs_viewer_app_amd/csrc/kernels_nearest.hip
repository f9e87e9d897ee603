// kernels_nearest.hip — the nearest search across models for gfx950 (spec/RENDER_SPEC.md §23, "Model nearest (across models)"):
// gsx_model_nearest, gsx_model_select_nearest, gsx_model_align_step and §27's gsx_model_align_plane_step.  The grid is section 18's, built over the TARGETS
// (kernels_neighbors.hip, once a round); the rules are nearest_math.h's and knn_math.h's, the rounds' schedule radius_search.h's (called
// by gsx_api_nearest.cpp).  The queries are the SOURCE's Gaussians,
// mapped by a 3x4 matrix: they are no members of the grid and may lie outside its box (neighbors_math.h: nb_cell_signed).  "n" is
// the source's length everywhere.
//   k_nearest_map       index order over the source: the participant bits (the filter, a finite stored position, a finite mapped
//                       position q), out_index / out_d2 = none / +inf, and one 16-byte entry (q, source index) a participant,
//                       appended to the first list with one returning add a wave (wave_reduce.h: wave_append); the list's order is free;
//   k_nearest_query     one lane per entry, k_knn_query's shape with ONE best (d2, index) pair in registers: the 27 cells around the
//                       query's signed cell; a record is a candidate if d2 <= min(r2, cap2) and its own cell IS the visited cell, and
//                       replaces the best if it has the smaller d2 or the same d2 and the smaller index.  There is no early end at
//                       d2 = 0: a smaller index may still tie.  Proven iff the best d2 is within the reach: every tie is then in the
//                       27 cells.  A lane that is not proven appends its entry to the next list, unless the round is final (r2 >=
//                       cap2): then nothing is in reach and the row stays "none";
//   k_nearest_brute     the exact fallback, one workgroup per entry: 256 lanes stride over all records, each keeps the least key
//                       (d2 bits << 32) | index of the records within cap2, and a wave and workgroup minimum picks value and
//                       tie-break in one compare;
//   k_nearest_stats     index order: the found queries' count, the least and largest sqrtf(d2), the double sums of sqrtf(d2) and of
//                       d2; one partial a workgroup, combined by one workgroup in index order: no atomics, the same bits every call;
//   k_nearest_transfer  the queries whose target is selected, as bits, before the select writes (source and targets may be one model);
//   k_nearest_select    k_knn_select's shape with the two hit rules;
//   k_nearest_align     index order, twice: the pairs' count and the sums of q and t, then about the float32 means the products of
//                       the float32 differences, taken and summed in double; partials and finish as the statistics';
//   k_nearest_align_plane  gsx_model_align_plane_step (spec §27): the same two passes over the found pairs whose target has a kept,
//                       fitted normal: the 6x6 normal matrix, its right-hand side and the two residual sums, with partials of its own.
// Every loop is bounded by n, 27, a bucket's or a list's length; no lane waits for another's progress; no kernel caps its grid.
// Built with -ffp-contract=off.  Bounds: a source index is checked against n before a store by it, a target index against the
// targets' length before a load by it, a list slot against n (a list's capacity), a bucket's end against the target count.
#include "gsx_internal.h"
#include "nearest_math.h"
#include "neighbors_grid.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
constexpr float kNearestInf = __builtin_huge_valf();

struct NearestStatsPartial {
    uint32_t count;
    float mn, mx;
    double sum, sum2;
};
__device__ inline NearestStatsPartial nearest_combine_stats(uint32_t count, float mn, float mx, double sum, double sum2) {
    return group_fold(NearestStatsPartial{wave_sum(count), wave_min(mn), wave_max(mx), wave_sum(sum), wave_sum(sum2)},
                      [](NearestStatsPartial a, const NearestStatsPartial& b) {
                          return NearestStatsPartial{a.count + b.count, fminf(a.mn, b.mn), fmaxf(a.mx, b.mx), a.sum + b.sum, a.sum2 + b.sum2};
                      });
}
// (DoubleTerms<T>, combine_terms: wave_reduce.h)
constexpr uint32_t kAlignTerms = 12;  // pass 0 uses 7 of them: n, sum q, sum t; pass 1 all: H, the two spreads, sum d2
using AlignPartial = DoubleTerms<kAlignTerms>;
__device__ inline AlignPartial nearest_combine_align(AlignPartial p) { return combine_terms(p); }
constexpr uint32_t kAlignPlaneTerms = 29;  // pass 0 uses 5 of them: pairs, sum q, left out; pass 1 all: A (21), b (6), sum e^2, sum d2
using AlignPlanePartial = DoubleTerms<kAlignPlaneTerms>;
static_assert(kAlignPlaneTerms <= kAlignPlanePartialDoubles && 8u + kAlignPlaneTerms <= kAlignPlaneDoubles, "the partials and the sums hold every term");
// the mapped position of a stored one
__device__ inline void nearest_map(const NearestJob& job, const uint4& e, float& qx, float& qy, float& qz) {
    const float x = __uint_as_float(e.x), y = __uint_as_float(e.y), z = __uint_as_float(e.z);
    qx = nearest_map_row(job.xform + 0, x, y, z);
    qy = nearest_map_row(job.xform + 4, x, y, z);
    qz = nearest_map_row(job.xform + 8, x, y, z);
}
}  // namespace

__global__ __launch_bounds__(256) void k_nearest_map(uint64_t n, ModelFilter f, const uint4* __restrict__ pc, NearestJob job) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    uint32_t nonfinite = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool part = prop_keep(f, n, i, t);  // (every lane of the wave makes the call: a ballot inside)
        uint4 entry = make_uint4(0u, 0u, 0u, 0u);
        if (part) {
            const uint4 e = pc[i];
            float qx, qy, qz;
            nearest_map(job, e, qx, qy, qz);
            part = nb_finite(__uint_as_float(e.x)) && nb_finite(__uint_as_float(e.y)) && nb_finite(__uint_as_float(e.z)) && nb_finite(qx) && nb_finite(qy) &&
                   nb_finite(qz);
            if (!part) nonfinite += 1u;
            entry = make_uint4(__float_as_uint(qx), __float_as_uint(qy), __float_as_uint(qz), (uint32_t)i);
        }
        const unsigned long long part64 = __ballot(part);
        if (i < n) {
            job.out_index[i] = kNearestNone;
            job.out_d2[i] = kNearestInf;
            if ((lane & 31u) == 0u) job.participants[i >> 5] = (uint32_t)(part64 >> lane);  // (bits at and above n are clear)
        }
        wave_append(part, entry, job.list[1], job.words + kNearestList + 1u, n);
    }
    nonfinite = wave_sum(nonfinite);
    if (lane == 0u && nonfinite) atomicAdd(job.words + kNearestNonfinite, nonfinite);  // (an integer sum: the same in any order)
}

__global__ __launch_bounds__(256) void k_nearest_query(uint64_t n, const uint4* __restrict__ src, uint32_t count, uint4* __restrict__ next,
                                                       uint32_t* __restrict__ next_count, NearestJob job) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool unresolved = false;
    uint4 self = make_uint4(0u, 0u, 0u, 0u);
    if (p < count) {
        const NbFrame g = nb_frame(job.nb);
        const float reach2 = nearest_reach2(job.nb.r2, job.cap2);
        self = src[p];
        const float qx = __uint_as_float(self.x), qy = __uint_as_float(self.y), qz = __uint_as_float(self.z);
        const int32_t cx = nb_cell_signed(qx, g.ox, g.inv_h), cy = nb_cell_signed(qy, g.oy, g.inv_h), cz = nb_cell_signed(qz, g.oz, g.inv_h);
        float best = kNearestInf;
        uint32_t best_index = kNearestNone;
        if (cx > -2 && cy > -2 && cz > -2) {  // (-2: no target is within the radius on that axis)
            // (a cell of -1 wraps to 0xFFFFFFFF: the walk drops it and its lower neighbour and visits cell 0)
            nb_walk(g, job.nb, NbCell{(uint32_t)cx, (uint32_t)cy, (uint32_t)cz}, [&](const uint4& r, const NbVisit& v) {
                const float d2 = nb_d2(qx, qy, qz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z));
                if (d2 <= reach2 && nearest_better(d2, r.w, best, best_index) && v.holds(r)) {
                    best = d2;
                    best_index = r.w;
                }
                return true;
            });
        }
        if (best <= reach2) {
            if (self.w < n) {  // (always: the map wrote an index below n)
                job.out_index[self.w] = best_index;
                job.out_d2[self.w] = best;
            }
        } else {
            unresolved = job.final_round == 0u;
        }
    }
    wave_append(unresolved, self, next, next_count, n);  // (every lane arrives here)
}

__global__ __launch_bounds__(256) void k_nearest_brute(uint64_t n, const uint4* __restrict__ src, uint32_t total, NearestJob job) {
    const uint32_t t = threadIdx.x;
    const uint4 self = src[blockIdx.x];
    const float qx = __uint_as_float(self.x), qy = __uint_as_float(self.y), qz = __uint_as_float(self.z);
    const uint32_t records = min(total, job.nb.result[kNbCount]);
    const float cap2 = job.cap2;
    uint64_t key = ((uint64_t)__float_as_uint(kNearestInf) << 32) | kNearestNone;
#pragma unroll 1
    for (uint32_t q = t; q < records; q += 256u) {
        const uint4 r = job.nb.records[q];
        const float d2 = nb_d2(qx, qy, qz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z));
        // (d2 is +0 or above, never NaN: the bits order as the values do; the index breaks ties)
        const uint64_t mine = ((uint64_t)__float_as_uint(d2) << 32) | r.w;
        if (d2 <= cap2 && mine < key) key = mine;
    }
    key = group_fold(wave_min(key), [](uint64_t a, uint64_t b) { return b < a ? b : a; });
    if (t == 0u && (uint32_t)key != kNearestNone && self.w < n) {
        job.out_index[self.w] = (uint32_t)key;
        job.out_d2[self.w] = __uint_as_float((uint32_t)(key >> 32));
    }
}

__global__ __launch_bounds__(256) void k_nearest_stats(uint64_t n, NearestJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    uint32_t count = 0;
    float mn = kNearestInf, mx = -kNearestInf;
    double sum = 0.0, sum2 = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        if (job.out_index[i] == kNearestNone) continue;
        const float d2 = job.out_d2[i], d = sqrtf(d2);
        count += 1u;
        mn = fminf(mn, d);
        mx = fmaxf(mx, d);
        sum += (double)d;
        sum2 += (double)d2;
    }
    const NearestStatsPartial p = nearest_combine_stats(count, mn, mx, sum, sum2);
    if (t == 0u) {
        double* out = job.partials + (size_t)blockIdx.x * kNearestPartialDoubles;
        uint32_t* w = reinterpret_cast<uint32_t*>(out);
        w[0] = p.count; w[1] = __float_as_uint(p.mn); w[2] = __float_as_uint(p.mx);
        out[2] = p.sum;
        out[3] = p.sum2;
    }
}

// One workgroup: the partials in index order.
__global__ __launch_bounds__(256) void k_nearest_stats_finish(uint32_t n_partials, NearestJob job) {
    const uint32_t t = threadIdx.x;
    uint32_t count = 0;
    float mn = kNearestInf, mx = -kNearestInf;
    double sum = 0.0, sum2 = 0.0;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const double* in = job.partials + (size_t)j * kNearestPartialDoubles;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(in);
        count += w[0];
        mn = fminf(mn, __uint_as_float(w[1]));
        mx = fmaxf(mx, __uint_as_float(w[2]));
        sum += in[2];
        sum2 += in[3];
    }
    const NearestStatsPartial p = nearest_combine_stats(count, mn, mx, sum, sum2);
    if (t != 0u) return;
    uint32_t* w = job.words;
    w[kNearestFound] = p.count;
    w[kNearestMin] = p.count ? __float_as_uint(p.mn) : 0u;
    w[kNearestMax] = p.count ? __float_as_uint(p.mx) : 0u;
    *reinterpret_cast<double*>(w + kNearestSum) = p.sum;  // (even word offsets of a 128-byte aligned block)
    *reinterpret_cast<double*>(w + kNearestSum2) = p.sum2;
}

__global__ __launch_bounds__(256) void k_nearest_transfer(uint64_t n, NearestJob job) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool on = false;
        if (i < n && job.dst_selection) {
            const uint32_t target = job.out_index[i];
            if (target != kNearestNone && target < job.n_dst) on = (job.dst_selection[target >> 5] >> (target & 31u)) & 1u;
        }
        const unsigned long long on64 = __ballot(on);
        if (i < n && (lane & 31u) == 0u) job.transfer[i >> 5] = (uint32_t)(on64 >> lane);
    }
}

__global__ __launch_bounds__(256) void k_nearest_select(uint64_t n, NearestJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const bool transfer = job.mode == kNearestSelectTransfer;
    SelectCounts counts;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool hit = false;
        if (i < n) {
            if (transfer) {
                hit = (job.transfer[i >> 5] >> (t & 31u)) & 1u;
            } else if ((job.participants[i >> 5] >> (t & 31u)) & 1u) {
                const float d = sqrtf(job.out_d2[i]);  // (+inf where nothing was found: hi = +inf takes it)
                hit = d >= job.lo && d <= job.hi;
            }
        }
        select_write(job.sel, hit, i, n, counts);
    }
    select_store_partial(job.sel, counts);
}

// pass 0: the pairs' count and the sums of q and t; pass 1: about the means of pass 0 rounded to float32, the products of the float32
// differences, in double: H (row: q's axis), sum |q - qm|^2, sum |t - tm|^2, and the sum of d2
__global__ __launch_bounds__(256) void k_nearest_align(uint64_t n, uint32_t pass, const uint4* __restrict__ pc, NearestJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    float qm[3] = {0.0f, 0.0f, 0.0f}, tm[3] = {0.0f, 0.0f, 0.0f};
    if (pass) {
        const double pairs = job.align[0];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            qm[a] = pairs > 0.0 ? (float)(job.align[1 + a] / pairs) : 0.0f;
            tm[a] = pairs > 0.0 ? (float)(job.align[4 + a] / pairs) : 0.0f;
        }
    }
    AlignPartial p;
#pragma unroll
    for (uint32_t k = 0; k < kAlignTerms; ++k) p.v[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        const uint32_t target = job.out_index[i];
        if (target == kNearestNone || target >= job.n_dst) continue;
        float q[3];
        nearest_map(job, pc[i], q[0], q[1], q[2]);
        const uint4 e = job.dst_pc[target];
        const float tt[3] = {__uint_as_float(e.x), __uint_as_float(e.y), __uint_as_float(e.z)};
        if (pass == 0u) {
            p.v[0] += 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p.v[1 + a] += (double)q[a];
                p.v[4 + a] += (double)tt[a];
            }
        } else {
            double dq[3], dt[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                dq[a] = (double)(q[a] - qm[a]);
                dt[a] = (double)(tt[a] - tm[a]);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) p.v[3 * a + b] += dq[a] * dt[b];
            }
            p.v[9] += (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
            p.v[10] += (dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2];
            p.v[11] += (double)job.out_d2[i];
        }
    }
    p = nearest_combine_align(p);
    if (t == 0u) {
        double* out = job.partials + (size_t)blockIdx.x * kNearestPartialDoubles;
#pragma unroll
        for (uint32_t k = 0; k < kAlignTerms; ++k) out[k] = p.v[k];
    }
}

__global__ __launch_bounds__(256) void k_nearest_align_finish(uint32_t pass, uint32_t n_partials, NearestJob job) {
    const uint32_t t = threadIdx.x;
    AlignPartial p;
#pragma unroll
    for (uint32_t k = 0; k < kAlignTerms; ++k) p.v[k] = 0.0;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const double* in = job.partials + (size_t)j * kNearestPartialDoubles;
#pragma unroll
        for (uint32_t k = 0; k < kAlignTerms; ++k) p.v[k] += in[k];
    }
    p = nearest_combine_align(p);
    if (t != 0u) return;
    double* out = job.align + (pass ? 8u : 0u);  // pass 0: [0..6]; pass 1: [8..19]
    const uint32_t terms = pass ? kAlignTerms : 7u;
    for (uint32_t k = 0; k < terms; ++k) out[k] = p.v[k];
}

// The point-to-plane step's sums (spec section 27; align_plane_math.h), k_nearest_align's shape over the found pairs whose target has a
// kept, fitted normal n within the variation limit.  pass 0: the used pairs' count, the sum of q, and the found pairs left out;
// pass 1: about the centre c of pass 0 rounded to float32, d = q - c and g = q - t in float32, and in double a = d x n, e = g . n,
// J = (a, n): the upper triangle of sum J J^T, sum J e, sum e^2 and the sum of d2.  Nothing changes with the sign of n.
__global__ __launch_bounds__(256) void k_nearest_align_plane(uint64_t n, uint32_t pass, const uint4* __restrict__ pc, NearestJob job, AlignPlaneJob plane) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (pass) {
        const double pairs = plane.sums[0];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = pairs > 0.0 ? (float)(plane.sums[1 + a] / pairs) : 0.0f;
    }
    AlignPlanePartial p;
#pragma unroll
    for (uint32_t k = 0; k < kAlignPlaneTerms; ++k) p.v[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        const uint32_t target = job.out_index[i];
        if (target == kNearestNone || target >= job.n_dst) continue;
        const float variation = plane.variation[target];
        if (!(variation < kNearestInf) || (plane.max_variation > 0.0f && !(variation <= plane.max_variation))) {  // (unfitted: +inf)
            if (pass == 0u) p.v[4] += 1.0;
            continue;
        }
        float q[3];
        nearest_map(job, pc[i], q[0], q[1], q[2]);
        if (pass == 0u) {
            p.v[0] += 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) p.v[1 + a] += (double)q[a];
            continue;
        }
        const uint4 e4 = job.dst_pc[target];
        const float tt[3] = {__uint_as_float(e4.x), __uint_as_float(e4.y), __uint_as_float(e4.z)};
        const float* nn = plane.normals + 3u * (size_t)target;
        double d[3], g[3], J[6];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            d[a] = (double)(q[a] - c[a]);
            g[a] = (double)(q[a] - tt[a]);
            J[3 + a] = (double)nn[a];
        }
        J[0] = d[1] * J[5] - d[2] * J[4];
        J[1] = d[2] * J[3] - d[0] * J[5];
        J[2] = d[0] * J[4] - d[1] * J[3];
        const double e = (g[0] * J[3] + g[1] * J[4]) + g[2] * J[5];
        uint32_t at = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int col = r; col < 6; ++col) p.v[at++] += J[r] * J[col];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) p.v[21 + r] += J[r] * e;
        p.v[27] += e * e;
        p.v[28] += (double)job.out_d2[i];
    }
    p = combine_terms(p);
    if (t == 0u) {
        double* out = plane.partials + (size_t)blockIdx.x * kAlignPlanePartialDoubles;
#pragma unroll
        for (uint32_t k = 0; k < kAlignPlaneTerms; ++k) out[k] = p.v[k];
    }
}

// One workgroup: the partials in index order.
__global__ __launch_bounds__(256) void k_nearest_align_plane_finish(uint32_t pass, uint32_t n_partials, AlignPlaneJob plane) {
    const uint32_t t = threadIdx.x;
    AlignPlanePartial p;
#pragma unroll
    for (uint32_t k = 0; k < kAlignPlaneTerms; ++k) p.v[k] = 0.0;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const double* in = plane.partials + (size_t)j * kAlignPlanePartialDoubles;
#pragma unroll
        for (uint32_t k = 0; k < kAlignPlaneTerms; ++k) p.v[k] += in[k];
    }
    p = combine_terms(p);
    if (t != 0u) return;
    double* out = plane.sums + (pass ? 8u : 0u);  // pass 0: [0..4]; pass 1: [8..36]
    const uint32_t terms = pass ? kAlignPlaneTerms : 5u;
#pragma unroll
    for (uint32_t k = 0; k < kAlignPlaneTerms; ++k)  // (unrolled: the terms stay in registers)
        if (k < terms) out[k] = p.v[k];
}

hipError_t launch_nearest_map(hipStream_t s, uint64_t n, const ModelFilter& f, const uint4* pc, const NearestJob& job) {
    GSX_LAUNCH(k_nearest_map, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, n, f, pc, job);
    return hipGetLastError();
}
hipError_t launch_nearest_query(hipStream_t s, uint64_t n, const uint4* src, uint32_t count, uint32_t to, const NearestJob& job) {
    GSX_LAUNCH(k_nearest_query, dim3((count + 255u) / 256u), dim3(256), 0, s, n, src, count, job.list[to & 1u], job.words + kNearestList + (to & 1u), job);
    return hipGetLastError();
}
hipError_t launch_nearest_brute(hipStream_t s, uint64_t n, const uint4* src, uint32_t count, uint32_t total, const NearestJob& job) {
    GSX_LAUNCH(k_nearest_brute, dim3(count), dim3(256), 0, s, n, src, total, job);
    return hipGetLastError();
}
hipError_t launch_nearest_stats(hipStream_t s, uint64_t n, const NearestJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_nearest_stats, dim3(groups), dim3(256), 0, s, n, job);
    GSX_LAUNCH(k_nearest_stats_finish, dim3(1), dim3(256), 0, s, groups, job);
    return hipGetLastError();
}
hipError_t launch_nearest_transfer(hipStream_t s, uint64_t n, const NearestJob& job) {
    GSX_LAUNCH(k_nearest_transfer, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, n, job);
    return hipGetLastError();
}
hipError_t launch_nearest_select(hipStream_t s, uint64_t n, const NearestJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_nearest_select, dim3(groups), dim3(256), 0, s, n, job);
    return launch_select_finish(s, job.sel, groups, job.words + kNearestHit, job.words + kNearestSelected);
}
hipError_t launch_nearest_align(hipStream_t s, uint64_t n, const uint4* pc, const NearestJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        GSX_LAUNCH(k_nearest_align, dim3(groups), dim3(256), 0, s, n, pass, pc, job);
        GSX_LAUNCH(k_nearest_align_finish, dim3(1), dim3(256), 0, s, pass, groups, job);
    }
    return hipGetLastError();
}

hipError_t launch_nearest_align_plane(hipStream_t s, uint64_t n, const uint4* pc, const NearestJob& job, const AlignPlaneJob& plane) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        GSX_LAUNCH(k_nearest_align_plane, dim3(groups), dim3(256), 0, s, n, pass, pc, job, plane);
        GSX_LAUNCH(k_nearest_align_plane_finish, dim3(1), dim3(256), 0, s, pass, groups, plane);
    }
    return hipGetLastError();
}

}  // namespace gsx
