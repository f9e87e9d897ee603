// kernels_neighbors.hip — the neighbour counts for gfx950 (spec/RENDER_SPEC.md §18, "Model neighbours"): gsx_model_neighbors and
// gsx_model_select_neighbors.  A hashed uniform grid, built by a counting sort, in six passes on one stream:
//   k_nb_reduce   index order: a Gaussian participates if it passes the filter (prop_keep: ModelFilter + extract_keep_word) and its
//                 three stored coordinates are finite; count, non-finite count and the minimum and maximum per axis, one partial a
//                 workgroup; k_nb_finish (one workgroup) combines them: the minimum is the grid's origin, the maximum is read by
//                 gsx_model_decimate_edge alone;
//   k_nb_cell     index order: the participant bits (a wave ballot, two words), the cell (neighbors_math.h: nb_cell) and its bucket,
//                 one non-returning integer add into the bucket's table word; counts[i] = 0 for every Gaussian;
//   k_nb_scan_*   the table's sizes become starts: block sums, the one-workgroup scan of gsx_model_extract over them
//                 (k_extract_scan), then the exclusive scan of every block plus its base, in place;
//   k_nb_scatter  index order: a participant draws its slot with ONE returning add on its bucket's table word and stores a 16-byte
//                 record (x, y, z bits, original index) there: the word that held the bucket's start ends as the bucket's end, which
//                 is the start of the next bucket, so the table needs no second copy.  The order inside a bucket depends on the
//                 order of the adds; no result does (a count is a sum over the bucket, a saturated count min(sum, cap));
//   k_nb_query    one lane per record, in bucket order, so a wave's lanes share cells: the walk over the 27 cells around the lane's
//                 own (neighbors_grid.h: nb_walk).  A record counts if d2 <= r2, it is not the lane's own and its own cell is the
//                 visited cell.  The lane stops at max_count.  The count goes to counts[original index], and into the workgroup's LDS bins (up to 4096
//                 words, non-returning LDS adds), which leave as non-returning global adds of the non-zero bins;
//   k_nb_select   index order: a participant is hit if its count lies in [count_lo, count_hi]; the write, the partial and its sum are
//                 selection_write.h's (select_write, k_select_finish).
// Every cross-workgroup combination is an integer add or a minimum of finite floats: the same bits in any order.  Built with
// -ffp-contract=off.  Offsets are 64-bit where they scale with n x 16.  Nothing of the model but the selection (k_nb_select) is
// written.  Bounds: a record slot is checked against n before the store, a bucket's end against the participant count before the walk.
#include "gsx_internal.h"
#include "neighbors_grid.h"
#include "neighbors_math.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
static_assert(kNbMaxCount + 1u <= 4096u, "the query's LDS bins");
static_assert(kNbScanBlock == 4u * 256u, "four table words a lane");
constexpr float kNbInf = __builtin_huge_valf();

}  // namespace

// What k_nb_reduce leaves per workgroup and k_nb_finish combines: sums, and minima and maxima of finite floats (or the identities):
// the same bits in any order.
struct NbPartial {
    uint32_t count = 0, nonfinite = 0;
    float mn[3] = {kNbInf, kNbInf, kNbInf}, mx[3] = {-kNbInf, -kNbInf, -kNbInf};
    __device__ void merge(const NbPartial& b) {
        count += b.count;
        nonfinite += b.nonfinite;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(mn[a], b.mn[a]);
            mx[a] = fmaxf(mx[a], b.mx[a]);
        }
    }
};
static_assert(sizeof(NbPartial) == 4 * kNbPartialWords, "count | non-finite | min xyz | max xyz");
// The workgroup's partial from its lanes', valid in thread 0.
__device__ inline NbPartial nb_fold(NbPartial p) {
    p.count = wave_sum(p.count);
    p.nonfinite = wave_sum(p.nonfinite);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p.mn[a] = wave_min(p.mn[a]);
        p.mx[a] = wave_max(p.mx[a]);
    }
    return group_fold(p, [](NbPartial a, const NbPartial& b) {
        a.merge(b);
        return a;
    });
}

__global__ __launch_bounds__(256) void k_nb_reduce(uint64_t n, ModelFilter f, const uint4* __restrict__ pc, NbPartial* __restrict__ partials) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    NbPartial p;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform: the round holds no Gaussian)
        const uint64_t i = base + k * 256u + t;
        if (prop_keep(f, n, i, t)) {  // (every lane of the wave makes the call: a ballot inside)
            const uint4 e = pc[i];
            const float x = __uint_as_float(e.x), y = __uint_as_float(e.y), z = __uint_as_float(e.z);
            if (nb_finite(x) && nb_finite(y) && nb_finite(z)) p.merge(NbPartial{1u, 0u, {x, y, z}, {x, y, z}});
            else p.nonfinite += 1u;
        }
    }
    p = nb_fold(p);
    // ONE partial per workgroup, plain stores ("Model properties": atomics on a few words cost more than the stream)
    if (t == 0u) partials[blockIdx.x] = p;
}

// One workgroup: the partials combined into the result block.
__global__ __launch_bounds__(256) void k_nb_finish(const NbPartial* __restrict__ partials, uint32_t n_partials, uint32_t* __restrict__ result) {
    const uint32_t t = threadIdx.x;
    NbPartial p;
    for (uint32_t j = t; j < n_partials; j += 256u) p.merge(partials[j]);
    p = nb_fold(p);
    if (t != 0u) return;
    result[kNbCount] = p.count;
    result[kNbNonfinite] = p.nonfinite;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        result[kNbOrigin + a] = __float_as_uint(p.mn[a]);
        result[kNbMax + a] = __float_as_uint(p.mx[a]);
    }
}

__global__ __launch_bounds__(256) void k_nb_cell(uint64_t n, ModelFilter f, const uint4* __restrict__ pc, NeighborJob job) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const NbFrame g = nb_frame(job);
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool part = prop_keep(f, n, i, t);
        if (part) {
            const uint4 e = pc[i];
            part = nb_finite(__uint_as_float(e.x)) && nb_finite(__uint_as_float(e.y)) && nb_finite(__uint_as_float(e.z));
            if (part) atomicAdd(&job.table[nb_bucket(g, nb_cell3(g, e))], 1u);  // (the value is not used: a non-returning add)
        }
        const unsigned long long part64 = __ballot(part);
        if (i < n) {
            job.counts[i] = 0u;
            if ((lane & 31u) == 0u) job.participants[i >> 5] = (uint32_t)(part64 >> lane);  // (bits at and above n are clear)
        }
    }
}

// The sum of one block of kNbScanBlock table words.
__global__ __launch_bounds__(256) void k_nb_scan_sums(const uint32_t* __restrict__ table, uint32_t words, uint32_t* __restrict__ sums) {
    const uint32_t at = blockIdx.x * kNbScanBlock + 4u * threadIdx.x;
    uint32_t own = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
        if (at + q < words) own += table[at + q];
    const uint32_t sum = group_fold(wave_sum(own), [](uint32_t a, uint32_t b) { return a + b; });
    if (threadIdx.x == 0u) sums[blockIdx.x] = sum;
}

// The exclusive scan of one block in place, on top of the block's base.
__global__ __launch_bounds__(256) void k_nb_scan_apply(uint32_t* __restrict__ table, uint32_t words, const uint32_t* __restrict__ bases) {
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t at = blockIdx.x * kNbScanBlock + 4u * t;
    uint32_t v[4], own = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        v[q] = at + q < words ? table[at + q] : 0u;
        own += v[q];
    }
    uint32_t incl = own;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = bases[blockIdx.x] + (incl - own);
    for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        if (at + q < words) table[at + q] = before;
        before += v[q];
    }
}

__global__ __launch_bounds__(256) void k_nb_scatter(uint64_t n, const uint4* __restrict__ pc, NeighborJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const NbFrame g = nb_frame(job);
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        if (!((job.participants[i >> 5] >> (t & 31u)) & 1u)) continue;
        const uint4 e = pc[i];
        const uint32_t slot = atomicAdd(&job.table[nb_bucket(g, nb_cell3(g, e))], 1u);  // the bucket's next free slot; the word ends as the bucket's end
        if (slot < n) job.records[slot] = make_uint4(e.x, e.y, e.z, (uint32_t)i);
    }
}

__global__ __launch_bounds__(256) void k_nb_query(uint64_t n, NeighborJob job) {
    __shared__ uint32_t s_bins[kNbMaxCount + 1u];
    const uint32_t t = threadIdx.x;
    const uint32_t bins = job.max_count + 1u;
    for (uint32_t j = t; j < bins; j += 256u) s_bins[j] = 0u;
    __syncthreads();
    const NbFrame g = nb_frame(job);
    const uint32_t p = blockIdx.x * 256u + t;
    if (p < g.total) {
        const float r2 = job.r2;
        const uint4 self = job.records[p];
        const float px = __uint_as_float(self.x), py = __uint_as_float(self.y), pz = __uint_as_float(self.z);
        const uint32_t cap = job.max_count;  // (1 at least)
        uint32_t cnt = 0;
        nb_walk(g, job, nb_cell3(g, self), [&](const uint4& r, const NbVisit& v) {
            if (nb_d2(px, py, pz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z)) <= r2 && r.w != self.w && v.holds(r)) cnt += 1u;
            return cnt < cap;
        });
        if (self.w < n) job.counts[self.w] = cnt;  // (always: the scatter wrote an index below n)
        atomicAdd(&s_bins[cnt], 1u);  // (non-returning LDS add)
    }
    __syncthreads();
    for (uint32_t j = t; j < bins; j += 256u) {
        const uint32_t c = s_bins[j];
        if (c) atomicAdd(&job.hist[j], c);
    }
}

__global__ __launch_bounds__(256) void k_nb_select(uint64_t n, NeighborJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    SelectCounts counts;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool hit = false;
        if (i < n && ((job.participants[i >> 5] >> (t & 31u)) & 1u)) {
            const uint32_t c = job.counts[i];
            hit = c >= job.count_lo && c <= job.count_hi;
        }
        select_write(job.sel, hit, i, n, counts);
    }
    select_store_partial(job.sel, counts);
}

hipError_t launch_neighbors_reduce(hipStream_t s, uint64_t n, const ModelFilter& f, const uint4* pc, const NeighborJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    NbPartial* partials = reinterpret_cast<NbPartial*>(job.partials);
    GSX_LAUNCH(k_nb_reduce, dim3(groups), dim3(256), 0, s, n, f, pc, partials);
    GSX_LAUNCH(k_nb_finish, dim3(1), dim3(256), 0, s, partials, groups, job.result);
    return hipGetLastError();
}
hipError_t launch_neighbors_cell(hipStream_t s, uint64_t n, const ModelFilter& f, const uint4* pc, const NeighborJob& job) {
    GSX_LAUNCH(k_nb_cell, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, n, f, pc, job);
    return hipGetLastError();
}
hipError_t launch_neighbors_scan(hipStream_t s, const NeighborJob& job) {
    const uint32_t words = 1u << job.bits, blocks = (words + kNbScanBlock - 1u) / kNbScanBlock;
    GSX_LAUNCH(k_nb_scan_sums, dim3(blocks), dim3(256), 0, s, job.table, words, job.scan_sums);
    const hipError_t e = launch_extract_scan(s, job.scan_sums, blocks, job.scan_bases, job.scan_total);
    if (e != hipSuccess) return e;
    GSX_LAUNCH(k_nb_scan_apply, dim3(blocks), dim3(256), 0, s, job.table, words, job.scan_bases);
    return hipGetLastError();
}
hipError_t launch_neighbors_scatter(hipStream_t s, uint64_t n, const uint4* pc, const NeighborJob& job) {
    GSX_LAUNCH(k_nb_scatter, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, n, pc, job);
    return hipGetLastError();
}
hipError_t launch_neighbors_query(hipStream_t s, uint64_t n, const NeighborJob& job) {
    GSX_LAUNCH(k_nb_query, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, n, job);
    return hipGetLastError();
}
hipError_t launch_neighbors_select(hipStream_t s, uint64_t n, const NeighborJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_nb_select, dim3(groups), dim3(256), 0, s, n, job);
    return launch_select_finish(s, job.sel, groups, job.result + kNbHit, job.result + kNbSelected);
}

}  // namespace gsx
