// kernels_normals.hip — the model normals for gfx950 (spec/RENDER_SPEC.md §26, "Model normals"): gsx_model_normals and
// gsx_model_select_normals.  The grid is section 18's (kernels_neighbors.hip builds it, once a round); the rules are normals_math.h's;
// the rounds' schedule is radius_search.h's, run by gsx_api_normals.cpp as gsx_api_knn.cpp runs it.
//   k_normals_fill       normals = 0, variation = +inf, indices = none: what a Gaussian that is not fitted keeps;
//   k_normals_query<K>   one lane per entry of `src`, k_knn_query's walk over the 27 cells.  A record is a candidate if d2 <= r2, it is
//                        not the entry itself (by index), its key (d2 bits, index) is below the lane's k-th smallest and its own cell
//                        IS the visited cell.  The K smallest keys live in 2 K registers (nm_offer: an unrolled compare-exchange chain
//                        over constant indices).  There is no early exit at a k-th distance of 0: a smaller index may still tie.  The
//                        list is proven iff its k-th d2 is <= r2; a proven lane fits at once: it gathers its k neighbours' positions
//                        by index from the model's position plane (16 B each, in list order) and stores the normal, the variation
//                        and, where wanted, the indices.  One that is not proven appends its entry to the next list (wave_append);
//   k_normals_brute<K>   the exact fallback, one workgroup per list entry: the lanes stride over all records, each keeps its K smallest
//                        keys; the 256 lists go to LDS (K x 256 x 8 B: 32 KiB at K = 16) and are merged in k steps: every lane offers
//                        the head of its list, a wave and workgroup minimum picks one (keys are unique: no lane tie-break), its owner
//                        advances.  Lane 0 fits;
//   k_normals_stats      index order: the fitted Gaussians' count, the variations' minimum, maximum and double sum, one partial a
//                        workgroup, combined by one workgroup in index order: no atomics, the same bits on every call;
//   k_normals_select     k_knn_select's shape with nm_select_hit on the stored normal and variation; the participant bits are not read:
//                        whoever does not participate kept the fill's variation, +inf, which is never hit.
// Every loop is bounded by n, 27, K or a list's length; no lane waits for another's progress; no kernel caps its grid.  Built with
// -ffp-contract=off.  Bounds: an original index is checked against n before a store by it, a gathered neighbour index against n
// before the load by it, a list slot against n (a list's capacity), a bucket's end against the participant count before the walk.
#include "gsx_internal.h"
#include "knn_math.h"
#include "neighbors_grid.h"
#include "normals_math.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
constexpr float kNormalsInf = __builtin_huge_valf();

struct NormalsStatsPartial {
    uint32_t count;
    float mn, mx;
    double sum;
};
__device__ inline NormalsStatsPartial normals_combine_stats(uint32_t count, float mn, float mx, double sum) {
    return group_fold(NormalsStatsPartial{wave_sum(count), wave_min(mn), wave_max(mx), wave_sum(sum)},
                      [](NormalsStatsPartial a, const NormalsStatsPartial& b) {
                          return NormalsStatsPartial{a.count + b.count, fminf(a.mn, b.mn), fmaxf(a.mx, b.mx), a.sum + b.sum};
                      });
}
__device__ inline void normals_store_double(uint32_t* __restrict__ at, double v) {  // at: an even word offset of a 128-byte aligned block
    *reinterpret_cast<double*>(at) = v;
}
__device__ inline double normals_load_double(const uint32_t* __restrict__ at) { return *reinterpret_cast<const double*>(at); }

// A resolved entry: the fit of its list, stored by its original index, and the list's indices where they are wanted.
template <int K>
__device__ inline void normals_store_entry(uint64_t n, const NormalsJob& job, const uint4& self, const uint64_t (&b)[K]) {
    const uint32_t index = self.w;
    if (index >= n) return;  // (never: the scatter wrote an index below n)
    const float p[3] = {__uint_as_float(self.x), __uint_as_float(self.y), __uint_as_float(self.z)};
    const uint4* __restrict__ pc = job.pc;
    const NormalFit f = nm_plane_fit(b, job.k, p, [&](uint32_t j, float (&out)[3]) {
        uint4 e = self;  // (an index at or above n never arrives: the records hold indices below n)
        if (j < n) e = pc[j];
        out[0] = __uint_as_float(e.x);
        out[1] = __uint_as_float(e.y);
        out[2] = __uint_as_float(e.z);
    }, job.orient, job.toward);
    float* __restrict__ nrm = job.normals + (uint64_t)index * 3u;
    nrm[0] = f.n[0];
    nrm[1] = f.n[1];
    nrm[2] = f.n[2];
    job.variation[index] = f.variation;
    if (job.indices) nm_store_indices(b, job.k, job.indices + (uint64_t)index * job.k);
}
}  // namespace

__global__ __launch_bounds__(256) void k_normals_fill(uint32_t* __restrict__ dst, uint64_t count, uint32_t value) {
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u;
        if (i < count) dst[i] = value;
    }
}

template <int K>
__global__ __launch_bounds__(256) void k_normals_query(uint64_t n, const uint4* __restrict__ src, uint32_t count, uint4* __restrict__ next,
                                                       uint32_t* __restrict__ next_count, NormalsJob job) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool unresolved = false;
    uint4 self = make_uint4(0u, 0u, 0u, 0u);
    if (p < count) {
        const NbFrame g = nb_frame(job.nb);
        const float r2 = job.nb.r2;
        self = src[p];
        const float px = __uint_as_float(self.x), py = __uint_as_float(self.y), pz = __uint_as_float(self.z);
        uint64_t b[K];
        nm_reset(b, job.k);
        nb_walk(g, job.nb, nb_cell3(g, self), [&](const uint4& r, const NbVisit& v) {
            const float d2 = nb_d2(px, py, pz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z));
            // (a key that is not below the k-th smallest changes no list: the test spares the chain and comes before the cell test)
            if (d2 <= r2 && r.w != self.w) {
                const uint64_t key = nm_key(d2, r.w);
                if (key < nm_last(b) && v.holds(r)) nm_offer(b, key);
            }
            return true;  // (no early exit: at a k-th distance of 0 a smaller index may still tie)
        });
        if (nm_list_proven(nm_last(b), r2))
            normals_store_entry(n, job, self, b);
        else
            unresolved = true;
    }
    wave_append(unresolved, self, next, next_count, n);  // (every lane arrives here; at most `count` <= n entries are appended)
}

template <int K>
__global__ __launch_bounds__(256) void k_normals_brute(uint64_t n, const uint4* __restrict__ src, uint32_t total, NormalsJob job) {
    static_assert(kNormalsBruteLanes == 256u, "one list a lane");
    __shared__ unsigned long long s_best[K][256];  // the lanes' lists, ascending down a column
    __shared__ unsigned long long s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint4 self = src[blockIdx.x];
    const float px = __uint_as_float(self.x), py = __uint_as_float(self.y), pz = __uint_as_float(self.z);
    const uint32_t records = min(total, job.nb.result[kNbCount]);
    uint64_t b[K];
    nm_reset(b, job.k);
#pragma unroll 1
    for (uint32_t q = t; q < records; q += 256u) {
        const uint4 r = job.nb.records[q];
        if (r.w == self.w) continue;  // self is excluded by index, not by value
        const uint64_t key = nm_key(nb_d2(px, py, pz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z)), r.w);
        if (key < nm_last(b)) nm_offer(b, key);
    }
#pragma unroll
    for (int q = 0; q < K; ++q) s_best[q][t] = b[q];  // (read back by this lane alone)
    uint32_t head = (uint32_t)K - job.k;  // (the slots before it are the pinned ones)
    uint64_t row[K];
    nm_reset(row, job.k);
#pragma unroll
    for (int q = 0; q < K; ++q) {
        if ((uint32_t)q + job.k < (uint32_t)K) continue;  // (uniform)
        const uint64_t mine = head < (uint32_t)K ? (uint64_t)s_best[head][t] : kNormalsEmpty;
        const uint64_t key = wave_min(mine);
        if (lane == 0u) s_wave[wave] = key;
        __syncthreads();
        unsigned long long best = s_wave[0];
#pragma unroll
        for (uint32_t w = 1; w < 4u; ++w) best = s_wave[w] < best ? s_wave[w] : best;
        __syncthreads();  // (before the next step's stores)
        row[q] = best;
        if (mine == best && best != kNormalsEmpty) head += 1u;  // (a neighbour's key is in one lane's list alone)
    }
    if (t == 0u) normals_store_entry(n, job, self, row);
}

// the fitted Gaussians' count and their variations' min, max and sum
__global__ __launch_bounds__(256) void k_normals_stats(uint64_t n, NormalsJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    uint32_t count = 0;
    float mn = kNormalsInf, mx = -kNormalsInf;
    double sum = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        const float s = job.variation[i];
        if (!nm_is_fitted(s)) continue;
        count += 1u;
        mn = fminf(mn, s);
        mx = fmaxf(mx, s);
        sum += (double)s;
    }
    const NormalsStatsPartial p = normals_combine_stats(count, mn, mx, sum);
    if (t == 0u) {
        uint32_t* out = job.partials + (size_t)blockIdx.x * kNormalsPartialWords;
        out[0] = p.count; out[1] = __float_as_uint(p.mn); out[2] = __float_as_uint(p.mx);
        normals_store_double(out + 4, p.sum);
    }
}

// One workgroup: the partials in index order.
__global__ __launch_bounds__(256) void k_normals_stats_finish(uint32_t n_partials, NormalsJob job) {
    const uint32_t t = threadIdx.x;
    uint32_t count = 0;
    float mn = kNormalsInf, mx = -kNormalsInf;
    double sum = 0.0;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const uint32_t* in = job.partials + (size_t)j * kNormalsPartialWords;
        count += in[0];
        mn = fminf(mn, __uint_as_float(in[1]));
        mx = fmaxf(mx, __uint_as_float(in[2]));
        sum += normals_load_double(in + 4);
    }
    const NormalsStatsPartial p = normals_combine_stats(count, mn, mx, sum);
    if (t != 0u) return;
    uint32_t* w = job.words;
    w[kNormalsFitted] = p.count;
    w[kNormalsVarMin] = p.count ? __float_as_uint(p.mn) : 0u;
    w[kNormalsVarMax] = p.count ? __float_as_uint(p.mx) : 0u;
    normals_store_double(w + kNormalsSum, p.sum);
    normals_store_double(w + kNormalsMean, p.count ? p.sum / (double)p.count : 0.0);
}

__global__ __launch_bounds__(256) void k_normals_select(uint64_t n, NormalsJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    SelectCounts counts;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool hit = false;
        if (i < n) {  // (a Gaussian that does not participate kept variation +inf: never a hit)
            const float* __restrict__ nrm = job.normals + i * 3u;
            const float nv[3] = {nrm[0], nrm[1], nrm[2]};
            hit = nm_select_hit(job.mode, job.flags, nv, job.variation[i], job.dir, job.lo, job.hi);
        }
        select_write(job.nb.sel, hit, i, n, counts);
    }
    select_store_partial(job.nb.sel, counts);
}

hipError_t launch_normals_fill(hipStream_t s, uint64_t n, const NormalsJob& job) {
    GSX_LAUNCH(k_normals_fill, dim3((uint32_t)extract_groups(n * 3u)), dim3(256), 0, s, reinterpret_cast<uint32_t*>(job.normals), n * 3u, 0u);
    GSX_LAUNCH(k_normals_fill, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, reinterpret_cast<uint32_t*>(job.variation), n, 0x7F800000u);
    if (job.indices) GSX_LAUNCH(k_normals_fill, dim3((uint32_t)extract_groups(n * job.k)), dim3(256), 0, s, job.indices, n * job.k, kNormalsNone);
    return hipGetLastError();
}
hipError_t launch_normals_query(hipStream_t s, uint64_t n, const uint4* src, uint32_t count, uint32_t to, const NormalsJob& job) {
    const dim3 grid((count + 255u) / 256u);
    uint4* next = job.list[to & 1u];
    uint32_t* next_count = job.words + kNormalsList + (to & 1u);
    switch (knn_round_k(job.k)) {
        case 4u: GSX_LAUNCH(k_normals_query<4>, grid, dim3(256), 0, s, n, src, count, next, next_count, job); break;
        case 8u: GSX_LAUNCH(k_normals_query<8>, grid, dim3(256), 0, s, n, src, count, next, next_count, job); break;
        default: GSX_LAUNCH(k_normals_query<16>, grid, dim3(256), 0, s, n, src, count, next, next_count, job); break;
    }
    return hipGetLastError();
}
hipError_t launch_normals_brute(hipStream_t s, uint64_t n, const uint4* src, uint32_t count, uint32_t total, const NormalsJob& job) {
    switch (knn_round_k(job.k)) {
        case 4u: GSX_LAUNCH(k_normals_brute<4>, dim3(count), dim3(256), 0, s, n, src, total, job); break;
        case 8u: GSX_LAUNCH(k_normals_brute<8>, dim3(count), dim3(256), 0, s, n, src, total, job); break;
        default: GSX_LAUNCH(k_normals_brute<16>, dim3(count), dim3(256), 0, s, n, src, total, job); break;
    }
    return hipGetLastError();
}
hipError_t launch_normals_stats(hipStream_t s, uint64_t n, const NormalsJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_normals_stats, dim3(groups), dim3(256), 0, s, n, job);
    GSX_LAUNCH(k_normals_stats_finish, dim3(1), dim3(256), 0, s, groups, job);
    return hipGetLastError();
}
hipError_t launch_normals_select(hipStream_t s, uint64_t n, const NormalsJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_normals_select, dim3(groups), dim3(256), 0, s, n, job);
    return launch_select_finish(s, job.nb.sel, groups, job.words + kNormalsHit, job.words + kNormalsSelected);
}

}  // namespace gsx
