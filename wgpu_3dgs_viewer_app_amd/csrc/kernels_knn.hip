// kernels_knn.hip — the nearest neighbours for gfx950 (spec/RENDER_SPEC.md §20, "Model nearest neighbours"): gsx_model_knn and
// gsx_model_select_knn.  The grid is section 18's (kernels_neighbors.hip builds it, once a round); the rules are knn_math.h's.
// The participants' count, box and trimmed box, from which the host derives the search radii (radius_search.h, called by
// gsx_api_knn.cpp), come from the bounds kernels (kernels_bounds.hip), whose participants are the same: the filter and three finite
// coordinates.
//   k_knn_fill      scores[] and rows[] = +inf: what a Gaussian that does not participate keeps;
//   k_knn_query<K>  one lane per entry of `src` (round 1: the grid's records in bucket order, so a wave's lanes share cells; later
//                   rounds: the unresolved list): the 27 cells around the entry's own, walked as k_nb_query walks them.  A record
//                   is a candidate if d2 <= r2, it is not the entry itself (by index) and its own cell IS the visited cell.  The K
//                   best live in K registers (knn_insert: an unrolled compare-exchange chain, no runtime index).  The row is proven
//                   iff its k-th smallest is <= r2 (knn_math.h): a proven lane stores its score, and its row if rows are wanted; one
//                   that is not proven drops what it has and appends its 16-byte entry to the next list: one returning add a wave
//                   (wave_reduce.h: wave_append).  The list's order differs from call to call; no result depends on it;
//   k_knn_brute<K>  the exact fallback, one workgroup per list entry: the lanes stride over all records, each keeps its K best; the
//                   256 lists go to LDS and are merged in k steps: every lane offers the head of its list, a wave and workgroup
//                   minimum of (value bits, lane) picks one, the winner advances its head.  Equal values of different lanes all
//                   count;
//   k_knn_stats     index order, twice: the finite scores' count, minimum, maximum and double sum, then the double sum of squared
//                   deviations from the mean; one partial a workgroup, combined by one workgroup in index order: no atomics, the
//                   same bits on every call ("Model properties");
//   k_knn_select    k_nb_select's shape with the score test.
// Every loop is bounded by n, 27, K or a list's length; no lane waits for another's progress; no kernel caps its grid.  Built with
// -ffp-contract=off.  Bounds: an original index is checked against n before a store by it, a list slot against n (a list's
// capacity), a bucket's end against the participant count before the walk.
#include "gsx_internal.h"
#include "knn_math.h"
#include "neighbors_grid.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
constexpr float kKnnInf = __builtin_huge_valf();

// The workgroup's statistics partial, valid in thread 0 afterwards: count, minimum, maximum, and a double sum added in the order of
// the wave's butterfly and in wave order across the four (wave_reduce.h).
struct KnnStatsPartial {
    uint32_t count;
    float mn, mx;
    double sum;
};
__device__ inline KnnStatsPartial knn_combine_stats(uint32_t count, float mn, float mx, double sum) {
    return group_fold(KnnStatsPartial{wave_sum(count), wave_min(mn), wave_max(mx), wave_sum(sum)}, [](KnnStatsPartial a, const KnnStatsPartial& b) {
        return KnnStatsPartial{a.count + b.count, fminf(a.mn, b.mn), fmaxf(a.mx, b.mx), a.sum + b.sum};
    });
}
__device__ inline void knn_store_double(uint32_t* __restrict__ at, double v) {  // at: an even word offset of a 128-byte aligned block
    *reinterpret_cast<double*>(at) = v;
}
__device__ inline double knn_load_double(const uint32_t* __restrict__ at) { return *reinterpret_cast<const double*>(at); }
}  // namespace

__global__ __launch_bounds__(256) void k_knn_fill(float* __restrict__ dst, uint64_t count) {
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u;
        if (i < count) dst[i] = kKnnInf;
    }
}

// A resolved entry's score, and its row where rows are wanted.
template <int K>
__device__ inline void knn_store_row(uint64_t n, const KnnJob& job, uint32_t index, const float (&b)[K]) {
    if (index >= n) return;  // (never: the scatter wrote an index below n)
    job.scores[index] = knn_score(b, job.k, job.score);
    if (job.rows) {
        knn_store(b, job.k, job.rows + (uint64_t)index * job.k);
    }
}

template <int K>
__global__ __launch_bounds__(256) void k_knn_query(uint64_t n, const uint4* __restrict__ src, uint32_t count, uint4* __restrict__ next, uint32_t* __restrict__ next_count,
                                                   KnnJob job) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool unresolved = false;
    uint4 self = make_uint4(0u, 0u, 0u, 0u);
    if (p < count) {
        const NbFrame g = nb_frame(job.nb);
        const float r2 = job.nb.r2;
        self = src[p];
        const float px = __uint_as_float(self.x), py = __uint_as_float(self.y), pz = __uint_as_float(self.z);
        float b[K];
        knn_clear(b, job.k);
        nb_walk(g, job.nb, nb_cell3(g, self), [&](const uint4& r, const NbVisit& v) {
            const float d2 = nb_d2(px, py, pz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z));
            // (a value that is not below the k-th best changes no row: the test spares the chain and comes before the cell test)
            if (d2 <= r2 && r.w != self.w && d2 < knn_kth(b) && v.holds(r)) {
                knn_insert(b, d2);
                return knn_kth(b) != 0.0f;  // the k-th best is 0: nothing can lower the row any more
            }
            return true;
        });
        if (knn_proven(knn_kth(b), r2))
            knn_store_row(n, job, self.w, b);
        else
            unresolved = true;
    }
    wave_append(unresolved, self, next, next_count, n);  // (every lane arrives here; at most `count` <= n entries are appended)
}

template <int K>
__global__ __launch_bounds__(256) void k_knn_brute(uint64_t n, const uint4* __restrict__ src, uint32_t total, KnnJob job) {
    static_assert(kKnnBruteLanes == 256u, "one list a lane");
    __shared__ float s_best[K][256];  // the lanes' lists, ascending down a column
    __shared__ unsigned long long s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint4 self = src[blockIdx.x];
    const float px = __uint_as_float(self.x), py = __uint_as_float(self.y), pz = __uint_as_float(self.z);
    const uint32_t records = min(total, job.nb.result[kNbCount]);
    float b[K];
    knn_clear(b, job.k);
#pragma unroll 1
    for (uint32_t q = t; q < records; q += 256u) {
        const uint4 r = job.nb.records[q];
        if (r.w == self.w) continue;  // self is excluded by index, not by value
        const float d2 = nb_d2(px, py, pz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z));
        if (d2 < knn_kth(b)) knn_insert(b, d2);
    }
#pragma unroll
    for (int q = 0; q < K; ++q) s_best[q][t] = b[q];  // (read back by this lane alone)
    uint32_t head = (uint32_t)K - job.k;  // (the slots before it are the pinned ones)
    float row[K];
    knn_clear(row, job.k);
#pragma unroll
    for (int q = 0; q < K; ++q) {
        if ((uint32_t)q + job.k < (uint32_t)K) continue;  // (uniform)
        const float mine = head < (uint32_t)K ? s_best[head][t] : kKnnInf;
        // (d2 is +0 or above, never NaN: the bits order as the values do; the lane breaks ties)
        const uint64_t key = wave_min(((uint64_t)__float_as_uint(mine) << 32) | t);
        if (lane == 0u) s_wave[wave] = key;
        __syncthreads();
        unsigned long long best = s_wave[0];
#pragma unroll
        for (uint32_t w = 1; w < 4u; ++w) best = s_wave[w] < best ? s_wave[w] : best;
        __syncthreads();  // (before the next step's stores)
        row[q] = __uint_as_float((uint32_t)(best >> 32));
        if ((uint32_t)best == t) head += 1u;
    }
    if (t == 0u) knn_store_row(n, job, self.w, row);
}

// pass 0: count, min, max, sum of the finite scores; pass 1: the sum of squared deviations from words[kKnnMean]
__global__ __launch_bounds__(256) void k_knn_stats(uint64_t n, uint32_t pass, KnnJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const double mean = pass ? knn_load_double(job.words + kKnnMean) : 0.0;
    uint32_t count = 0;
    float mn = kKnnInf, mx = -kKnnInf;
    double sum = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        const float s = job.scores[i];
        if (!nb_finite(s)) continue;  // (a Gaussian that does not participate, or a row that holds a +inf)
        if (pass) {
            const double d = (double)s - mean;
            sum += d * d;
        } else {
            count += 1u;
            mn = fminf(mn, s);
            mx = fmaxf(mx, s);
            sum += (double)s;
        }
    }
    const KnnStatsPartial p = knn_combine_stats(count, mn, mx, sum);
    if (t == 0u) {
        uint32_t* out = job.partials + (size_t)blockIdx.x * kKnnPartialWords;
        out[0] = p.count; out[1] = __float_as_uint(p.mn); out[2] = __float_as_uint(p.mx);
        knn_store_double(out + 4, p.sum);
    }
}

// One workgroup: the partials in index order.
__global__ __launch_bounds__(256) void k_knn_stats_finish(uint32_t pass, uint32_t n_partials, KnnJob job) {
    const uint32_t t = threadIdx.x;
    uint32_t count = 0;
    float mn = kKnnInf, mx = -kKnnInf;
    double sum = 0.0;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const uint32_t* in = job.partials + (size_t)j * kKnnPartialWords;
        count += in[0];
        mn = fminf(mn, __uint_as_float(in[1]));
        mx = fmaxf(mx, __uint_as_float(in[2]));
        sum += knn_load_double(in + 4);
    }
    const KnnStatsPartial p = knn_combine_stats(count, mn, mx, sum);
    if (t != 0u) return;
    uint32_t* w = job.words;
    if (pass == 0u) {
        w[kKnnScored] = p.count;
        w[kKnnScoreMin] = p.count ? __float_as_uint(p.mn) : 0u;
        w[kKnnScoreMax] = p.count ? __float_as_uint(p.mx) : 0u;
        knn_store_double(w + kKnnSum, p.sum);
        knn_store_double(w + kKnnMean, p.count ? p.sum / (double)p.count : 0.0);
    } else {
        const uint32_t m = w[kKnnScored];
        const double std = knn_std(p.sum, m);
        knn_store_double(w + kKnnSs, p.sum);
        knn_store_double(w + kKnnStd, std);
        w[kKnnThreshold] = job.mode == kKnnSelectOutliers ? __float_as_uint(knn_threshold(knn_load_double(w + kKnnMean), std, job.std_ratio)) : 0u;
    }
}

__global__ __launch_bounds__(256) void k_knn_select(uint64_t n, KnnJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const bool outliers = job.mode == kKnnSelectOutliers;
    const float threshold = __uint_as_float(job.words[kKnnThreshold]);
    const bool any_scored = job.words[kKnnScored] != 0u;
    SelectCounts counts;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool hit = false;
        if (i < n && ((job.nb.participants[i >> 5] >> (t & 31u)) & 1u)) {
            const float s = job.scores[i];
            hit = outliers ? (any_scored && s > threshold) : (s >= job.lo && s <= job.hi);
        }
        select_write(job.nb.sel, hit, i, n, counts);
    }
    select_store_partial(job.nb.sel, counts);
}

hipError_t launch_knn_fill(hipStream_t s, uint64_t n, const KnnJob& job) {
    GSX_LAUNCH(k_knn_fill, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, job.scores, n);
    if (job.rows) GSX_LAUNCH(k_knn_fill, dim3((uint32_t)extract_groups(n * job.k)), dim3(256), 0, s, job.rows, n * job.k);
    return hipGetLastError();
}
hipError_t launch_knn_query(hipStream_t s, uint64_t n, const uint4* src, uint32_t count, uint32_t to, const KnnJob& job) {
    const dim3 grid((count + 255u) / 256u);
    uint4* next = job.list[to & 1u];
    uint32_t* next_count = job.words + kKnnList + (to & 1u);
    switch (knn_round_k(job.k)) {
        case 4u: GSX_LAUNCH(k_knn_query<4>, grid, dim3(256), 0, s, n, src, count, next, next_count, job); break;
        case 8u: GSX_LAUNCH(k_knn_query<8>, grid, dim3(256), 0, s, n, src, count, next, next_count, job); break;
        default: GSX_LAUNCH(k_knn_query<16>, grid, dim3(256), 0, s, n, src, count, next, next_count, job); break;
    }
    return hipGetLastError();
}
hipError_t launch_knn_brute(hipStream_t s, uint64_t n, const uint4* src, uint32_t count, uint32_t total, const KnnJob& job) {
    switch (knn_round_k(job.k)) {
        case 4u: GSX_LAUNCH(k_knn_brute<4>, dim3(count), dim3(256), 0, s, n, src, total, job); break;
        case 8u: GSX_LAUNCH(k_knn_brute<8>, dim3(count), dim3(256), 0, s, n, src, total, job); break;
        default: GSX_LAUNCH(k_knn_brute<16>, dim3(count), dim3(256), 0, s, n, src, total, job); break;
    }
    return hipGetLastError();
}
hipError_t launch_knn_stats(hipStream_t s, uint64_t n, const KnnJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        GSX_LAUNCH(k_knn_stats, dim3(groups), dim3(256), 0, s, n, pass, job);
        GSX_LAUNCH(k_knn_stats_finish, dim3(1), dim3(256), 0, s, pass, groups, job);
    }
    return hipGetLastError();
}
hipError_t launch_knn_select(hipStream_t s, uint64_t n, const KnnJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_knn_select, dim3(groups), dim3(256), 0, s, n, job);
    return launch_select_finish(s, job.nb.sel, groups, job.words + kKnnHit, job.words + kKnnSelected);
}

}  // namespace gsx
