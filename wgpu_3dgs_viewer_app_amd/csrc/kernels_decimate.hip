// kernels_decimate.hip — gsx_model_decimate for gfx950 (spec/RENDER_SPEC.md §22, "Model decimate"): the Gaussians that share a cell
// of the neighbour grid become one moment-matched Gaussian of a new model.  After the grid's four passes (kernels_neighbors.hip: the
// records lie in bucket order, in an arbitrary order inside a bucket) on one stream:
//   k_dec_order      one lane per record: its bucket from the table.  A bucket of at most kDecRankBucket records is ordered by
//                    counting: the lane's rank is the number of records of the bucket whose (cell, index) key is smaller, and its key
//                    record goes to sorted[start + rank].  The first record of a larger bucket appends the bucket to `big`;
//   k_dec_sort_big   a workgroup per entry of `big` (any order: every bucket lands in its own range): a bitonic network over the
//                    bucket's key records, in LDS up to kDecLdsBucket records, in place in `sorted` above that — slower, by one
//                    workgroup however large the bucket, and as correct;
//   k_dec_heads      position order: a record whose predecessor has another cell key is its cell's head, and the head is the member
//                    with the smallest index: the representative.  The head bits (a ballot) and one popcount partial a workgroup;
//                    the representative's bit is set in the keep words by an OR whose result nobody reads;
//   k_dec_popc       the keep words' popcount partials.  Both bit planes are then scanned by k_extract_scan: a head's rank is its
//                    run, a representative's rank its destination index;
//   k_dec_runs       a head stores its position under its run and its destination index (from the keep words alone);
//   k_dec_map        every record looks its run up (the heads at or before it) and stores the destination index under its original
//                    index; a head also stores its cell's start and length by destination index, and counts into the statistics;
//   k_dec_merge      (a destination exists) one wave per cell of two members and more, lanes as the 58 columns of the sums
//                    (decimate_math.h).  64 members at a time: lane L decodes member L's position, covariance and colour into LDS,
//                    then every lane walks the members in ascending index and adds its column's term — the SH lanes load their one
//                    value of the member from its plane.  Both weightings are summed side by side (the mass sum decides at the end
//                    which one counts), so the members are read once.  The order of every sum is the member order: no float atomic,
//                    the same bits on every call.  Lane 0 writes the planes and the shade record of the cell from one set of words.
// The singletons, and every representative, are k_extract_scatter's copy of the stored bits.
// Built with -ffp-contract=off.  Offsets are 64-bit where they scale with n x 16.  Bounds: a slot of `sorted` is start + rank < end <=
// the participant count; an original index is checked against n before it addresses the map or the keep words; an entry of `big`
// against its capacity.
#include "decimate_math.h"
#include "gsx_internal.h"
#include "neighbors_grid.h"
#include "pod_planes.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
constexpr uint32_t kDecSortGroups = 1024u;  // workgroups of k_dec_sort_big: each takes every 1024th entry of `big`

__device__ inline uint4 dec_key_record(const NbFrame& g, const uint4 rec, uint32_t* bucket = nullptr) {
    const NbCell c = nb_cell3(g, rec);
    const uint64_t key = dec_cell_key(c.x, c.y, c.z);
    if (bucket) *bucket = nb_bucket(g, c);
    return make_uint4((uint32_t)key, (uint32_t)(key >> 32), rec.w, 0u);
}
// (cell, index) order of two key records; no two records share an index
__device__ inline bool dec_less(const uint4 a, const uint4 b) {
    if (a.y != b.y) return a.y < b.y;
    if (a.x != b.x) return a.x < b.x;
    return a.z < b.z;
}
// One compare-exchange network over a[0 .. size): every merge ascending, so the absent records past `size` stand for keys above all
// others and a pair that reaches one is left alone.  256 lanes; ends with a barrier.
__device__ inline void dec_bitonic(uint4* a, uint32_t size) {
    const uint32_t t = threadIdx.x;
    uint32_t pow2 = 1u;
    while (pow2 < size) pow2 <<= 1;
    const uint32_t half = pow2 >> 1;
    for (uint32_t k = 2u; k <= pow2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            const bool flip = j == (k >> 1);  // the first step of a merge mirrors the upper half
            for (uint32_t i = t; i < half; i += 256u) {
                const uint32_t off = i & (j - 1u), lo = ((i - off) << 1) + off;
                const uint32_t hi = flip ? ((i - off) << 1) + (k - 1u) - off : lo + j;
                if (hi < size) {
                    const uint4 x = a[lo], y = a[hi];
                    if (dec_less(y, x)) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// one SH float of a stored Gaussian, exactly dequantised (pod_planes.h: pod_load_sh's layout)
template <int SH>
__device__ inline float dec_load_sh(const ExtractPlanes& src, uint64_t n_src, uint64_t i, uint32_t f) {
    if (SH == GSX_SH_SINGLE) {
        if (f == 44u) return __uint_as_float(src.sh1[i]);
        return __uint_as_float(reinterpret_cast<const uint32_t*>(src.sh4)[((uint64_t)(f >> 2) * n_src + i) * 4u + (f & 3u)]);
    } else if (SH == GSX_SH_HALF) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(src.sh_h)[((uint64_t)(f >> 3) * n_src + i) * 4u + ((f & 7u) >> 1)];
        return (f & 1u) ? h_hi(w) : h_lo(w);
    } else if (SH == GSX_SH_NORM8) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(src.sh_q)[((uint64_t)(f >> 4) * n_src + i) * 4u + ((f & 15u) >> 2)];
        return dq_snorm8(w, (int)(f & 3u));
    }
    return 0.0f;
}
}  // namespace

__global__ __launch_bounds__(256) void k_dec_order(uint64_t n, DecimateJob job) {
    const NeighborJob& nb = job.nb;
    const NbFrame g = nb_frame(nb);
    const uint32_t total = min(g.total, (uint32_t)n);
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= total) return;
    uint32_t b;
    const uint4 own = dec_key_record(g, nb.records[p], &b);
    const uint32_t start = b ? nb.table[b - 1u] : 0u, end = min(nb.table[b], total);
    if (p < start || p >= end) return;  // (never: the scatter put the record into its bucket's range)
    if (end - start <= kDecRankBucket) {
        uint32_t rank = 0;
#pragma unroll 1
        for (uint32_t q = start; q < end; ++q) {
            const uint4 other = dec_key_record(g, nb.records[q]);
            rank += dec_less(other, own) ? 1u : 0u;  // (the record itself is not below itself)
        }
        job.sorted[start + rank] = own;  // (rank < end - start: the keys differ, so the ranks are a permutation)
    } else if (p == start) {
        const uint32_t slot = atomicAdd(&job.words[kDecBig], 1u);  // (any order: a bucket is sorted inside its own range)
        if (slot < job.big_cap) job.big[slot] = b;
    }
}

__global__ __launch_bounds__(256) void k_dec_sort_big(uint64_t n, DecimateJob job) {
    __shared__ uint4 s_rec[kDecLdsBucket];
    const NeighborJob& nb = job.nb;
    const uint32_t t = threadIdx.x;
    const NbFrame g = nb_frame(nb);
    const uint32_t total = min(g.total, (uint32_t)n);
    const uint32_t n_big = min(job.words[kDecBig], job.big_cap);
#pragma unroll 1
    for (uint32_t e = blockIdx.x; e < n_big; e += gridDim.x) {  // (uniform: the barriers below are reached by every lane)
        const uint32_t b = job.big[e];
        const uint32_t start = b ? nb.table[b - 1u] : 0u, end = min(nb.table[b], total);
        if (start >= end) continue;
        const uint32_t size = end - start;
        const bool in_lds = size <= kDecLdsBucket;
        uint4* a = in_lds ? s_rec : job.sorted + start;
        for (uint32_t q = t; q < size; q += 256u) a[q] = dec_key_record(g, nb.records[start + q]);
        __syncthreads();
        dec_bitonic(a, size);
        if (in_lds)
            for (uint32_t q = t; q < size; q += 256u) job.sorted[start + q] = s_rec[q];
        __syncthreads();  // s_rec is rewritten by the next bucket
    }
}

__global__ __launch_bounds__(256) void k_dec_heads(uint64_t n, DecimateJob job) {
    __shared__ uint32_t s_sum[8];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t total = min(job.nb.result[kNbCount], (uint32_t)n);
    const uint32_t base = blockIdx.x * kExtractGroup;
    uint32_t count = 0;  // lanes 0 and 32 of a wave
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= total) break;  // (uniform)
        const uint32_t p = base + k * 256u + t;
        bool head = false;
        if (p < total) {
            const uint4 cur = job.sorted[p];
            if (p == 0u) {
                head = true;
            } else {
                const uint4 prev = job.sorted[p - 1u];  // (another bucket's last record has another cell: a cell lies in one bucket)
                head = prev.x != cur.x || prev.y != cur.y;
            }
            // a head has the smallest index of its cell: the representative.  The OR's result is not used.
            if (head && cur.z < n) atomicOr(&job.keep[cur.z >> 5], 1u << (cur.z & 31u));
        }
        const unsigned long long heads64 = __ballot(head);
        if ((lane & 31u) == 0u && p < total) {
            const uint32_t word = (uint32_t)(heads64 >> lane);  // (bits at and above total are clear)
            job.heads[p >> 5] = word;
            count += extract_popc(word);
        }
    }
    if ((lane & 31u) == 0u) s_sum[t >> 5] = count;
    __syncthreads();
    if (t == 0u) {
        uint32_t s = 0;
        for (int j = 0; j < 8; ++j) s += s_sum[j];
        job.head_partials[blockIdx.x] = s;
    }
}

// the popcount partial of one group of kExtractGroupWords keep words
__global__ __launch_bounds__(64) void k_dec_popc(uint64_t n, const uint32_t* __restrict__ keep, uint32_t* __restrict__ partials) {
    const uint32_t lane = threadIdx.x;
    const uint64_t w = (uint64_t)blockIdx.x * kExtractGroupWords + lane;
    const uint32_t c = wave_sum((lane < kExtractGroupWords && w * 32u < n) ? extract_popc(keep[w]) : 0u);
    if (lane == 0u) partials[blockIdx.x] = c;
}

__global__ __launch_bounds__(256) void k_dec_runs(uint64_t n, DecimateJob job) {
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    const uint32_t t = threadIdx.x;
    const uint32_t total = min(job.nb.result[kNbCount], (uint32_t)n);
    const uint32_t base = blockIdx.x * kExtractGroup;
    if (blockIdx.x == 0u && t == 0u) job.run_start[min((uint32_t)job.totals[0], total)] = total;  // the end of the last run
    extract_group_ranks(job.heads, total, base, s_keep, s_before);
    if (s_before[kExtractGroupWords] == 0u) return;  // (uniform)
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t local = k * 256u + t, w = local >> 5, bit = local & 31u, word = s_keep[w];
        if (!((word >> bit) & 1u)) continue;  // (the head words are clear at and above total)
        const uint32_t p = base + local;
        const uint32_t r = job.head_bases[blockIdx.x] + s_before[w] + extract_rank(word, bit);
        const uint32_t idx = job.sorted[p].z;
        if (r >= total || idx >= n) continue;  // (never)
        // the representative's rank among the representatives: its group's base, the words of the group before its own, its word
        uint32_t j = job.keep_bases[idx >> 10];
        for (uint32_t ww = (idx >> 10) << 5; ww < (idx >> 5); ++ww) j += extract_popc(job.keep[ww]);
        j += extract_rank(job.keep[idx >> 5], idx & 31u);
        job.run_start[r] = p;
        job.run_dst[r] = j;
    }
}

__global__ __launch_bounds__(256) void k_dec_map(uint64_t n, DecimateJob job) {
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    __shared__ uint32_t s_single, s_largest;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t total = min(job.nb.result[kNbCount], (uint32_t)n);
    const uint32_t base = blockIdx.x * kExtractGroup;
    if (t == 0u) {
        s_single = 0u;
        s_largest = 0u;
    }
    extract_group_ranks(job.heads, total, base, s_keep, s_before);  // (ends with a barrier)
    uint32_t single = 0, largest = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t local = k * 256u + t, w = local >> 5, bit = local & 31u, word = s_keep[w];
        const uint32_t p = base + local;
        if (p >= total) continue;
        // the heads at or before p, less one: p's run (position 0 is a head)
        const uint32_t r = job.head_bases[blockIdx.x] + s_before[w] + extract_popc(word & ((2u << bit) - 1u)) - 1u;
        if (r >= total) continue;  // (never)
        const uint32_t j = job.run_dst[r], idx = job.sorted[p].z;
        if (idx < n) job.map[idx] = j;
        if (((word >> bit) & 1u) && j < total) {
            const uint32_t len = job.run_start[r + 1u] - p;
            job.cell_start[j] = p;
            job.cell_len[j] = len;
            single += len == 1u ? 1u : 0u;
            largest = max(largest, len);
        }
    }
    single = wave_sum(single);
    largest = wave_max(largest);
    if (lane == 0u) {
        atomicAdd(&s_single, single);
        atomicMax(&s_largest, largest);
    }
    __syncthreads();
    if (t == 0u && s_largest) {  // integer add and max: the same words in any order
        atomicAdd(&job.words[kDecSingletons], s_single);
        atomicMax(&job.words[kDecLargest], s_largest);
    }
}

template <int SH, int COV>
__global__ __launch_bounds__(64) void k_dec_merge(uint64_t n_src, uint64_t n_dst, DecimateJob job, ExtractPlanes src, ExtractPlanes dst) {
    constexpr uint32_t kShWords = PodKind<SH, COV>::kShWords, kStride = PodKind<SH, COV>::kStride;
    constexpr uint32_t kRecWords = kStride ? kStride : 1u;
    __shared__ float s_v[64][kDecGeo + 2];  // a member's mass and its 13 values (15 words a row: the rows spread over the banks)
    __shared__ uint32_t s_idx[64];
    __shared__ float s_out[64];
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    if (j >= n_dst) return;
    const uint32_t len = job.cell_len[j];
    if (len < 2u) return;  // (uniform) a singleton is k_extract_scatter's copy
    const uint32_t start = job.cell_start[j];
    const uint32_t rep = job.sorted[start].z;
    if (rep >= n_src) return;  // (never)
    const uint4 pc_r = src.pc[rep];
    const float pr[3] = {__uint_as_float(pc_r.x), __uint_as_float(pc_r.y), __uint_as_float(pc_r.z)};
    float acc_m = 0.0f, acc_u = 0.0f;  // this lane's column under the mass weights and under the weight 1
    uint32_t max_a = 0;
#pragma unroll 1
    for (uint32_t cb = 0; cb < len; cb += 64u) {
        const uint32_t cnt = min(64u, len - cb);
        __syncthreads();  // the chunk before has been read
        if (lane < cnt) {
            const uint32_t i = min(job.sorted[start + cb + lane].z, (uint32_t)n_src - 1u);
            const uint4 pc = src.pc[i];
            const float p[3] = {__uint_as_float(pc.x), __uint_as_float(pc.y), __uint_as_float(pc.z)};
            float c[6], v[kDecGeo];
            pod_load_cov<COV>(src, i, c);
            uint32_t a;
            s_v[lane][0] = dec_member(p, pr, c, pc.w, v, &a);
#pragma unroll
            for (uint32_t q = 0; q < kDecGeo; ++q) s_v[lane][1u + q] = v[q];
            s_idx[lane] = i;
            max_a = max(max_a, a);
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t k0 = 0; k0 < cnt; k0 += 4u) {  // four members' loads in flight, their terms added in member order
            float m[4], v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t k = min(k0 + u, cnt - 1u);
                m[u] = s_v[k][0];
                if (lane < kDecGeo) v[u] = s_v[k][1u + lane];
                else if (SH != GSX_SH_NONE && lane < kDecColumns) v[u] = dec_load_sh<SH>(src, n_src, s_idx[k], lane - kDecGeo);
                else v[u] = 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                if (k0 + u < cnt) {
                    acc_m = dec_acc(acc_m, m[u], v[u]);
                    acc_u = dec_acc(acc_u, 1.0f, v[u]);
                }
            }
        }
    }
    max_a = wave_max(max_a);
    const float M = __shfl(acc_m, 0, 64);  // column 0 under the mass weights: W = M
    const bool mass = dec_mass(M);
    const float acc = mass ? acc_m : acc_u;
    __syncthreads();
    s_out[lane] = acc;
    __syncthreads();
    float g[kDecGeo], mu[3], cov[6], inv;
#pragma unroll
    for (uint32_t q = 0; q < kDecGeo; ++q) g[q] = s_out[q];
    uint32_t color;
    dec_finish(g, mass, M, max_a, pr, mu, cov, &color, &inv);
    uint4 g1, g2;
    pod_encode_cov<COV>(cov, g1, g2);
    const uint4 pc_out = make_uint4(__float_as_uint(mu[0]), __float_as_uint(mu[1]), __float_as_uint(mu[2]), color);
    if (lane == 0u) {
        dst.pc[j] = pc_out;
        if (COV == GSX_COV3D_SINGLE) {
            dst.cov_a[j] = g1;
            dst.cov_b[j] = make_uint2(g2.x, g2.y);
        } else {
            dst.cov_h[j] = make_uint2(g1.x, g1.y);
            dst.cov_h2[j] = g1.z;
        }
    }
    if (SH == GSX_SH_NONE) return;
    // the merged SH float f sits in lane 13 + f; lane 0 gathers the 45 and writes the words of the kind once (pod_planes.h:
    // pod_encode_sh), into the planes and, with the geometry words, into the shade record: one set of words, spare words zero
    const float shv = (lane >= kDecGeo && lane < kDecColumns) ? dec_sh(acc, inv) : 0.0f;
    __syncthreads();  // s_out has been read
    s_out[lane] = shv;
    __syncthreads();
    if (lane != 0u) return;
    float sh[48];
#pragma unroll
    for (uint32_t f = 0; f < 48u; ++f) sh[f] = f < 45u ? s_out[kDecGeo + f] : 0.0f;
    uint4 rec[kRecWords];
#pragma unroll
    for (uint32_t q = 0; q < kRecWords; ++q) rec[q] = make_uint4(0u, 0u, 0u, 0u);
    pod_encode_sh<SH>(sh, rec);
    if (SH == GSX_SH_SINGLE) {
#pragma unroll
        for (int p = 0; p < kShPlanes4; ++p) dst.sh4[(uint64_t)p * n_dst + j] = rec[p];
        dst.sh1[j] = rec[11].x;
    } else if (SH == GSX_SH_HALF) {
#pragma unroll
        for (int p = 0; p < 6; ++p) dst.sh_h[(uint64_t)p * n_dst + j] = rec[p];
    } else if (SH == GSX_SH_NORM8) {
#pragma unroll
        for (int p = 0; p < 3; ++p) dst.sh_q[(uint64_t)p * n_dst + j] = rec[p];
    }
    if (kStride != 0u) {
        rec[kShWords] = pc_out;
        rec[kShWords + 1u] = g1;
        if (COV == GSX_COV3D_SINGLE) rec[kShWords + 2u] = g2;
        uint4* out = dst.sh_aos + (uint64_t)j * kStride;
#pragma unroll
        for (uint32_t q = 0; q < kStride; ++q) out[q] = rec[q];
    }
}

hipError_t launch_decimate_order(hipStream_t s, uint64_t n, const DecimateJob& job) {
    GSX_LAUNCH(k_dec_order, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, n, job);
    GSX_LAUNCH(k_dec_sort_big, dim3(kDecSortGroups), dim3(256), 0, s, n, job);
    return hipGetLastError();
}
hipError_t launch_decimate_cells(hipStream_t s, uint64_t n, const DecimateJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_dec_heads, dim3(groups), dim3(256), 0, s, n, job);
    GSX_LAUNCH(k_dec_popc, dim3(groups), dim3(64), 0, s, n, job.keep, job.keep_partials);
    hipError_t e = launch_extract_scan(s, job.head_partials, groups, job.head_bases, job.totals);
    if (e != hipSuccess) return e;
    if ((e = launch_extract_scan(s, job.keep_partials, groups, job.keep_bases, job.totals + 1)) != hipSuccess) return e;
    GSX_LAUNCH(k_dec_runs, dim3(groups), dim3(256), 0, s, n, job);
    GSX_LAUNCH(k_dec_map, dim3(groups), dim3(256), 0, s, n, job);
    return hipGetLastError();
}
hipError_t launch_decimate_merge(hipStream_t s, int sh_kind, int cov_kind, uint64_t n_src, uint64_t n_dst, const DecimateJob& job, const ExtractPlanes& src,
                                 const ExtractPlanes& dst) {
    return dispatch_pod_kind(sh_kind, cov_kind, [&](auto sh, auto cov) {
        GSX_LAUNCH((k_dec_merge<decltype(sh)::value, decltype(cov)::value>), dim3((uint32_t)n_dst), dim3(64), 0, s, n_src, n_dst, job, src, dst);
        return hipGetLastError();
    });
}

}  // namespace gsx
