// kernels_clusters.hip — the model clusters for gfx950 (spec/RENDER_SPEC.md §19, "Model clusters"): gsx_model_clusters and
// gsx_model_select_clusters.  The grid is section 18's (kernels_neighbors.hip: reduce, cell, scan, scatter), unchanged; on top of it:
//   k_cl_init    parent[i] = i for every Gaussian (the region section 18 calls counts);
//   k_cl_hook    one lane per record, in bucket order, walks the 27 cells around its own as k_nb_query does (neighbors_grid.h:
//                nb_walk, with its own-cell test).  No cap, no early exit.  A record within the radius whose original index is
//                below the lane's own is united with the lane's: each unordered pair once.  The union-find is clusters_math.h's,
//                lock-free: nobody waits for anybody;
//   k_cl_label   a separate launch, index order: label[i] = cl_find(i), or 0xFFFFFFFF for a Gaussian that does not participate;
//                size[label] is counted by non-returning adds, combined first over the wave and, for the workgroup's smallest
//                label, over the workgroup; with seeds, a plain store of 1 to seeded[label] for a selected participant (every
//                writer stores the same value);
//   k_cl_stats   index order: sizes[i] = size[label[i]]; the clusters are the Gaussians with label[i] == i, the largest one the
//                maximum of (size << 32) | ~label — the smallest label wins a tie; one partial a workgroup, k_cl_finish combines them;
//   k_cl_select  k_nb_select's shape with the hit test of the mode; the write, the partial and its sum are selection_write.h's.
// Memory model: every access to parent[] in k_cl_hook and k_cl_label is a relaxed agent-scope atomic (load, compare-and-swap, min),
// which the L2-private XCDs resolve at the memory side; a CU's L1 is never asked.  No lane polls for another's progress: there is no
// flag and no spin on a word somebody else must write.  A stale parent value is an older link of the same tree (clusters_math.h), the
// compare-and-swap acts on the word itself, and what one launch wrote is visible to the next by the stream's order.
// Every cross-workgroup combination is an integer add or maximum: the same bits in any order.  Offsets are 64-bit where they scale
// with n x 16.  Nothing of the model but the selection (k_cl_select) is written.  Bounds: a record's original index is checked
// against n before it indexes parent[], a bucket's end against the participant count before the walk, a label against n before it
// indexes size[] or seeded[].
#include "gsx_internal.h"
#include "clusters_math.h"
#include "neighbors_grid.h"
#include "neighbors_math.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
// parent[] through relaxed agent-scope atomics: clusters_math.h's three primitives
struct ClParent {
    uint32_t* parent;
    __device__ uint32_t load(uint32_t i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) const { return atomicCAS(parent + i, expect, v); }
    __device__ void min(uint32_t i, uint32_t v) const { atomicMin(parent + i, v); }  // (the value is not used: non-returning)
};

// What k_cl_stats leaves per workgroup and k_cl_finish combines: the clusters' count and the largest one's key, in thread 0.
struct ClPartial {
    uint32_t clusters;
    uint64_t key;
};
__device__ inline ClPartial cl_fold(uint32_t clusters, uint64_t key) {
    return group_fold(ClPartial{wave_sum(clusters), wave_max(key)},
                      [](ClPartial a, const ClPartial& b) { return ClPartial{a.clusters + b.clusters, b.key > a.key ? b.key : a.key}; });
}
}  // namespace

__global__ __launch_bounds__(256) void k_cl_init(uint64_t n, uint32_t* __restrict__ parent) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_cl_hook(uint64_t n, NeighborJob job) {
    const NbFrame g = nb_frame(job);
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= g.total) return;
    const float r2 = job.r2;
    const uint4 self = job.records[p];
    if (self.w >= n) return;  // (never: the scatter wrote an index below n)
    const float px = __uint_as_float(self.x), py = __uint_as_float(self.y), pz = __uint_as_float(self.z);
    ClParent parent{job.counts};
    nb_walk(g, job, nb_cell3(g, self), [&](const uint4& r, const NbVisit& v) {
        // the index first: the pair belongs to the lane with the larger index (and a record is not its own pair)
        if (r.w < self.w && nb_d2(px, py, pz, __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z)) <= r2 && v.holds(r))
            cl_union(parent, self.w, r.w);
        return true;  // (no cap, no early exit)
    });
}

// Index order, kExtractGroup Gaussians a workgroup in four rounds.  The sizes are counted in three steps, because the common model is
// ONE large cluster and ten million adds on one word take 113 ms (measured; DESIGN section 4, "Model clusters"): the workgroup's
// smallest label — the large cluster's, whose label is a small index, where the workgroup holds any of it — is counted in LDS and
// leaves as one add a workgroup; every other label is counted over the wave by ballots and leaves as one add per wave and label.
__global__ __launch_bounds__(256) void k_cl_label(uint64_t n, ClusterJob job) {
    __shared__ uint32_t s_lowest, s_count;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    if (t == 0u) {
        s_lowest = kClNone;
        s_count = 0u;
    }
    __syncthreads();
    ClParent parent{job.nb.counts};
    uint32_t l[4], lowest = kClNone;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        l[k] = kClNone;
        if (i < n) {
            const uint32_t bit = t & 31u;
            if ((job.nb.participants[i >> 5] >> bit) & 1u) {
                const uint32_t root = cl_find(parent, (uint32_t)i);
                if (root < n) {  // (always)
                    l[k] = root;
                    if (job.seeds && job.nb.sel.valid && ((job.nb.sel.words[i >> 5] >> bit) & 1u)) job.seeded[root] = 1u;
                }
            }
            job.label[i] = l[k];
        }
        lowest = min(lowest, l[k]);
    }
    lowest = wave_min(lowest);
    if (lane == 0u && lowest != kClNone) atomicMin(&s_lowest, lowest);  // (LDS)
    __syncthreads();
    const uint32_t common = s_lowest;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const bool part = l[k] != kClNone;
        const unsigned long long in_common = __ballot(part && l[k] == common);
        if (lane == 0u && in_common) atomicAdd(&s_count, (uint32_t)__popcll(in_common));  // (LDS)
        bool pending = part && l[k] != common;
        for (unsigned long long todo = __ballot(pending); todo; todo = __ballot(pending)) {  // (uniform over the wave: once per label)
            const uint32_t first = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t lab = (uint32_t)__shfl((int)l[k], (int)first, 64);
            const unsigned long long same = __ballot(pending && l[k] == lab);
            if (lane == first) atomicAdd(&job.size[lab], (uint32_t)__popcll(same));  // (the value is not used: a non-returning add)
            pending = pending && l[k] != lab;
        }
    }
    __syncthreads();
    if (t == 0u && s_count) atomicAdd(&job.size[common], s_count);  // (s_count > 0: common is a label below n)
}

__global__ __launch_bounds__(256) void k_cl_stats(uint64_t n, ClusterJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    uint32_t clusters = 0;
    uint64_t key = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        const uint32_t l = job.label[i];
        uint32_t s = 0;
        if (l < n) {
            s = job.size[l];
            if (l == (uint32_t)i) {
                clusters += 1u;
                const uint64_t mine = ((uint64_t)s << 32) | (uint32_t)~l;
                key = mine > key ? mine : key;
            }
        }
        job.sizes[i] = s;
    }
    const ClPartial p = cl_fold(clusters, key);
    if (t == 0u) {
        // ONE partial per workgroup, plain stores ("Model properties": atomics on a few words cost more than the stream)
        uint32_t* out = job.nb.partials + (size_t)blockIdx.x * kNbPartialWords;
        out[0] = p.clusters;
        out[2] = (uint32_t)p.key;
        out[3] = (uint32_t)(p.key >> 32);
    }
}

// One workgroup: the partials of k_cl_stats combined into the result block.
__global__ __launch_bounds__(256) void k_cl_finish(const uint32_t* __restrict__ partials, uint32_t n_partials, uint32_t* __restrict__ result) {
    const uint32_t t = threadIdx.x;
    uint32_t clusters = 0;
    uint64_t key = 0;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const uint32_t* in = partials + (size_t)j * kNbPartialWords;
        clusters += in[0];
        const uint64_t theirs = ((uint64_t)in[3] << 32) | in[2];
        key = theirs > key ? theirs : key;
    }
    const ClPartial p = cl_fold(clusters, key);
    if (t != 0u) return;
    result[kClClusters] = p.clusters;
    result[kClKey] = (uint32_t)p.key;
    result[kClKey + 1u] = (uint32_t)(p.key >> 32);
}

__global__ __launch_bounds__(256) void k_cl_select(uint64_t n, ClusterJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const uint32_t largest = ~job.nb.result[kClKey];  // (0xFFFFFFFF without participants: no label below n equals it)
    SelectCounts counts;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool hit = false;
        if (i < n) {
            const uint32_t l = job.label[i];
            if (l < n) {  // participates
                if (job.mode == kClBySize) {
                    const uint32_t s = job.sizes[i];
                    hit = s >= job.size_lo && s <= job.size_hi;
                } else if (job.mode == kClLargest) {
                    hit = l == largest;
                } else {
                    hit = job.seeded[l] != 0u;
                }
            }
        }
        select_write(job.nb.sel, hit, i, n, counts);
    }
    select_store_partial(job.nb.sel, counts);
}

hipError_t launch_clusters_hook(hipStream_t s, uint64_t n, const ClusterJob& job) {
    const uint32_t blocks = (uint32_t)((n + 255u) / 256u);
    GSX_LAUNCH(k_cl_init, dim3(blocks), dim3(256), 0, s, n, job.nb.counts);
    GSX_LAUNCH(k_cl_hook, dim3(blocks), dim3(256), 0, s, n, job.nb);
    return hipGetLastError();
}
hipError_t launch_clusters_label(hipStream_t s, uint64_t n, const ClusterJob& job) {
    GSX_LAUNCH(k_cl_label, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, n, job);
    return hipGetLastError();
}
hipError_t launch_clusters_stats(hipStream_t s, uint64_t n, const ClusterJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_cl_stats, dim3(groups), dim3(256), 0, s, n, job);
    GSX_LAUNCH(k_cl_finish, dim3(1), dim3(256), 0, s, job.nb.partials, groups, job.nb.result);
    return hipGetLastError();
}
hipError_t launch_clusters_select(hipStream_t s, uint64_t n, const ClusterJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_cl_select, dim3(groups), dim3(256), 0, s, n, job);
    return launch_select_finish(s, job.nb.sel, groups, job.nb.result + kNbHit, job.nb.result + kNbSelected);
}

}  // namespace gsx
