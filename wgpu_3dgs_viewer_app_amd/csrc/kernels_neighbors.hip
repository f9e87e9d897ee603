// kernels_neighbors.hip — the neighbour counts for gfx950 (spec/RENDER_SPEC.md §18, "Model neighbours"): gsx_model_neighbors and
// gsx_model_select_neighbors.  A hashed uniform grid, built by a counting sort, in six passes on one stream:
//   k_nb_reduce   index order: a Gaussian participates if it passes the filter (prop_keep: ModelFilter + extract_keep_word) and its
//                 three stored coordinates are finite; count, non-finite count and the minimum per axis, one partial a workgroup;
//                 k_nb_finish (one workgroup) combines them: the minimum is the grid's origin;
//   k_nb_cell     index order: the participant bits (a wave ballot, two words), the cell (neighbors_math.h: nb_cell) and its bucket,
//                 one non-returning integer add into the bucket's table word; counts[i] = 0 for every Gaussian;
//   k_nb_scan_*   the table's sizes become starts: block sums, the one-workgroup scan of gsx_model_extract over them
//                 (k_extract_scan), then the exclusive scan of every block plus its base, in place;
//   k_nb_scatter  index order: a participant draws its slot with ONE returning add on its bucket's table word and stores a 16-byte
//                 record (x, y, z bits, original index) there: the word that held the bucket's start ends as the bucket's end, which
//                 is the start of the next bucket, so the table needs no second copy.  The order inside a bucket depends on the
//                 order of the adds; no result does (a count is a sum over the bucket, a saturated count min(sum, cap));
//   k_nb_query    one lane per record, in bucket order, so a wave's lanes share cells: the 27 cells around the lane's own, for each
//                 the bucket it hashes to, walked from start to end.  A record counts if d2 <= r2, it is not the lane's own and its
//                 own cell IS the visited cell — two of the 27 cells that share a bucket would otherwise count it twice.  The lane
//                 stops at max_count.  The count goes to counts[original index], and into the workgroup's LDS bins (up to 4096
//                 words, non-returning LDS adds), which leave as non-returning global adds of the non-zero bins;
//   k_nb_select   index order: 64 counts are balloted into the wave's two selection words; lanes 0 and 32 apply the op, clear the
//                 tail, store, and count hit and selected bits: one partial a workgroup, k_nb_finish combines them.
// Every cross-workgroup combination is an integer add or a minimum of finite floats: the same bits in any order.  Built with
// -ffp-contract=off.  Offsets are 64-bit where they scale with n x 16.  Nothing of the model but the selection (k_nb_select) is
// written.  Bounds: a record slot is checked against n before the store, a bucket's end against the participant count before the walk.
#include "gsx_internal.h"
#include "neighbors_math.h"

namespace gsx {

namespace {
enum : uint32_t { kNbModeReduce = 0, kNbModeSelect = 1 };
static_assert(kNbMaxCount + 1u <= 4096u, "the query's LDS bins");
static_assert(kNbScanBlock == 4u * 256u, "four table words a lane");

__device__ inline uint32_t nb_wave_sum(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ inline float nb_wave_min(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o, 64));
    return x;
}
constexpr float kNbInf = __builtin_huge_valf();

// The workgroup's partial from its lanes' values: sums of a0, a1, minima of m0..m2 (finite floats or +inf).
__device__ inline void nb_store_partial(uint32_t* __restrict__ partials, uint32_t a0, uint32_t a1, float m0, float m1, float m2) {
    __shared__ uint32_t s_part[4][5];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    a0 = nb_wave_sum(a0);
    a1 = nb_wave_sum(a1);
    m0 = nb_wave_min(m0);
    m1 = nb_wave_min(m1);
    m2 = nb_wave_min(m2);
    if (lane == 0u) {
        s_part[wave][0] = a0; s_part[wave][1] = a1;
        s_part[wave][2] = __float_as_uint(m0); s_part[wave][3] = __float_as_uint(m1); s_part[wave][4] = __float_as_uint(m2);
    }
    __syncthreads();
    if (t == 0u) {
        for (uint32_t w = 1; w < 4u; ++w) {
            a0 += s_part[w][0];
            a1 += s_part[w][1];
            m0 = fminf(m0, __uint_as_float(s_part[w][2]));
            m1 = fminf(m1, __uint_as_float(s_part[w][3]));
            m2 = fminf(m2, __uint_as_float(s_part[w][4]));
        }
        // ONE partial per workgroup, plain stores ("Model properties": atomics on a few words cost more than the stream)
        uint32_t* p = partials + (size_t)blockIdx.x * kNbPartialWords;
        p[0] = a0; p[1] = a1; p[2] = __float_as_uint(m0); p[3] = __float_as_uint(m1); p[4] = __float_as_uint(m2);
    }
}
}  // namespace

__global__ __launch_bounds__(256) void k_nb_reduce(uint64_t n, ModelFilter f, const uint4* __restrict__ pc, uint32_t* __restrict__ partials) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    uint32_t count = 0, nonfinite = 0;
    float mx = kNbInf, my = kNbInf, mz = kNbInf;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform: the round holds no Gaussian)
        const uint64_t i = base + k * 256u + t;
        if (prop_keep(f, n, i, t)) {  // (every lane of the wave makes the call: a ballot inside)
            const uint4 e = pc[i];
            const float x = __uint_as_float(e.x), y = __uint_as_float(e.y), z = __uint_as_float(e.z);
            if (nb_finite(x) && nb_finite(y) && nb_finite(z)) {
                count += 1u;
                mx = fminf(mx, x);
                my = fminf(my, y);
                mz = fminf(mz, z);
            } else {
                nonfinite += 1u;
            }
        }
    }
    nb_store_partial(partials, count, nonfinite, mx, my, mz);
}

// One workgroup: the partials combined into the result block's words of the mode.
__global__ __launch_bounds__(256) void k_nb_finish(uint32_t mode, const uint32_t* __restrict__ partials, uint32_t n_partials, uint32_t* __restrict__ result) {
    __shared__ uint32_t s_out[kNbPartialWords];
    const uint32_t t = threadIdx.x;
    uint32_t a0 = 0, a1 = 0;
    float m0 = kNbInf, m1 = kNbInf, m2 = kNbInf;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const uint32_t* p = partials + (size_t)j * kNbPartialWords;
        a0 += p[0];
        a1 += p[1];
        if (mode == kNbModeReduce) {
            m0 = fminf(m0, __uint_as_float(p[2]));
            m1 = fminf(m1, __uint_as_float(p[3]));
            m2 = fminf(m2, __uint_as_float(p[4]));
        }
    }
    nb_store_partial(s_out, a0, a1, m0, m1, m2);  // (blockIdx.x is 0: the partial lands at s_out[0..4])
    if (t != 0u) return;
    if (mode == kNbModeReduce) {
        result[kNbCount] = s_out[0];
        result[kNbNonfinite] = s_out[1];
        result[kNbOrigin + 0] = s_out[2];
        result[kNbOrigin + 1] = s_out[3];
        result[kNbOrigin + 2] = s_out[4];
    } else {
        result[kNbHit] = s_out[0];
        result[kNbSelected] = s_out[1];
    }
}

__global__ __launch_bounds__(256) void k_nb_cell(uint64_t n, ModelFilter f, const uint4* __restrict__ pc, NeighborJob job) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const float ox = __uint_as_float(job.result[kNbOrigin + 0]), oy = __uint_as_float(job.result[kNbOrigin + 1]),
                oz = __uint_as_float(job.result[kNbOrigin + 2]);
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool part = prop_keep(f, n, i, t);
        if (part) {
            const uint4 e = pc[i];
            const float x = __uint_as_float(e.x), y = __uint_as_float(e.y), z = __uint_as_float(e.z);
            part = nb_finite(x) && nb_finite(y) && nb_finite(z);
            if (part) {
                const uint32_t b = nb_bucket(nb_cell(x, ox, job.inv_h), nb_cell(y, oy, job.inv_h), nb_cell(z, oz, job.inv_h), job.bits);
                atomicAdd(&job.table[b], 1u);  // (the value is not used: a non-returning add)
            }
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
    __shared__ uint32_t s_wave[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t at = blockIdx.x * kNbScanBlock + 4u * t;
    uint32_t own = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
        if (at + q < words) own += table[at + q];
    own = nb_wave_sum(own);
    if (lane == 0u) s_wave[wave] = own;
    __syncthreads();
    if (t == 0u) sums[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
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
    const float ox = __uint_as_float(job.result[kNbOrigin + 0]), oy = __uint_as_float(job.result[kNbOrigin + 1]),
                oz = __uint_as_float(job.result[kNbOrigin + 2]);
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        if (!((job.participants[i >> 5] >> (t & 31u)) & 1u)) continue;
        const uint4 e = pc[i];
        const float x = __uint_as_float(e.x), y = __uint_as_float(e.y), z = __uint_as_float(e.z);
        const uint32_t b = nb_bucket(nb_cell(x, ox, job.inv_h), nb_cell(y, oy, job.inv_h), nb_cell(z, oz, job.inv_h), job.bits);
        const uint32_t slot = atomicAdd(&job.table[b], 1u);  // the bucket's next free slot; the word ends as the bucket's end
        if (slot < n) job.records[slot] = make_uint4(e.x, e.y, e.z, (uint32_t)i);
    }
}

__global__ __launch_bounds__(256) void k_nb_query(uint64_t n, NeighborJob job) {
    __shared__ uint32_t s_bins[kNbMaxCount + 1u];
    const uint32_t t = threadIdx.x;
    const uint32_t bins = job.max_count + 1u;
    for (uint32_t j = t; j < bins; j += 256u) s_bins[j] = 0u;
    __syncthreads();
    const uint32_t total = job.result[kNbCount];
    const uint32_t p = blockIdx.x * 256u + t;
    if (p < total) {
        const float ox = __uint_as_float(job.result[kNbOrigin + 0]), oy = __uint_as_float(job.result[kNbOrigin + 1]),
                    oz = __uint_as_float(job.result[kNbOrigin + 2]);
        const float r2 = job.r2, inv_h = job.inv_h;
        const uint4 self = job.records[p];
        const float px = __uint_as_float(self.x), py = __uint_as_float(self.y), pz = __uint_as_float(self.z);
        const uint32_t cx = nb_cell(px, ox, inv_h), cy = nb_cell(py, oy, inv_h), cz = nb_cell(pz, oz, inv_h);
        const uint32_t cap = job.max_count;
        uint32_t cnt = 0;
#pragma unroll 1
        for (uint32_t c = 0; c < 27u && cnt < cap; ++c) {
            // (a coordinate below 0 wraps above kNbMaxCell: there is no such cell)
            const uint32_t vx = cx + (c % 3u) - 1u, vy = cy + ((c / 3u) % 3u) - 1u, vz = cz + (c / 9u) - 1u;
            if (vx > kNbMaxCell || vy > kNbMaxCell || vz > kNbMaxCell) continue;
            const uint32_t b = nb_bucket(vx, vy, vz, job.bits);
            uint32_t q = b ? job.table[b - 1u] : 0u;
            const uint32_t end = min(job.table[b], total);
#pragma unroll 1
            for (; q < end && cnt < cap; ++q) {
                const uint4 r = job.records[q];
                const float rx = __uint_as_float(r.x), ry = __uint_as_float(r.y), rz = __uint_as_float(r.z);
                if (nb_d2(px, py, pz, rx, ry, rz) <= r2 && r.w != self.w) {
                    if (nb_cell(rx, ox, inv_h) == vx && nb_cell(ry, oy, inv_h) == vy && nb_cell(rz, oz, inv_h) == vz) cnt += 1u;
                }
            }
        }
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
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    uint32_t hit_count = 0, selected = 0;  // lanes 0 and 32 of a wave
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k * 256u >= n) break;  // (uniform)
        const uint64_t i = base + k * 256u + t;
        bool hit = false;
        if (i < n && ((job.participants[i >> 5] >> (t & 31u)) & 1u)) {
            const uint32_t c = job.counts[i];
            hit = c >= job.count_lo && c <= job.count_hi;
        }
        const unsigned long long hits64 = __ballot(hit);
        if ((lane & 31u) == 0u && i < n) {  // this lane reads and writes the word of its 32: no other wave touches it
            const uint64_t w = i >> 5;
            const uint32_t hits = (uint32_t)(hits64 >> lane);
            const uint32_t old = job.selection_valid ? job.selection[w] : 0u;
            const uint32_t now = (job.op == (uint32_t)GSX_SELECTION_SET ? hits : (job.op == (uint32_t)GSX_SELECTION_ADD ? (old | hits) : (old & ~hits))) &
                                 extract_tail_mask(n, w);
            job.selection[w] = now;
            hit_count += extract_popc(hits);
            selected += extract_popc(now);
        }
    }
    nb_store_partial(job.partials, hit_count, selected, kNbInf, kNbInf, kNbInf);
}

hipError_t launch_neighbors_reduce(hipStream_t s, uint64_t n, const ModelFilter& f, const uint4* pc, const NeighborJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_nb_reduce, dim3(groups), dim3(256), 0, s, n, f, pc, job.partials);
    GSX_LAUNCH(k_nb_finish, dim3(1), dim3(256), 0, s, (uint32_t)kNbModeReduce, job.partials, groups, job.result);
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
    GSX_LAUNCH(k_nb_finish, dim3(1), dim3(256), 0, s, (uint32_t)kNbModeSelect, job.partials, groups, job.result);
    return hipGetLastError();
}

}  // namespace gsx
