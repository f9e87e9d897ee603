// kernels_bounds.hip — gsx_model_bounds for gfx950 (spec/RENDER_SPEC.md §11, "Model bounds"): the box, the centre and the
// centroid of a model's Gaussian centres, and the trimmed box, from the resident position plane (`pc`, 16 B per Gaussian).
//   k_bounds_reduce   streams the plane like k_mask_evaluate does (256 lanes, four non-temporal 16-byte loads per lane in flight
//                     before any arithmetic), decides the filter from the bit planes, keeps min / max / counts / a float64 sum per
//                     lane and leaves ONE partial per workgroup;
//   k_bounds_finish   one workgroup: combines the partials in index order and writes the result;
//   k_bounds_hist     (trim_permille > 0) the same stream again: a 2048-bin histogram per axis over [min, max], accumulated in
//                     LDS with integer atomics and flushed with integer atomics — order-independent, so exact;
//   k_bounds_trim     one workgroup, one wave per axis and end: the bin where the cumulative count first exceeds k.
// No floating-point atomics anywhere: the result is the same bits from run to run.  The histogram's arithmetic is bounds_math.h.
#include "gsx_internal.h"

namespace gsx {

// Gaussians per lane and chunk, 256 apart.  On 10 M Gaussians 2 and 4 are level and 8 is 11 % slower (DESIGN §4 "Model bounds",
// variants; profiles/r09_bench_bounds.txt)
constexpr uint32_t kBoundsPerLane = 4;
constexpr uint32_t kBoundsChunk = 256u * kBoundsPerLane;    // Gaussians per workgroup and chunk

__device__ inline float4 bd_ld_stream(const float4* p) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// One chunk's loads of one lane: the positions and the words of the bit planes that are present (a word serves 32 lanes: the
// 32 loads of one address are one request).  Everything is issued before the first verdict.
struct BoundsLoads {
    float4 p[kBoundsPerLane];
    uint32_t mask[kBoundsPerLane], sel[kBoundsPerLane], edited[kBoundsPerLane];
};
__device__ inline void bd_load(const float4* __restrict__ pc, uint64_t n, const ModelFilter& f, uint64_t base, BoundsLoads* L) {
#pragma unroll
    for (uint32_t k = 0; k < kBoundsPerLane; ++k) {
        const uint64_t i = base + k * 256u;
        const bool in = i < n;  // indices >= n never count, whatever the tail bits of a word say
        L->p[k] = in ? bd_ld_stream(pc + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        L->mask[k] = (in && f.mask) ? f.mask[i >> 5] : 0xFFFFFFFFu;
        L->sel[k] = (in && f.selection) ? f.selection[i >> 5] : 0xFFFFFFFFu;
        L->edited[k] = (in && f.edited) ? f.edited[i >> 5] : 0u;
    }
}
// does Gaussian i = base + k * 256 pass the filter?  (the edit flag word is read only where the `edited` bit is set)
__device__ inline bool bd_keep(const ModelFilter& f, uint64_t n, uint64_t base, uint32_t k, const BoundsLoads& L) {
    const uint64_t i = base + k * 256u;
    const uint32_t b = (uint32_t)i & 31u;
    bool keep = i < n && ((L.mask[k] >> b) & 1u) && ((L.sel[k] >> b) & 1u);
    if (keep && ((L.edited[k] >> b) & 1u)) keep = !extract_flag_hides(__float_as_uint(f.edit_a[i].x));
    return keep;
}

__device__ inline void bd_merge(BoundsPartial* a, const BoundsPartial& b) {  // a, then b: the order of the float64 sums
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a->mn[c] = fminf(a->mn[c], b.mn[c]);
        a->mx[c] = fmaxf(a->mx[c], b.mx[c]);
        a->sum[c] += b.sum[c];
    }
    a->count += b.count;
    a->nonfinite += b.nonfinite;
}
__device__ inline BoundsPartial bd_identity() {
    BoundsPartial a;
    for (int c = 0; c < 3; ++c) {
        a.mn[c] = INFINITY;
        a.mx[c] = -INFINITY;
        a.sum[c] = 0.0;
    }
    a.count = a.nonfinite = 0;
    return a;
}

__global__ __launch_bounds__(256) void k_bounds_reduce(const float4* __restrict__ pc, uint64_t n, ModelFilter f,
                                                        BoundsPartial* __restrict__ partials) {
    BoundsPartial acc = bd_identity();
    const uint64_t chunks = (n + kBoundsChunk - 1) / kBoundsChunk;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t base = c * kBoundsChunk + threadIdx.x;
        BoundsLoads L;
        bd_load(pc, n, f, base, &L);
#pragma unroll
        for (uint32_t k = 0; k < kBoundsPerLane; ++k) {
            if (!bd_keep(f, n, base, k, L)) continue;
            const float4 p = L.p[k];
            if (bounds_finite(p.x) && bounds_finite(p.y) && bounds_finite(p.z)) {
                acc.mn[0] = fminf(acc.mn[0], p.x); acc.mx[0] = fmaxf(acc.mx[0], p.x);
                acc.mn[1] = fminf(acc.mn[1], p.y); acc.mx[1] = fmaxf(acc.mx[1], p.y);
                acc.mn[2] = fminf(acc.mn[2], p.z); acc.mx[2] = fmaxf(acc.mx[2], p.z);
                acc.sum[0] += (double)p.x; acc.sum[1] += (double)p.y; acc.sum[2] += (double)p.z;
                acc.count += 1;
            } else {
                acc.nonfinite += 1;
            }
        }
    }
    // across the wave: butterflies (a + b == b + a bit for bit, so every lane ends with the same value); across the workgroup:
    // the four wave results through LDS, merged in wave order by one lane.  No atomics.
#pragma unroll
    for (uint32_t off = 32; off >= 1; off >>= 1) {
        BoundsPartial o;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o.mn[c] = __shfl_xor(acc.mn[c], off);
            o.mx[c] = __shfl_xor(acc.mx[c], off);
            o.sum[c] = __shfl_xor(acc.sum[c], off);
        }
        o.count = __shfl_xor(acc.count, off);
        o.nonfinite = __shfl_xor(acc.nonfinite, off);
        bd_merge(&acc, o);
    }
    __shared__ BoundsPartial waves[4];
    if ((threadIdx.x & 63u) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        BoundsPartial r = waves[0];
        for (int w = 1; w < 4; ++w) bd_merge(&r, waves[w]);
        partials[blockIdx.x] = r;
    }
}

// One workgroup.  Lane t merges its run of consecutive partials in index order, then neighbours are merged pairwise (t with t + 1,
// t with t + 2, ...): left operand first at every step, so the whole is the partials in index order under one fixed bracketing.
// It also clears the histogram the trimmed passes are about to fill.
__global__ __launch_bounds__(256) void k_bounds_finish(const BoundsPartial* __restrict__ partials, uint32_t n_partials, uint32_t clear_hist,
                                                        gsx_model_bounds_t* __restrict__ out, uint32_t* __restrict__ hist) {
    __shared__ BoundsPartial acc[256];
    const uint32_t t = threadIdx.x, per = (n_partials + 255u) / 256u;
    BoundsPartial a = bd_identity();
    for (uint32_t r0 = 0; r0 < per; r0 += 8u) {
        BoundsPartial run[8];  // eight of the run's loads are issued before the first of them is merged
#pragma unroll
        for (uint32_t r = 0; r < 8u; ++r) {
            const uint32_t j = t * per + r0 + r;
            run[r] = (r0 + r < per && j < n_partials) ? partials[j] : bd_identity();
        }
#pragma unroll
        for (uint32_t r = 0; r < 8u; ++r) bd_merge(&a, run[r]);
    }
    acc[t] = a;
    if (clear_hist)
        for (uint32_t j = t; j < 3u * kBoundsBins; j += 256u) hist[j] = 0u;
    __syncthreads();
    for (uint32_t s = 1; s < 256u; s <<= 1) {
        if ((t & (2u * s - 1u)) == 0) bd_merge(&acc[t], acc[t + s]);
        __syncthreads();
    }
    if (t == 0) {
        const BoundsPartial r = acc[0];
        gsx_model_bounds_t o;
        o.count = r.count;
        o.n_nonfinite = r.nonfinite;
        if (r.count == 0) {
            bounds_empty(o.min);
        } else {
            for (int c = 0; c < 3; ++c) {
                o.min[c] = o.trim_min[c] = r.mn[c];
                o.max[c] = o.trim_max[c] = r.mx[c];
                o.center[c] = 0.5f * (r.mn[c] + r.mx[c]);
                o.mean[c] = (float)(r.sum[c] / (double)r.count);
            }
        }
        *out = o;
    }
}

// The histogram pass: the same stream and the same verdicts as k_bounds_reduce; the bins live in LDS (24 KiB per workgroup).
__global__ __launch_bounds__(256) void k_bounds_hist(const float4* __restrict__ pc, uint64_t n, ModelFilter f,
                                                      const gsx_model_bounds_t* __restrict__ res, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[3u * kBoundsBins];
    if (res->count == 0) return;  // (uniform)
    BoundsAxis ax[3];
    for (int c = 0; c < 3; ++c) ax[c] = bounds_axis(res->min[c], res->max[c]);
    if (!ax[0].live && !ax[1].live && !ax[2].live) return;
    for (uint32_t j = threadIdx.x; j < 3u * kBoundsBins; j += 256u) bins[j] = 0u;
    __syncthreads();
    const uint64_t chunks = (n + kBoundsChunk - 1) / kBoundsChunk;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t base = c * kBoundsChunk + threadIdx.x;
        BoundsLoads L;
        bd_load(pc, n, f, base, &L);
#pragma unroll
        for (uint32_t k = 0; k < kBoundsPerLane; ++k) {
            if (!bd_keep(f, n, base, k, L)) continue;
            const float4 p = L.p[k];
            if (!(bounds_finite(p.x) && bounds_finite(p.y) && bounds_finite(p.z))) continue;
            if (ax[0].live) atomicAdd(&bins[bounds_bin(ax[0], p.x)], 1u);
            if (ax[1].live) atomicAdd(&bins[kBoundsBins + bounds_bin(ax[1], p.y)], 1u);
            if (ax[2].live) atomicAdd(&bins[2u * kBoundsBins + bounds_bin(ax[2], p.z)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < 3u * kBoundsBins; j += 256u) {
        const uint32_t cnt = bins[j];
        if (cnt) atomicAdd(&hist[j], cnt);
    }
}

// One workgroup of six waves: wave w scans axis w / 2 from its low end (w even) or its high end (w odd).  A lane sums 32 bins in
// scan order, the wave takes the prefix sums, and the first lane whose prefix exceeds k finds the bin among its 32 (bounds_scan).
// Axes without a histogram keep the min / max k_bounds_finish wrote.
constexpr uint32_t kBoundsScanPerLane = kBoundsBins / 64u;
__global__ __launch_bounds__(384) void k_bounds_trim(const uint32_t* __restrict__ hist, uint32_t trim_permille, gsx_model_bounds_t* out) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, axis = wave >> 1;
    const bool reverse = (wave & 1u) != 0;
    const uint64_t count = out->count;
    if (count == 0) return;
    const BoundsAxis ax = bounds_axis(out->min[axis], out->max[axis]);
    if (!ax.live) return;  // (uniform per wave; nothing below synchronises the workgroup)
    const uint64_t k = bounds_trim_k(count, trim_permille);
    // this lane's 32 bins: scan positions [32 lane, 32 lane + 32), i.e. ascending indices from 32 lane, or descending from bins - 1 - 32 lane
    const uint32_t* seg = hist + axis * kBoundsBins + (reverse ? kBoundsBins - kBoundsScanPerLane * (lane + 1u) : kBoundsScanPerLane * lane);
    uint64_t own = 0;
    for (uint32_t j = 0; j < kBoundsScanPerLane; ++j) own += seg[j];
    uint64_t incl = own;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint64_t up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    const unsigned long long found = __ballot(incl > k);
    if (found == 0ull) return;  // (k < count: cannot happen)
    if (lane != (uint32_t)__ffsll((long long)found) - 1u) return;
    uint64_t before;
    const uint32_t pos = kBoundsScanPerLane * lane + bounds_scan(seg, kBoundsScanPerLane, reverse, k - (incl - own), &before);
    if (reverse) out->trim_max[axis] = bounds_trim_hi(ax, pos);
    else out->trim_min[axis] = bounds_trim_lo(ax, pos);
}

// at most kBoundsMaxGroups workgroups, and every one of them the same number of chunks (but for the last few, one fewer)
uint32_t bounds_reduce_groups(uint64_t n) {
    const uint64_t chunks = (n + kBoundsChunk - 1) / kBoundsChunk, rounds = (chunks + kBoundsMaxGroups - 1) / kBoundsMaxGroups;
    return rounds ? (uint32_t)((chunks + rounds - 1) / rounds) : 0u;
}

hipError_t launch_bounds_reduce(hipStream_t s, const float4* pc, uint64_t n, const ModelFilter& f, BoundsPartial* partials) {
    GSX_LAUNCH(k_bounds_reduce, dim3(bounds_reduce_groups(n)), dim3(256), 0, s, pc, n, f, partials);
    return hipGetLastError();
}
hipError_t launch_bounds_finish(hipStream_t s, const BoundsPartial* partials, uint32_t n_partials, bool clear_hist, gsx_model_bounds_t* out,
                                uint32_t* hist) {
    GSX_LAUNCH(k_bounds_finish, dim3(1), dim3(256), 0, s, partials, n_partials, clear_hist ? 1u : 0u, out, hist);
    return hipGetLastError();
}
hipError_t launch_bounds_trim(hipStream_t s, const float4* pc, uint64_t n, const ModelFilter& f, uint32_t trim_permille,
                              gsx_model_bounds_t* out, uint32_t* hist) {
    // fewer, longer-lived workgroups than the reduction: each flushes up to 3 x 2048 bins with global atomics
    const uint32_t groups = (uint32_t)std::min<uint64_t>((n + kBoundsChunk - 1) / kBoundsChunk, kBoundsHistGroups);
    GSX_LAUNCH(k_bounds_hist, dim3(groups), dim3(256), 0, s, pc, n, f, out, hist);
    GSX_LAUNCH(k_bounds_trim, dim3(1), dim3(384), 0, s, hist, trim_permille, out);
    return hipGetLastError();
}

}  // namespace gsx
