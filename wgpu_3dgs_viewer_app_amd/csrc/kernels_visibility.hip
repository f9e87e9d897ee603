// kernels_visibility.hip — per-Gaussian visibility from a camera for gfx950 (spec/RENDER_SPEC.md section 24; gsx_model_visibility,
// gsx_model_select_visibility).
//
// k_vis_tiles   one 128-lane workgroup per 16x16 tile, two pixels a lane, the tile's COMPLETE front-to-back list staged through LDS
//               128 records at a time: k_composite's shape (kernels_composite.hip) and, per pixel, its operation sequence for q, the
//               support test, alpha, w = T * alpha and T — packed f32, no contraction — without the colour.  What the compositor
//               throws away is kept per Gaussian: the maximum of w (as the bits of a non-negative float, which order like the
//               floats), the sum of round_to_nearest(w * 2^24) and the count of the pixels that blended it.  Per record, a wave
//               that has a hit reduces the three over its 64 lanes (wave_reduce.h; the count from two ballots) and ONE lane issues
//               atomicMax (u32), atomicAdd (u64) and atomicAdd (u32) into the model's planes; a wave without a hit does none of it.
//               Integer atomics only: a maximum and integer sums do not depend on the order, so every call returns the same bytes.
// k_vis_stats   n_seen and peak_max over the resident planes: group_fold, then one atomic a workgroup (integers again).
// k_vis_select  one compare per Gaussian on the resident planes; the selection is written by selection_write.h.
#include <algorithm>

#include "gsx_internal.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {

constexpr int kVisBatch = 128;  // records staged through LDS per barrier pair (k_composite's)

typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f splat2(float x) { return v2f{x, x}; }
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }  // v_pk_fma_f32

// w as the planes keep it: the bits of the float for the maximum, round_to_nearest(w * 2^24) for the sum.  w <= 1 (T <= 1 and
// alpha <= 1), so the fixed-point value is at most 2^24 and a wave's 128 of them fit 32 bits.  A w that is not above 0 (0, a negative
// or NaN product of records no frame should hold) counts as 0 in both.
__device__ __forceinline__ uint32_t vis_bits(float w) { return w > 0.0f ? __float_as_uint(w) : 0u; }
__device__ __forceinline__ uint32_t vis_fixed(float w) { return w > 0.0f ? (uint32_t)rintf(fminf(w, 1.0f) * 16777216.0f) : 0u; }

}  // namespace

template <int MODE /* 0 splat (gaussian falloff), 1 constant alpha inside the cutoff */, bool CLAMP /* alpha_max < 1 or alpha_min > 0 */>
__global__ __launch_bounds__(128) void k_vis_tiles(const FrameConsts f, const uint2* __restrict__ ranges, const uint32_t* __restrict__ list,
                                                    const float4* __restrict__ rec_a, const float4* __restrict__ rec_b, const VisPlanes planes,
                                                    float* __restrict__ transmittance, uint32_t* __restrict__ words) {
    __shared__ float2 s_mean[kVisBatch];
    __shared__ float4 s_conic[kVisBatch];  // (a, 2b, c, opacity)
    __shared__ uint32_t s_idx[kVisBatch];

    const uint32_t tile = blockIdx.x;
    const uint32_t tx = tile % f.tiles_x, ty = tile / f.tiles_x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t px = tx * kTile + (tid & 15u), py = ty * kTile + 2u * (tid >> 4);
    const bool in0 = px < f.w_px && py < f.h_px, in1 = px < f.w_px && py + 1u < f.h_px;
    const float pxf = (float)px + 0.5f;
    const v2f pyf = v2f{(float)py + 0.5f, (float)(py + 1u) + 0.5f};
    const uint2 range = ranges[tile];
    const size_t fbo = (size_t)py * f.w_px + px;

    v2f T = splat2(1.0f);
    // the support test `!done && 0 <= q <= k2` as one unsigned compare per pixel (k_composite)
    const uint32_t live = f.k2 > 0.0f ? __float_as_uint(f.k2) + 1u : (f.k2 == 0.0f ? 1u : 0u);
    uint32_t lim0 = (in0 && !(T.x < f.t_eps)) ? live : 0u, lim1 = (in1 && !(T.y < f.t_eps)) ? live : 0u;
    unsigned long long my_pairs = 0ull, my_weight = 0ull;  // this wave's, in lane 0

    // software pipeline: the gather of batch b + 1 (list -> two record planes) is in flight while batch b is walked out of LDS
    const float4 pad_a = make_float4(3.0e38f, 3.0e38f, 0.0f, 0.0f), pad_b = make_float4(1.0f, 0.0f, 1.0f, 0.0f);
    float4 pa = pad_a, pb = pad_b;
    uint32_t pidx = 0u;
    if (range.x + tid < range.y) {
        pidx = list[range.x + tid];
        pa = rec_a[pidx];
        pb = rec_b[pidx];
    }
    for (uint32_t base = range.x; base < range.y; base += kVisBatch) {
        // vote + barrier: also protects the LDS batch of the previous iteration
        if (__syncthreads_and((lim0 | lim1) == 0u)) break;
        s_mean[tid] = make_float2(pa.x, pa.y);
        s_conic[tid] = make_float4(pb.x, 2.0f * pb.y, pb.z, pb.w);
        s_idx[tid] = pidx;
        __syncthreads();
        {
            const uint32_t nxt = base + kVisBatch + tid;
            pa = pad_a;
            pb = pad_b;
            pidx = 0u;
            if (nxt < range.y) {
                pidx = list[nxt];
                pa = rec_a[pidx];
                pb = rec_b[pidx];
            }
        }
        const uint32_t cnt = min((uint32_t)kVisBatch, range.y - base);
        for (uint32_t j = 0; j < cnt; ++j) {
            if ((j & 3u) == 0u && !__ballot((lim0 | lim1) != 0u)) break;  // every pixel of the wave is closed
            const float2 m = s_mean[j];
            const float4 co = s_conic[j];
            const float dx = pxf - m.x;
            const v2f dy = pyf - splat2(m.y);
            // q = fma(a*dx, dx, fma(c*dy, dy, ((2b)*dx)*dy))
            const v2f q = fma2(splat2(co.x * dx), splat2(dx), fma2(splat2(co.z) * dy, dy, splat2(co.y * dx) * dy));
            const bool h0 = __float_as_uint(q.x) < lim0, h1 = __float_as_uint(q.y) < lim1;
            if (!__ballot(h0 || h1)) continue;  // (wave-uniform: no pixel of the wave supports the record)
            v2f alpha;
            if (MODE == 0) {
                const v2f e = splat2(-0.72134752044448170368f) * q;
                alpha = splat2(co.w) * v2f{__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
            } else {
                alpha = splat2(co.w * 1.0f);
            }
            bool b0 = h0, b1 = h1;  // the pixel blends the record
            if (CLAMP) {
                alpha.x = fminf(f.alpha_max, alpha.x);
                alpha.y = fminf(f.alpha_max, alpha.y);
                b0 = h0 && !(alpha.x < f.alpha_min);
                b1 = h1 && !(alpha.y < f.alpha_min);
            }
            // a pixel that is not hit takes alpha = 0: w = 0 and T * (1 - 0) = T, bit for bit (k_composite leaves such a lane alone)
            alpha.x = b0 ? alpha.x : 0.0f;
            alpha.y = b1 ? alpha.y : 0.0f;
            const v2f wgt = T * alpha;
            T = T * (splat2(1.0f) - alpha);
            // only a blend lowers T, so T < t_eps here means saturated now or before
            lim0 = T.x < f.t_eps ? 0u : lim0;
            lim1 = T.y < f.t_eps ? 0u : lim1;
            const uint32_t pairs = (uint32_t)__popcll(__ballot(b0)) + (uint32_t)__popcll(__ballot(b1));
            if (pairs == 0u) continue;  // (wave-uniform: alpha_min removed every hit; every w is 0)
            const uint32_t peak = wave_max(max(vis_bits(wgt.x), vis_bits(wgt.y)));
            const uint32_t fixed = wave_sum(vis_fixed(wgt.x) + vis_fixed(wgt.y));
            if (lane == 0u) {
                const uint32_t g = s_idx[j];
                atomicMax(&planes.peak[g], peak);
                atomicAdd(&planes.weight[g], (unsigned long long)fixed);
                atomicAdd(&planes.pixels[g], pairs);
                my_pairs += pairs;
                my_weight += fixed;
            }
        }
    }
    if (transmittance) {
        if (in0) transmittance[fbo] = T.x;
        if (in1) transmittance[fbo + f.w_px] = T.y;
    }
    if (lane == 0u && my_pairs) {
        atomicAdd(reinterpret_cast<unsigned long long*>(words + kVisPairs), my_pairs);
        atomicAdd(reinterpret_cast<unsigned long long*>(words + kVisWeight), my_weight);
    }
}

namespace {
struct VisStatsPartial {
    uint32_t seen, peak;
};
}  // namespace

__global__ __launch_bounds__(256) void k_vis_stats(uint64_t n, const uint32_t* __restrict__ peak, uint32_t* __restrict__ words) {
    uint32_t seen = 0u, mx = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t p = peak[i];
        seen += p != 0u ? 1u : 0u;
        mx = max(mx, p);
    }
    const VisStatsPartial p = group_fold(VisStatsPartial{wave_sum(seen), wave_max(mx)}, [](VisStatsPartial a, const VisStatsPartial& b) {
        return VisStatsPartial{a.seen + b.seen, a.peak > b.peak ? a.peak : b.peak};
    });
    if (threadIdx.x == 0u && p.seen) {
        atomicAdd(&words[kVisSeen], p.seen);
        atomicMax(&words[kVisPeakMax], p.peak);
    }
}

// One workgroup of 256 per 1024 Gaussians (extract_groups), one partial each: the resident measure of every Gaussian that passes the
// filter against [lo, hi] in double — a float peak, a weight below 2^53 / 2^24 and a 32-bit count are exact there.
__global__ __launch_bounds__(256) void k_vis_select(uint64_t n, ModelFilter f, VisSelectJob job) {
    const uint32_t t = threadIdx.x;
    SelectCounts counts;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (base + k * 256u >= n) break;  // (uniform: the round holds no Gaussian)
        const bool keep = prop_keep(f, n, i, t);
        double x = 0.0;
        if (keep) {
            if (job.measure == (uint32_t)GSX_VIS_PEAK) x = (double)__uint_as_float(job.planes.peak[i]);
            else if (job.measure == (uint32_t)GSX_VIS_WEIGHT) x = (double)job.planes.weight[i] * (1.0 / 16777216.0);
            else x = (double)job.planes.pixels[i];
        }
        select_write(job.sel, keep && x >= job.lo && x <= job.hi, i, n, counts);
    }
    select_store_partial(job.sel, counts);
}

hipError_t launch_vis_tiles(hipStream_t s, const FrameConsts& f, const uint2* ranges, const uint32_t* list, const Records& rec, const VisPlanes& planes,
                            float* transmittance, uint32_t* words) {
    const uint32_t tiles = f.tiles_x * f.tiles_y;
    if (!tiles) return hipSuccess;
    const dim3 grid(tiles), block(128);
    const bool clamp = f.alpha_max < 1.0f || f.alpha_min > 0.0f;  // (launch_composite's rule: the default constants need no clamping)
#define GSX_V(M, C) GSX_LAUNCH((k_vis_tiles<M, C>), grid, block, 0, s, f, ranges, list, rec.a, rec.b, planes, transmittance, words)
    if (f.display_mode == GSX_DISPLAY_SPLAT) { if (clamp) GSX_V(0, true); else GSX_V(0, false); }
    else { if (clamp) GSX_V(1, true); else GSX_V(1, false); }
#undef GSX_V
    return hipGetLastError();
}

hipError_t launch_vis_stats(hipStream_t s, uint64_t n, const VisPlanes& planes, uint32_t* words) {
    if (n == 0) return hipSuccess;
    const uint32_t groups = (uint32_t)std::min<uint64_t>((n + 255u) / 256u, 2048u);
    GSX_LAUNCH(k_vis_stats, dim3(groups), dim3(256), 0, s, n, planes.peak, words);
    return hipGetLastError();
}

hipError_t launch_vis_select(hipStream_t s, uint64_t n, const ModelFilter& f, const VisSelectJob& job) {
    if (n == 0) return hipSuccess;
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_vis_select, dim3(groups), dim3(256), 0, s, n, f, job);
    return launch_select_finish(s, job.sel, groups, job.words + kVisHit, job.words + kVisSelected);
}

}  // namespace gsx
