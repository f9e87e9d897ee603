// kernels_depthmap.hip — the splats' depth per pixel for gfx950 (spec/RENDER_SPEC.md section 25; gsx_render_depth_map).
//
// k_depth_tiles   one 128-lane workgroup per 16x16 tile, two pixels a lane, the tile's COMPLETE front-to-back list staged through LDS
//                 128 records at a time: k_vis_tiles' shape (kernels_visibility.hip) and, per pixel, the compositor's operation
//                 sequence for q, the support test, alpha, w = T * alpha and T — packed f32, no contraction.  What it keeps is per
//                 PIXEL, so there is no wave reduction and no atomic: A += w, S = fma(w, d, S) with d the record's view depth (the
//                 float whose bits are its depth key — the key plane is resident for every Gaussian, rec.c only where something shaded
//                 it), and the first record after whose blend T < threshold (its depth, its Gaussian index; the layer is the launch's).
//                 One launch a model, nearest model first; every launch but the first (FIRST) starts from the planes the one before
//                 left.  A pixel that has crossed keeps threshold = -inf, so `T < threshold` is the whole crossing test.
// k_depth_finish  over the finished planes: the optional NDC plane, and the call's statistics — counts and the minimum / maximum of
//                 the bits of positive floats, folded per workgroup, then one integer atomic each: the same bytes on every call.
#include <algorithm>
#include <cmath>

#include "gsx_internal.h"
#include "wave_reduce.h"

namespace gsx {

namespace {

constexpr int kDepthBatch = 128;  // records staged through LDS per barrier pair (k_composite's, k_vis_tiles')

typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f splat2(float x) { return v2f{x, x}; }
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }  // v_pk_fma_f32

}  // namespace

template <int MODE /* 0 splat (gaussian falloff), 1 constant alpha inside the cutoff */, bool CLAMP /* alpha_max < 1 or alpha_min > 0 */,
          bool FIRST /* the nearest model: the pixels start at T = 1, A = S = 0, no crossing */>
__global__ __launch_bounds__(128) void k_depth_tiles(const FrameConsts f, const uint2* __restrict__ ranges, const uint32_t* __restrict__ list,
                                                      const float4* __restrict__ rec_a, const float4* __restrict__ rec_b,
                                                      const uint32_t* __restrict__ rec_key, const DepthMapPlanes planes, const float threshold,
                                                      const uint32_t layer) {
    __shared__ float2 s_mean[kDepthBatch];
    __shared__ float4 s_conic[kDepthBatch];  // (a, 2b, c, opacity)
    __shared__ float s_depth[kDepthBatch];
    __shared__ uint32_t s_idx[kDepthBatch];

    const uint32_t tile = blockIdx.x;
    const uint32_t tx = tile % f.tiles_x, ty = tile / f.tiles_x;
    const uint32_t tid = threadIdx.x;
    const uint32_t px = tx * kTile + (tid & 15u), py = ty * kTile + 2u * (tid >> 4);
    const bool in0 = px < f.w_px && py < f.h_px, in1 = px < f.w_px && py + 1u < f.h_px;
    const float pxf = (float)px + 0.5f;
    const v2f pyf = v2f{(float)py + 0.5f, (float)(py + 1u) + 0.5f};
    const uint2 range = ranges[tile];
    const size_t o0 = (size_t)py * f.w_px + px, o1 = o0 + f.w_px;

    // a model behind continues from what the planes hold.  (A tile without entries leaves them as they are: nothing is read or written.)
    if (!FIRST && range.x >= range.y) return;
    v2f T = splat2(1.0f), A = splat2(0.0f), S = splat2(0.0f), thr = splat2(threshold);
    if (!FIRST) {
        if (in0) {
            T.x = planes.transmittance[o0];
            A.x = planes.alpha[o0];
            S.x = planes.sum[o0];
            if (planes.layer[o0] != kDepthMapNone) thr.x = -INFINITY;
        }
        if (in1) {
            T.y = planes.transmittance[o1];
            A.y = planes.alpha[o1];
            S.y = planes.sum[o1];
            if (planes.layer[o1] != kDepthMapNone) thr.y = -INFINITY;
        }
    }
    const bool open0 = thr.x == threshold, open1 = thr.y == threshold;  // no crossing in front of this launch
    float surf0 = INFINITY, surf1 = INFINITY;
    uint32_t idx0 = kDepthMapNone, idx1 = kDepthMapNone;
    // the support test `!done && 0 <= q <= k2` as one unsigned compare per pixel (k_composite)
    const uint32_t live = f.k2 > 0.0f ? __float_as_uint(f.k2) + 1u : (f.k2 == 0.0f ? 1u : 0u);
    uint32_t lim0 = (in0 && !(T.x < f.t_eps)) ? live : 0u, lim1 = (in1 && !(T.y < f.t_eps)) ? live : 0u;

    // software pipeline: the gather of batch b + 1 (list -> key plane and two record planes) is in flight while batch b is walked out of LDS
    const float4 pad_a = make_float4(3.0e38f, 3.0e38f, 0.0f, 0.0f), pad_b = make_float4(1.0f, 0.0f, 1.0f, 0.0f);
    float4 pa = pad_a, pb = pad_b;
    uint32_t pidx = 0u, pkey = 0u;
    if (range.x + tid < range.y) {
        pidx = list[range.x + tid];
        pa = rec_a[pidx];
        pb = rec_b[pidx];
        pkey = rec_key[pidx];
    }
    for (uint32_t base = range.x; base < range.y; base += kDepthBatch) {
        // vote + barrier: also protects the LDS batch of the previous iteration.  (A closed pixel has crossed: threshold >= t_epsilon.)
        if (__syncthreads_and((lim0 | lim1) == 0u)) break;
        s_mean[tid] = make_float2(pa.x, pa.y);
        s_conic[tid] = make_float4(pb.x, 2.0f * pb.y, pb.z, pb.w);
        s_depth[tid] = __uint_as_float(pkey);
        s_idx[tid] = pidx;
        __syncthreads();
        {
            const uint32_t nxt = base + kDepthBatch + tid;
            pa = pad_a;
            pb = pad_b;
            pidx = 0u;
            pkey = 0u;
            if (nxt < range.y) {
                pidx = list[nxt];
                pa = rec_a[pidx];
                pb = rec_b[pidx];
                pkey = rec_key[pidx];
            }
        }
        const uint32_t cnt = min((uint32_t)kDepthBatch, range.y - base);
        for (uint32_t j = 0; j < cnt; ++j) {
            if ((j & 3u) == 0u && !__ballot((lim0 | lim1) != 0u)) break;  // every pixel of the wave is closed
            const float2 m = s_mean[j];
            const float4 co = s_conic[j];
            const float dx = pxf - m.x;
            const v2f dy = pyf - splat2(m.y);
            // q = fma(a*dx, dx, fma(c*dy, dy, ((2b)*dx)*dy))
            const v2f q = fma2(splat2(co.x * dx), splat2(dx), fma2(splat2(co.z) * dy, dy, splat2(co.y * dx) * dy));
            const bool h0 = __float_as_uint(q.x) < lim0, h1 = __float_as_uint(q.y) < lim1;
            if (!__ballot(h0 || h1)) continue;  // (wave-uniform: no pixel of the wave supports the record; T, A and S stay)
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
            // a pixel that is not hit takes alpha = 0: w = 0, A + 0 = A, fma(0, d, S) = S (d is finite) and T * (1 - 0) = T, bit for bit
            alpha.x = b0 ? alpha.x : 0.0f;
            alpha.y = b1 ? alpha.y : 0.0f;
            const v2f wgt = T * alpha;
            T = T * (splat2(1.0f) - alpha);
            const float d = s_depth[j];
            A = A + wgt;
            S = fma2(wgt, splat2(d), S);
            // only a blend lowers T, so T < t_eps here means saturated now or before — and T < thr: this record took it across
            lim0 = T.x < f.t_eps ? 0u : lim0;
            lim1 = T.y < f.t_eps ? 0u : lim1;
            const bool c0 = T.x < thr.x, c1 = T.y < thr.y;
            if (__ballot(c0 || c1)) {  // (wave-uniform; once per pixel)
                const uint32_t g = s_idx[j];
                surf0 = c0 ? d : surf0;
                surf1 = c1 ? d : surf1;
                idx0 = c0 ? g : idx0;
                idx1 = c1 ? g : idx1;
                thr.x = c0 ? -INFINITY : thr.x;
                thr.y = c1 ? -INFINITY : thr.y;
            }
        }
    }
    // rows of 16 pixels: a wave writes 8 runs of 64 bytes per plane
    if (in0) {
        planes.transmittance[o0] = T.x;
        planes.alpha[o0] = A.x;
        planes.sum[o0] = S.x;
        const bool crossed = open0 && thr.x != threshold;
        if (FIRST || crossed) {
            planes.surface[o0] = surf0;
            planes.index[o0] = idx0;
            planes.layer[o0] = crossed ? layer : kDepthMapNone;
        }
    }
    if (in1) {
        planes.transmittance[o1] = T.y;
        planes.alpha[o1] = A.y;
        planes.sum[o1] = S.y;
        const bool crossed = open1 && thr.y != threshold;
        if (FIRST || crossed) {
            planes.surface[o1] = surf1;
            planes.index[o1] = idx1;
            planes.layer[o1] = crossed ? layer : kDepthMapNone;
        }
    }
}

namespace {
struct DepthStatsPartial {
    uint32_t covered, crossed, lo, hi;
};
}  // namespace

// npx < 2^32 (the call refuses more).  ndc: nullable.  surface > 0 wherever there is a crossing (a depth key of a visible record), so
// its bits order like the floats.
__global__ __launch_bounds__(256) void k_depth_finish(uint32_t npx, const DepthMapPlanes planes, float* __restrict__ ndc, float p22, float p23,
                                                       uint32_t* __restrict__ words) {
    uint32_t covered = 0u, crossed = 0u, lo = 0xFFFFFFFFu, hi = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < npx; i += (uint64_t)gridDim.x * 256u) {
        const bool x = planes.layer[i] != kDepthMapNone;
        const float s = planes.surface[i];
        covered += planes.alpha[i] > 0.0f ? 1u : 0u;
        crossed += x ? 1u : 0u;
        if (x) {
            lo = min(lo, __float_as_uint(s));
            hi = max(hi, __float_as_uint(s));
        }
        if (ndc) ndc[i] = x ? fminf(fmaxf(p23 / s - p22, 0.0f), 1.0f) : 1.0f;
    }
    const DepthStatsPartial p =
        group_fold(DepthStatsPartial{wave_sum(covered), wave_sum(crossed), wave_min(lo), wave_max(hi)}, [](DepthStatsPartial a, const DepthStatsPartial& b) {
            return DepthStatsPartial{a.covered + b.covered, a.crossed + b.crossed, a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi};
        });
    if (threadIdx.x == 0u && (p.covered | p.crossed)) {
        atomicAdd(&words[kDepthMapCovered], p.covered);
        atomicAdd(&words[kDepthMapCrossed], p.crossed);
        atomicMax(&words[kDepthMapMin], ~p.lo);  // (the minimum, kept inverted: the words start as zeros)
        atomicMax(&words[kDepthMapMax], p.hi);
    }
}

hipError_t launch_depth_tiles(hipStream_t s, const FrameConsts& f, const uint2* ranges, const uint32_t* list, const Records& rec,
                              const DepthMapPlanes& planes, float threshold, uint32_t layer, bool first) {
    const uint32_t tiles = f.tiles_x * f.tiles_y;
    if (!tiles) return hipSuccess;
    const dim3 grid(tiles), block(128);
    const bool clamp = f.alpha_max < 1.0f || f.alpha_min > 0.0f;  // (launch_composite's rule: the default constants need no clamping)
#define GSX_D(M, C, F) GSX_LAUNCH((k_depth_tiles<M, C, F>), grid, block, 0, s, f, ranges, list, rec.a, rec.b, rec.key, planes, threshold, layer)
#define GSX_DF(M, C) do { if (first) GSX_D(M, C, true); else GSX_D(M, C, false); } while (0)
    if (f.display_mode == GSX_DISPLAY_SPLAT) { if (clamp) GSX_DF(0, true); else GSX_DF(0, false); }
    else { if (clamp) GSX_DF(1, true); else GSX_DF(1, false); }
#undef GSX_DF
#undef GSX_D
    return hipGetLastError();
}

hipError_t launch_depth_finish(hipStream_t s, uint64_t npx, const DepthMapPlanes& planes, float* ndc, float p22, float p23, uint32_t* words) {
    if (npx == 0) return hipSuccess;
    const uint32_t groups = (uint32_t)std::min<uint64_t>((npx + 255u) / 256u, 2048u);
    GSX_LAUNCH(k_depth_finish, dim3(groups), dim3(256), 0, s, (uint32_t)npx, planes, ndc, p22, p23, words);
    return hipGetLastError();
}

}  // namespace gsx
