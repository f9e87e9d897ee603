// shade_quads.h — shading of the admitted records of a lazily projected frame, four lanes to a record.  Build-internal, device code.
//
// One body, two homes: the stand-alone kernel k_shade_quads (kernels_project.hip: the serial order) and the rider workgroups of the
// depth sort's launches (kernels_sort.hip: k_msd_sweep / k_bucket_sort, speculated frames).  Nothing between the compaction and the
// compositor reads the conic / colour records, so on a speculated frame the pass rides beside kernels that are a few hundred
// workgroups waiting on look-backs: the same instructions on the same inputs, only where and when they run changes.
#pragma once
#include <hip/hip_fp16.h>

#include "gsx_internal.h"
#include "pod_quant.h"  // h_lo, h_hi, dq_snorm8
#include "project_math.h"

namespace gsx {

// k_shade for the 256-byte record copy (f32 SH + f32 covariance), four lanes to a record.  One record per lane meant sixteen 16-byte
// loads 256 bytes apart from lane to lane: every load instruction touched 64 different lines, a wave's working set was 16 KB of a
// 32 KB L1 shared by eight waves, and the sectors were fetched again and again (75 MB of records in 41 us: 1.8 TB/s).  Here the
// four lanes of a quad load the record side by side — lane s takes words s, s + 4, s + 8, s + 12: every instruction reads whole
// 64-byte sectors, sixteen sectors a wave — and hand each other their words by quad broadcasts (v_mov_dpp: no LDS, no barrier).
// All four lanes then run the SAME arithmetic on the same sixteen words — the code of k_shade, value for value — and lane 0 stores.
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v, const int s) {
    // quad_perm [s, s, s, s]
    switch (s) {
        case 0: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x00, 0xF, 0xF, false);
        case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xF, 0xF, false);
        case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xF, 0xF, false);
        default: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xF, 0xF, false);
    }
}
// the SH words of a shade record (plane order, as the pod stores them) -> the stream's floats: what load_shade<.., AOS = true> feeds
template <int DEG, int SHK>
__device__ __forceinline__ void feed_record_words(ShStream<DEG>& st, const uint4* w) {
    constexpr int kFloats = ShNeed<DEG>::floats;
    if (SHK == GSX_SH_SINGLE) {
#pragma unroll
        for (int p = 0; p < ShNeed<DEG>::planes4; ++p) {
            st.feed(4 * p, __uint_as_float(w[p].x)); st.feed(4 * p + 1, __uint_as_float(w[p].y));
            st.feed(4 * p + 2, __uint_as_float(w[p].z)); st.feed(4 * p + 3, __uint_as_float(w[p].w));
        }
        if (DEG == 3) st.feed(44, __uint_as_float(w[11].x));
    } else if (SHK == GSX_SH_HALF) {
        constexpr int kP = (kFloats + 7) / 8;
#pragma unroll
        for (int p = 0; p < kP; ++p) {
            st.feed(8 * p, h_lo(w[p].x)); st.feed(8 * p + 1, h_hi(w[p].x)); st.feed(8 * p + 2, h_lo(w[p].y)); st.feed(8 * p + 3, h_hi(w[p].y));
            st.feed(8 * p + 4, h_lo(w[p].z)); st.feed(8 * p + 5, h_hi(w[p].z)); st.feed(8 * p + 6, h_lo(w[p].w)); st.feed(8 * p + 7, h_hi(w[p].w));
        }
    } else {
        constexpr int kP = (kFloats + 15) / 16;
#pragma unroll
        for (int p = 0; p < kP; ++p) {
            const uint32_t q[4] = {w[p].x, w[p].y, w[p].z, w[p].w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) st.feed(16 * p + 4 * k + bb, dq_snorm8(q[k], bb));
        }
    }
}

// Four lanes to a shade record, every pod kind (round 5; f32 pods since round 4): the quad loads the record side by side — STRIDE / 4
// coalesced 16-byte loads per lane, whole 64-byte sectors — and every lane gets every word by quad broadcasts.
// The calling lane's quad shades pairs[first], pairs[first + stride], ... below `end`; skip (nullable): ballots of the records that
// are shaded already (repair round: what the first round admitted).  threadIdx.x & 3 is the lane's place in its quad.
template <int DEG, int SHK, int COVK>
__device__ __forceinline__ void shade_quads(const FrameConsts& f, const PodPlanes& pod, const Records& rec, const uint2* __restrict__ pairs,
                                            const unsigned long long* __restrict__ skip, const int write_a, const uint32_t first,
                                            const uint32_t end, const uint32_t stride) {
    constexpr uint32_t kStride = SHK == GSX_SH_SINGLE ? 16u : (SHK == GSX_SH_HALF ? (COVK == GSX_COV3D_SINGLE ? 12u : 8u) : 8u);
    constexpr uint32_t kGeo = SHK == GSX_SH_SINGLE ? 12u : (SHK == GSX_SH_HALF ? 6u : 3u);
    constexpr int kLoads = (int)(kStride / 4u);
    const uint32_t sub = threadIdx.x & 3u;
    // One pass over a record is a chain of three round trips — its index, its record, its stores — and a quad that walks them one
    // after the other is latency, not bandwidth (as a rider it has four waves a SIMD to hide them behind, not seven).  So three records
    // are under way at a time: the index of the one after next is loaded and the next one's record is on its way while this one's
    // arithmetic runs.  Per record the loads, the arithmetic and the stores are what they were.
    auto index_of = [&](uint32_t j, uint32_t& i) -> bool {   // (the quad's four lanes share j)
        if (j >= end) return false;
        i = pairs[j].y;
        return !(skip && ((skip[i >> 6] >> (i & 63u)) & 1ull));
    };
    auto load_record = [&](uint32_t i, uint4 (&mine)[kLoads]) {
#pragma unroll
        for (int k = 0; k < kLoads; ++k) mine[k] = pod.sh_aos[(uint64_t)i * kStride + sub + 4u * (uint32_t)k];
    };
    auto shade_record = [&](uint32_t i, const uint4 (&mine)[kLoads]) {
        uint4 w[kStride];   // the record's words, in every lane of the quad
#pragma unroll
        for (int k = 0; k < kLoads; ++k)
#pragma unroll
            for (int sl = 0; sl < 4; ++sl)
                w[sl + 4 * k] = make_uint4(quad_bcast(mine[k].x, sl), quad_bcast(mine[k].y, sl), quad_bcast(mine[k].z, sl), quad_bcast(mine[k].w, sl));
        const float4 pc = make_float4(__uint_as_float(w[kGeo].x), __uint_as_float(w[kGeo].y), __uint_as_float(w[kGeo].z), __uint_as_float(w[kGeo].w));
        ViewClip vc;
        Splat2D sp{};
        if (!pm_view_cull(f, pc.x, pc.y, pc.z, vc)) return;  // cannot happen: it is visible
        if (COVK == GSX_COV3D_SINGLE) {
            if (!pm_cov2d_rect(f, vc, __uint_as_float(w[kGeo + 1].x), __uint_as_float(w[kGeo + 1].y), __uint_as_float(w[kGeo + 1].z), __uint_as_float(w[kGeo + 1].w),
                               __uint_as_float(w[kGeo + 2].x), __uint_as_float(w[kGeo + 2].y), sp))
                return;
        } else {
            const uint4 a = w[kGeo + 1];
            if (!pm_cov2d_rect(f, vc, h_lo(a.x), h_hi(a.x), h_lo(a.y), h_hi(a.y), h_lo(a.z), h_hi(a.z), sp)) return;
        }
        ShStream<DEG> st;   // (load_shade<DEG, SHK, true>, fed from registers)
        st.begin(f, pc.x, pc.y, pc.z, __float_as_uint(pc.w));
        feed_record_words<DEG, SHK>(st, w);
        float r, g, b;
        st.finish(r, g, b);
        if (sub == 0u) {
            if (write_a) rec.a[i] = make_float4(sp.mx, sp.my, __uint_as_float(sp.rx), __uint_as_float(sp.ry));
            rec.b[i] = make_float4(sp.con_a, sp.con_b, sp.con_c, (float)(__float_as_uint(pc.w) >> 24) * (1.0f / 255.0f));
            rec.c[i] = make_float4(r, g, b, vc.d);
        }
    };
    uint32_t i_now = 0u, i_next = 0u;
    uint4 rec_now[kLoads] = {}, rec_next[kLoads] = {};
    const bool live_first = index_of(first, i_now);
    if (live_first) load_record(i_now, rec_now);
    bool live_now = live_first, live_next = index_of(first + stride, i_next);
    for (uint32_t j = first; j < end; j += stride) {
        if (live_next) load_record(i_next, rec_next);
        uint32_t i_after = 0u;
        const bool live_after = index_of(j + 2u * stride, i_after);
        if (live_now) shade_record(i_now, rec_now);
        i_now = i_next;
        live_now = live_next;
#pragma unroll
        for (int k = 0; k < kLoads; ++k) rec_now[k] = rec_next[k];
        i_next = i_after;
        live_next = live_after;
    }
}

// ---- riders: workgroups appended behind a carrier kernel's own (blockIdx.x >= own) whose only job is the body above ----
// A rider takes no ticket, touches no status word of its carrier and never waits; it reads the compaction's output (only .y, in any
// order), which no kernel between the compaction and the compositor of a speculated frame overwrites.  The carrier is a template
// on the rider: NoRide leaves the kernel what it was.
// (struct ShadeRide: gsx_internal.h)
struct NoRide {
    static constexpr bool active = false;
    using Args = uint32_t;   // (a placeholder the kernel does not read)
};
template <int DEG, int SHK, int COVK>
struct ShadeRider {
    static constexpr bool active = true;
    using Args = ShadeRide;
    static __device__ __forceinline__ void run(const Args& r) {
        const uint32_t count = *r.d_n;
        const uint32_t j0 = (uint32_t)(((uint64_t)count * r.lo) >> 8), j1 = (uint32_t)(((uint64_t)count * r.hi) >> 8);
        const uint32_t quads = blockDim.x >> 2;
        shade_quads<DEG, SHK, COVK>(r.f, r.pod, r.rec, r.pairs, r.skip, (int)r.write_a, j0 + (blockIdx.x - r.own) * quads + (threadIdx.x >> 2), j1,
                                    (gridDim.x - r.own) * quads);
    }
};
// calls fn(ShadeRider<DEG, SHK, COVK>{}) for the pod's instantiation
template <class F>
inline void shade_rider_dispatch(const FrameConsts& f, const PodPlanes& pod, F&& fn) {
    const bool ch = pod.cov_kind == GSX_COV3D_HALF;
#define GSX_RIDER_DEG(SHK, COVK)                                  \
    switch ((int)f.sh_deg) {                                      \
        case 0: fn(ShadeRider<0, SHK, COVK>{}); break;            \
        case 1: fn(ShadeRider<1, SHK, COVK>{}); break;            \
        case 2: fn(ShadeRider<2, SHK, COVK>{}); break;            \
        default: fn(ShadeRider<3, SHK, COVK>{}); break;           \
    }
    if (pod.sh_kind == GSX_SH_SINGLE) {
        if (ch) { GSX_RIDER_DEG(GSX_SH_SINGLE, GSX_COV3D_HALF) } else { GSX_RIDER_DEG(GSX_SH_SINGLE, GSX_COV3D_SINGLE) }
    } else if (pod.sh_kind == GSX_SH_HALF) {
        if (ch) { GSX_RIDER_DEG(GSX_SH_HALF, GSX_COV3D_HALF) } else { GSX_RIDER_DEG(GSX_SH_HALF, GSX_COV3D_SINGLE) }
    } else {
        if (ch) { GSX_RIDER_DEG(GSX_SH_NORM8, GSX_COV3D_HALF) } else { GSX_RIDER_DEG(GSX_SH_NORM8, GSX_COV3D_SINGLE) }
    }
#undef GSX_RIDER_DEG
}

}  // namespace gsx
