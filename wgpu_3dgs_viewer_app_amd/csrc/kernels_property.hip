// kernels_property.hip — the model properties for gfx950 (spec/RENDER_SPEC.md §17, "Model properties"): gsx_model_property_values,
// gsx_model_histogram and gsx_model_select_range.  ONE kernel frame over the model, k_property<CLS, MODE>:
//   a workgroup of 256 takes chunks of kExtractGroup = 1024 consecutive Gaussians (grid stride), four rounds of 256 a chunk, one
//   lane per Gaussian; a wave's 64 Gaussians are two whole words of every bit plane.  A lane decides the filter from the shared
//   ModelFilter planes (prop_keep: extract_keep_word, the hidden word from a wave ballot as in k_extract_keep), computes its value
//   (property_math.h) and then, by MODE:
//     kPropValues  stores it (no filter: every Gaussian);
//     kPropReduce  count / non-finite count / min and max as order-preserving integer keys, for an AUTO_RANGE histogram;
//     kPropHist    the same four and below / above, and the bin counted in LDS (uint32 counters, up to 4096 = 16 KiB), flushed with
//                  non-returning global integer adds of the non-zero counters;
//     kPropSelect  decides the lane's hit; the write into the wave's two selection words, the partial and its sum are
//                  selection_write.h's (select_write, k_select_finish), shared with the other selects.
//   CLS: kClsPc reads only the 16-byte position + colour element (properties 0..9); kClsCovSingle / kClsCovHalf read the covariance
//   planes through pod_planes.h's exact decode and run ex_solve (properties 10..12), only for Gaussians that pass the filter.
// Every cross-workgroup combination is an integer add, min or max: the result is the same bits in any order.  A workgroup leaves
// ONE partial (kPropPartialWords words, plain stores); k_property_finish (the select: k_select_finish), one workgroup, combines the
// at most kPropMaxGroups of them into the result block.  Only the histogram's bins meet in global atomics.
// Built with -ffp-contract=off.  Plane offsets are 64-bit.  Nothing of the model but the selection (kPropSelect) is written.
#include "gsx_internal.h"
#include "pod_planes.h"
#include "property_math.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
enum : int { kClsPc = 0, kClsCovSingle = 1, kClsCovHalf = 2 };
static_assert(kPropMaxGroups == 2048, "eight workgroups a CU");
constexpr uint32_t kPropHistGroups = 1024;  // ... of the histogram mode: each flushes up to 4096 bins (k_bounds_hist's choice)
// The bins are ONE set of LDS counters per workgroup, every lane adding for itself.  One copy of the bins per wave (bin counts up
// to 1024) and a single add for a wave whose lanes all fall into one bin were built and measured on 10 M Gaussians, uniform and
// with every value in one bin: neither gained (each 2 to 4 % slower), so neither is here.

__device__ inline uint4 prop_ld_stream(const uint4* p) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// The planes a property reads, of ExtractPlanes' thirteen: the kernel's arguments live in scalar registers for the whole loop.
struct PropPlanes {
    const uint4* pc;
    uint4* cov_a;
    uint2* cov_b;
    uint2* cov_h;
    uint32_t* cov_h2;
};

// s_xf: the transform of a GSX_PROP_WORLD position, in LDS (15 floats: R, s, t).  It is read, as broadcasts, only by the lanes of a
// world-space call: held in scalar registers for the whole loop, beside the planes, the range and the filter, it was what no longer
// fitted them.
template <int CLS>
__device__ inline float prop_value(const PropertyJob& job, const float* s_xf, const PropPlanes& src, uint64_t i) {
    if (CLS == kClsPc) {
        const uint4 pc = prop_ld_stream(src.pc + i);
        PropTransform xf{};
        if (job.world) {
#pragma unroll
            for (int k = 0; k < 9; ++k) xf.R[k] = s_xf[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                xf.s[k] = s_xf[9 + k];
                xf.t[k] = s_xf[12 + k];
            }
        }
        return prop_value_pc(job.property, pc.x, pc.y, pc.z, pc.w, job.world != 0u, xf);
    } else {
        ExtractPlanes planes{};  // (pod_load_cov reads the covariance planes of its kind only)
        planes.cov_a = src.cov_a;
        planes.cov_b = src.cov_b;
        planes.cov_h = src.cov_h;
        planes.cov_h2 = src.cov_h2;
        float c[6];
        pod_load_cov<(CLS == kClsCovSingle ? GSX_COV3D_SINGLE : GSX_COV3D_HALF)>(planes, i, c);
        return prop_value_scale(job.property, c);
    }
}

// What k_property leaves per workgroup and k_property_finish combines (kPropPartialWords words, the last two unused): integer sums,
// minimum and maximum of order-preserving keys: the same bits in any order.
struct PropPartial {
    uint32_t count = 0, below = 0, above = 0, nonfinite = 0, kmin = kPropKeyMinIdentity, kmax = kPropKeyMaxIdentity;
    __device__ void merge(const PropPartial& b) {
        count += b.count; below += b.below; above += b.above; nonfinite += b.nonfinite;
        kmin = min(kmin, b.kmin);
        kmax = max(kmax, b.kmax);
    }
    __device__ void take(float v) {  // a finite value
        count += 1u;
        kmin = min(kmin, prop_key(v));
        kmax = max(kmax, prop_key(v));
    }
};
// The workgroup's partial from its lanes', valid in thread 0.
__device__ inline PropPartial prop_fold(const PropPartial& p) {
    return group_fold(PropPartial{wave_sum(p.count), wave_sum(p.below), wave_sum(p.above), wave_sum(p.nonfinite), wave_min(p.kmin), wave_max(p.kmax)},
                      [](PropPartial a, const PropPartial& b) {
                          a.merge(b);
                          return a;
                      });
}
}  // namespace

// One workgroup: the result block's identities and the histogram's zeros.
__global__ __launch_bounds__(256) void k_property_reset(uint32_t* __restrict__ result, uint32_t* __restrict__ hist, uint32_t bins) {
    const uint32_t t = threadIdx.x;
    if (t < kPropResultWords) result[t] = (t == kPropMinKey || t == kPropAutoMinKey) ? kPropKeyMinIdentity : 0u;
    for (uint32_t j = t; j < bins; j += 256u) hist[j] = 0u;
}

template <int CLS, uint32_t MODE>
__global__ __launch_bounds__(256) void k_property(uint64_t n, ModelFilter f, PropPlanes src, PropertyJob job) {
    __shared__ uint32_t s_bins[MODE == kPropHist ? kPropMaxBins : 1u];
    const uint32_t t = threadIdx.x;
    __shared__ float s_xf[CLS == kClsPc ? 16 : 1];
    if (CLS == kClsPc && t == 0u) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_xf[k] = job.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s_xf[9 + k] = job.s[k];
            s_xf[12 + k] = job.t[k];
        }
    }
    if (CLS == kClsPc) __syncthreads();
    // the range of the histogram and of the select (uniform)
    float lo = job.lo, hi = job.hi;
    if (MODE == kPropHist && job.auto_range) {
        const bool any = job.result[kPropAutoCount] != 0u;
        lo = any ? prop_unkey(job.result[kPropAutoMinKey]) : 0.0f;
        hi = any ? prop_unkey(job.result[kPropAutoMaxKey]) : 0.0f;
    }
    const PropRange range = prop_range(lo, hi, job.bins);
    if (MODE == kPropHist) {
        for (uint32_t j = t; j < range.bins; j += 256u) s_bins[j] = 0u;
        __syncthreads();
    }

    PropPartial p;        // per lane (hist, reduce)
    SelectCounts counts;  // (select)
    const uint64_t chunks = extract_groups(n);
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t base = c * kExtractGroup;
#pragma unroll 1
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint64_t i = base + k * 256u + t;
            if (base + k * 256u >= n) break;  // (uniform: the round holds no Gaussian)
            if (MODE == kPropValues) {
                if (i < n) job.values[i] = prop_value<CLS>(job, s_xf, src, i);
                continue;
            }
            const bool keep = prop_keep(f, n, i, t);
            const float v = keep ? prop_value<CLS>(job, s_xf, src, i) : 0.0f;
            if (MODE == kPropReduce) {
                if (keep) {
                    if (prop_finite(v)) p.take(v);
                    else p.nonfinite += 1u;
                }
            } else if (MODE == kPropHist) {
                uint32_t cls = kPropNonfinite;
                bool binned = false;
                if (keep) {
                    cls = prop_classify(range, v);
                    if (cls == kPropNonfinite) {
                        p.nonfinite += 1u;
                    } else {
                        p.take(v);
                        if (cls == kPropBelow) p.below += 1u;
                        else if (cls == kPropAbove) p.above += 1u;
                        else binned = true;
                    }
                }
                if (binned) atomicAdd(&s_bins[cls], 1u);
            } else {  // kPropSelect
                select_write(job.sel, keep && prop_hit(range, v, job.bins != 0u, job.bin_lo, job.bin_hi), i, n, counts);
            }
        }
    }
    if (MODE == kPropValues) return;
    if (MODE == kPropSelect) {
        select_store_partial(job.sel, counts);
        return;
    }

    // ---- the workgroup's partial: across the wave by butterflies, across the waves through LDS (wave_reduce.h) ----
    p = prop_fold(p);
    // ONE partial per workgroup, plain stores: 2048 workgroups adding to the same few words took longer than the stream itself
    // (DESIGN section 4); k_property_finish combines them
    if (t == 0u) *reinterpret_cast<PropPartial*>(job.partials + (size_t)blockIdx.x * kPropPartialWords) = p;
    if (MODE == kPropHist) {  // (the barrier above is behind every LDS add)
        for (uint32_t j = t; j < range.bins; j += 256u) {
            const uint32_t cnt = s_bins[j];
            if (cnt) atomicAdd(&job.hist[j], cnt);
        }
    }
}

// One workgroup: the partials of k_property combined (integer sums, min and max: any order gives the same bits) into the result
// block's words of the mode.
__global__ __launch_bounds__(256) void k_property_finish(uint32_t mode, const uint32_t* __restrict__ partials, uint32_t n_partials, uint32_t* __restrict__ result) {
    const uint32_t t = threadIdx.x;
    PropPartial p;
    for (uint32_t j = t; j < n_partials; j += 256u) p.merge(*reinterpret_cast<const PropPartial*>(partials + (size_t)j * kPropPartialWords));
    p = prop_fold(p);
    if (t != 0u) return;
    if (mode == kPropReduce) {
        result[kPropAutoCount] = p.count;
        result[kPropAutoNonfinite] = p.nonfinite;
        result[kPropAutoMinKey] = p.kmin;
        result[kPropAutoMaxKey] = p.kmax;
    } else {
        result[kPropCount] = p.count;
        result[kPropBelowAt] = p.below;
        result[kPropAboveAt] = p.above;
        result[kPropNonfiniteAt] = p.nonfinite;
        result[kPropMinKey] = p.kmin;
        result[kPropMaxKey] = p.kmax;
    }
}

hipError_t launch_property_reset(hipStream_t s, uint32_t* result, uint32_t* hist, uint32_t bins) {
    GSX_LAUNCH(k_property_reset, dim3(1), dim3(256), 0, s, result, hist, bins);
    return hipGetLastError();
}

namespace {
template <int CLS>
hipError_t launch_property_cls(hipStream_t s, uint32_t mode, uint64_t n, const ModelFilter& f, const ExtractPlanes& planes, const PropertyJob& job) {
    const PropPlanes src{planes.pc, planes.cov_a, planes.cov_b, planes.cov_h, planes.cov_h2};
    const uint32_t groups = (uint32_t)std::min<uint64_t>(extract_groups(n), mode == kPropHist ? kPropHistGroups : kPropMaxGroups);
    const dim3 grid(groups), block(256);
    switch (mode) {
        case kPropValues: GSX_LAUNCH((k_property<CLS, kPropValues>), grid, block, 0, s, n, f, src, job); break;
        case kPropReduce: GSX_LAUNCH((k_property<CLS, kPropReduce>), grid, block, 0, s, n, f, src, job); break;
        case kPropHist: GSX_LAUNCH((k_property<CLS, kPropHist>), grid, block, 0, s, n, f, src, job); break;
        case kPropSelect: GSX_LAUNCH((k_property<CLS, kPropSelect>), grid, block, 0, s, n, f, src, job); break;
        default: return hipErrorInvalidValue;
    }
    if (mode == kPropSelect) return launch_select_finish(s, job.sel, groups, job.result + kPropHit, job.result + kPropSelected);
    if (mode != kPropValues) GSX_LAUNCH(k_property_finish, dim3(1), dim3(256), 0, s, mode, job.partials, groups, job.result);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_property(hipStream_t s, uint32_t mode, int cov_kind, uint64_t n, const ModelFilter& f, const ExtractPlanes& src, const PropertyJob& job) {
    if (n == 0) return hipSuccess;
    if (!prop_is_scale(job.property)) return launch_property_cls<kClsPc>(s, mode, n, f, src, job);
    if (cov_kind == GSX_COV3D_SINGLE) return launch_property_cls<kClsCovSingle>(s, mode, n, f, src, job);
    if (cov_kind == GSX_COV3D_HALF) return launch_property_cls<kClsCovHalf>(s, mode, n, f, src, job);
    return hipErrorInvalidValue;
}

}  // namespace gsx
