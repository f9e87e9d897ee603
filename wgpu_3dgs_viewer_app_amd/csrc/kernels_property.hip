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
//     kPropSelect  ballots the 64 hits into the wave's two selection words; lanes 0 and 32 apply the op to the word they read and
//                  write it back, tail bits clear, and count hits and selected bits.
//   CLS: kClsPc reads only the 16-byte position + colour element (properties 0..9); kClsCovSingle / kClsCovHalf read the covariance
//   planes through pod_planes.h's exact decode and run ex_solve (properties 10..12), only for Gaussians that pass the filter.
// Every cross-workgroup combination is an integer add, min or max: the result is the same bits in any order.  A workgroup leaves
// ONE partial (kPropPartialWords words, plain stores); k_property_finish, one workgroup, combines the at most kPropMaxGroups of them
// into the result block.  Only the histogram's bins meet in global atomics.
// Built with -ffp-contract=off.  Plane offsets are 64-bit.  Nothing of the model but the selection (kPropSelect) is written.
#include "gsx_internal.h"
#include "pod_planes.h"
#include "property_math.h"

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

__device__ inline uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ inline uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor(x, o, 64));
    return x;
}
__device__ inline uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor(x, o, 64));
    return x;
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
    __shared__ uint32_t s_part[4][6];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
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

    // per lane: c0 count (hist, reduce) or hits (select); c1 below or selected; c2 above; c3 non-finite; the keys of min and max
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, kmin = kPropKeyMinIdentity, kmax = kPropKeyMaxIdentity;
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
                    if (prop_finite(v)) {
                        c0 += 1u;
                        kmin = min(kmin, prop_key(v));
                        kmax = max(kmax, prop_key(v));
                    } else {
                        c3 += 1u;
                    }
                }
            } else if (MODE == kPropHist) {
                uint32_t cls = kPropNonfinite;
                bool binned = false;
                if (keep) {
                    cls = prop_classify(range, v);
                    if (cls == kPropNonfinite) {
                        c3 += 1u;
                    } else {
                        c0 += 1u;
                        kmin = min(kmin, prop_key(v));
                        kmax = max(kmax, prop_key(v));
                        if (cls == kPropBelow) c1 += 1u;
                        else if (cls == kPropAbove) c2 += 1u;
                        else binned = true;
                    }
                }
                if (binned) atomicAdd(&s_bins[cls], 1u);
            } else {  // kPropSelect
                const bool hit = keep && prop_hit(range, v, job.bins != 0u, job.bin_lo, job.bin_hi);
                const unsigned long long hits64 = __ballot(hit);
                // The wave's lanes have read the words of their Gaussians above (prop_keep: the selection as it was before the call);
                // this lane now reads and writes the word of its 32: no other wave touches it.
                if ((lane & 31u) == 0u && i < n) {
                    const uint64_t w = i >> 5;
                    const uint32_t hits = (uint32_t)(hits64 >> lane);
                    const uint32_t old = job.selection_valid ? job.selection[w] : 0u;
                    const uint32_t now = prop_apply_op(job.op, old, hits) & extract_tail_mask(n, w);
                    job.selection[w] = now;
                    c0 += extract_popc(hits);
                    c1 += extract_popc(now);
                }
            }
        }
    }
    if (MODE == kPropValues) return;

    // ---- the workgroup's partials: across the wave by butterflies, across the waves through LDS, then one atomic a counter ----
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    if (MODE != kPropSelect) {
        c2 = wave_sum(c2);
        c3 = wave_sum(c3);
        kmin = wave_min(kmin);
        kmax = wave_max(kmax);
    }
    if (lane == 0u) {
        s_part[wave][0] = c0; s_part[wave][1] = c1; s_part[wave][2] = c2; s_part[wave][3] = c3; s_part[wave][4] = kmin; s_part[wave][5] = kmax;
    }
    __syncthreads();
    if (t == 0u) {
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, mn = kPropKeyMinIdentity, mx = kPropKeyMaxIdentity;
        for (uint32_t w = 0; w < 4u; ++w) {
            a0 += s_part[w][0]; a1 += s_part[w][1]; a2 += s_part[w][2]; a3 += s_part[w][3];
            mn = min(mn, s_part[w][4]);
            mx = max(mx, s_part[w][5]);
        }
        // ONE partial per workgroup, plain stores: 2048 workgroups adding to the same few words took longer than the stream itself
        // (DESIGN section 4); k_property_finish combines them
        uint32_t* p = job.partials + (size_t)blockIdx.x * kPropPartialWords;
        p[0] = a0; p[1] = a1; p[2] = a2; p[3] = a3; p[4] = mn; p[5] = mx;
    }
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
    __shared__ uint32_t s_part[4][6];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, mn = kPropKeyMinIdentity, mx = kPropKeyMaxIdentity;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const uint32_t* p = partials + (size_t)j * kPropPartialWords;
        a0 += p[0]; a1 += p[1]; a2 += p[2]; a3 += p[3];
        mn = min(mn, p[4]);
        mx = max(mx, p[5]);
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0u) {
        s_part[wave][0] = a0; s_part[wave][1] = a1; s_part[wave][2] = a2; s_part[wave][3] = a3; s_part[wave][4] = mn; s_part[wave][5] = mx;
    }
    __syncthreads();
    if (t != 0u) return;
    a0 = a1 = a2 = a3 = 0u;
    mn = kPropKeyMinIdentity;
    mx = kPropKeyMaxIdentity;
    for (uint32_t w = 0; w < 4u; ++w) {
        a0 += s_part[w][0]; a1 += s_part[w][1]; a2 += s_part[w][2]; a3 += s_part[w][3];
        mn = min(mn, s_part[w][4]);
        mx = max(mx, s_part[w][5]);
    }
    if (mode == kPropSelect) {
        result[kPropHit] = a0;
        result[kPropSelected] = a1;
    } else if (mode == kPropReduce) {
        result[kPropAutoCount] = a0;
        result[kPropAutoNonfinite] = a3;
        result[kPropAutoMinKey] = mn;
        result[kPropAutoMaxKey] = mx;
    } else {
        result[kPropCount] = a0;
        result[kPropBelowAt] = a1;
        result[kPropAboveAt] = a2;
        result[kPropNonfiniteAt] = a3;
        result[kPropMinKey] = mn;
        result[kPropMaxKey] = mx;
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
