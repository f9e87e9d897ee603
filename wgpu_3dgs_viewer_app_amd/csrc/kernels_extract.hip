// kernels_extract.hip — gsx_model_extract for gfx950 (spec/RENDER_SPEC.md §12, "Model extract"): a stable stream compaction of a
// model's resident planes into a new model.  A workgroup of either wide kernel owns kExtractGroup = 1024 consecutive Gaussians.
//   k_extract_keep     one pass over the bit planes: the keep words (extract_math.h: mask & selection & ~hidden, inverted on
//                      request, bits at or above n cleared) and ONE popcount partial per workgroup.  The hidden word comes from a
//                      wave ballot over the stored edit flags, which are read only with SKIP_HIDDEN and only where `edited` is set;
//   k_extract_scan     one workgroup: the exclusive scan of the partials in index order, kExtractScanPass at a time with the
//                      running sum carried from pass to pass; leaves the total in the workspace's first word;
//   k_extract_scatter  destination index = the workgroup's base + the ranks of the preceding words of the workgroup + the rank in
//                      the word, from the keep words alone.  SoA planes: one lane per source Gaussian.  Shade records (sh_aos, 128
//                      to 256 B each): the workgroup lists its kept Gaussians in LDS and copies `aos_stride` lanes per record, one
//                      uint4 each, so a wave's store instruction covers 1 KiB of contiguous bytes.  The edit planes travel in the
//                      same launch.
// Integer arithmetic only, no atomics that return a value: the result is the same bits from call to call.  Every plane offset is
// 64-bit (11 x 16 x n bytes pass 4 GiB at 24 M Gaussians).
#include "gsx_internal.h"
#include "pod_planes.h"

namespace gsx {

static_assert(kExtractEditEnabled == GSX_EDIT_ENABLED && kExtractEditHidden == GSX_EDIT_HIDDEN, "extract_math.h restates the edit flags");
static_assert(kExtractGroup == 4u * 256u, "four Gaussians a lane, 256 apart");

__global__ __launch_bounds__(256) void k_extract_keep(uint64_t n, ModelFilter f, uint32_t* __restrict__ keep, uint32_t* __restrict__ partials) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    uint32_t count = 0;  // lanes 0 and 32 of a wave: the popcounts of the words they wrote
    uint32_t word[4], edited[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {  // a word serves 32 lanes: the 32 loads of one address are one request
        const uint64_t i = base + k * 256u + t;
        word[k] = 0u;
        edited[k] = (i < n && f.edited) ? f.edited[i >> 5] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        bool hidden = false;
        if ((edited[k] >> (t & 31u)) & 1u) hidden = extract_flag_hides(__float_as_uint(f.edit_a[i].x));  // (edited[k] is 0 at i >= n)
        const unsigned long long hidden64 = __ballot(hidden);
        if ((lane & 31u) == 0 && i < n) {
            ExtractWords x;
            x.mask = f.mask ? f.mask[i >> 5] : 0xFFFFFFFFu;
            x.selection = f.selection ? f.selection[i >> 5] : (f.select_none ? 0u : 0xFFFFFFFFu);
            x.hidden = (uint32_t)(hidden64 >> lane);
            word[k] = extract_keep_word(x, f.invert != 0, n, i >> 5);
            keep[i >> 5] = word[k];
            count += extract_popc(word[k]);
        }
    }
    __shared__ uint32_t sums[8];
    if ((lane & 31u) == 0) sums[t >> 5] = count;
    __syncthreads();
    if (t == 0) {
        uint32_t s = 0;
        for (int j = 0; j < 8; ++j) s += sums[j];
        partials[blockIdx.x] = s;
    }
}

// One workgroup.  Pass p scans partials [256 p, 256 p + 256): an inclusive scan inside each wave (shuffles), the four wave totals
// through LDS in wave order, the carry of the passes before in a register.  Integer sums in a fixed order.
__global__ __launch_bounds__(kExtractScanPass) void k_extract_scan(const uint32_t* __restrict__ partials, uint64_t n_partials, uint32_t* __restrict__ bases,
                                                                    uint64_t* __restrict__ total) {
    __shared__ uint32_t wave_sum[kExtractScanPass / 64u];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t carry = 0;
    for (uint64_t j0 = 0; j0 < n_partials; j0 += kExtractScanPass) {
        const uint64_t j = j0 + t;
        const uint32_t own = j < n_partials ? partials[j] : 0u;
        uint32_t incl = own;
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, pass = 0;
        for (uint32_t w = 0; w < kExtractScanPass / 64u; ++w) {
            if (w < wave) before += wave_sum[w];
            pass += wave_sum[w];
        }
        if (j < n_partials) bases[j] = carry + before + (incl - own);
        carry += pass;
        __syncthreads();  // wave_sum is rewritten by the next pass
    }
    if (t == 0) *total = carry;
}

// the kept lanes of one source Gaussian each copy one 16-, 8- or 4-byte element of every plane (loads first, then stores)
template <class T, int PLANES>
__device__ inline void ex_copy_planes(const T* __restrict__ src, uint64_t n_src, uint64_t i, T* __restrict__ dst, uint64_t n_dst, uint64_t j) {
    T v[PLANES];
#pragma unroll
    for (int p = 0; p < PLANES; ++p) v[p] = src[(uint64_t)p * n_src + i];
#pragma unroll
    for (int p = 0; p < PLANES; ++p) dst[(uint64_t)p * n_dst + j] = v[p];
}

template <int SH, int COV>
__global__ __launch_bounds__(256) void k_extract_scatter(uint64_t n_src, uint64_t n_dst, uint64_t dst_offset, const uint32_t* __restrict__ keep,
                                                          const uint32_t* __restrict__ bases, ExtractPlanes src, ExtractPlanes dst) {
    constexpr uint32_t kStride = PodKind<SH, COV>::kStride;
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    __shared__ uint16_t s_list[kExtractGroup];  // the workgroup's kept Gaussians, by rank: index inside the workgroup
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    extract_group_ranks(keep, n_src, base, s_keep, s_before);
    const uint32_t kept = s_before[kExtractGroupWords];
    if (kept == 0) return;  // (uniform)
    const uint64_t j0 = dst_offset + bases[blockIdx.x];  // (dst_offset: 0 for extract; gsx_model_merge lands a source anywhere in dst)
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t local = k * 256u + t, w = local >> 5, bit = local & 31u, word = s_keep[w];
        if (!((word >> bit) & 1u)) continue;  // (the keep words are clear at and above n_src)
        const uint32_t r = s_before[w] + extract_rank(word, bit);
        const uint64_t i = base + local, j = j0 + r;
        // extract_group_list's entry, written here beside the copy that needs the same rank: as a pass of its own in front of the
        // loop the f32 scatter was 7 % slower where 3 in 100 are kept (profiles/r13_model_ops_refactor.txt)
        if (kStride) s_list[r] = (uint16_t)local;
        dst.pc[j] = src.pc[i];
        if (COV == GSX_COV3D_SINGLE) {
            dst.cov_a[j] = src.cov_a[i];
            dst.cov_b[j] = src.cov_b[i];
        } else {
            dst.cov_h[j] = src.cov_h[i];
            dst.cov_h2[j] = src.cov_h2[i];
        }
        if (SH == GSX_SH_SINGLE) {
            ex_copy_planes<uint4, kShPlanes4>(src.sh4, n_src, i, dst.sh4, n_dst, j);
            dst.sh1[j] = src.sh1[i];
        } else if (SH == GSX_SH_HALF) {
            ex_copy_planes<uint4, 6>(src.sh_h, n_src, i, dst.sh_h, n_dst, j);
        } else if (SH == GSX_SH_NORM8) {
            ex_copy_planes<uint4, 3>(src.sh_q, n_src, i, dst.sh_q, n_dst, j);
        }
        if (dst.edit_a) {
            dst.edit_a[j] = src.edit_a[i];
            dst.edit_b[j] = src.edit_b[i];
            // dst's `edited` plane starts zeroed; an OR whose result nobody reads gives the same word in any order
            // (merge_math.h: with an offset the first and last word of a source are shared with its neighbours)
            if ((src.edited[i >> 5] >> bit) & 1u) atomicOr(&dst.edited[merge_bit_word(j0, r)], merge_bit_mask(j0, r));
        }
    }
    if (kStride == 0u) return;
    __syncthreads();
    // the shade records: word q of the workgroup's output is word q % kStride of its (q / kStride)-th kept Gaussian; consecutive
    // lanes write consecutive uint4s.  Four loads in flight per lane.
    const uint32_t words = kept * kStride;
    const uint4* __restrict__ s_aos = src.sh_aos + base * kStride;
    uint4* __restrict__ d_aos = dst.sh_aos + j0 * kStride;
    auto load = [&](uint32_t q) {  // (past the end: word 0 again, never stored)
        constexpr uint32_t kDiv = kStride ? kStride : 1u;  // (kStride = 0 never gets here)
        const uint32_t qq = q < words ? q : 0u;
        return s_aos[(uint32_t)s_list[qq / kDiv] * kStride + qq % kDiv];
    };
    for (uint32_t q0 = t; q0 < words; q0 += 4u * 256u) {
        const uint32_t q1 = q0 + 256u, q2 = q0 + 512u, q3 = q0 + 768u;
        const uint4 v0 = load(q0), v1 = load(q1), v2 = load(q2), v3 = load(q3);
        d_aos[q0] = v0;
        if (q1 < words) d_aos[q1] = v1;
        if (q2 < words) d_aos[q2] = v2;
        if (q3 < words) d_aos[q3] = v3;
    }
}

hipError_t launch_extract_keep(hipStream_t s, uint64_t n, const ModelFilter& f, uint32_t* keep, uint32_t* partials) {
    GSX_LAUNCH(k_extract_keep, dim3((uint32_t)extract_groups(n)), dim3(256), 0, s, n, f, keep, partials);
    return hipGetLastError();
}
hipError_t launch_extract_scan(hipStream_t s, const uint32_t* partials, uint64_t n_partials, uint32_t* bases, uint64_t* total) {
    GSX_LAUNCH(k_extract_scan, dim3(1), dim3(kExtractScanPass), 0, s, partials, n_partials, bases, total);
    return hipGetLastError();
}
hipError_t launch_extract_scatter(hipStream_t s, int sh_kind, int cov_kind, uint64_t n_src, uint64_t n_dst, uint64_t dst_offset, const uint32_t* keep,
                                  const uint32_t* bases, const ExtractPlanes& src, const ExtractPlanes& dst) {
    const dim3 grid((uint32_t)extract_groups(n_src)), block(256);
    return dispatch_pod_kind(sh_kind, cov_kind, [&](auto sh, auto cov) {
        GSX_LAUNCH((k_extract_scatter<decltype(sh)::value, decltype(cov)::value>), grid, block, 0, s, n_src, n_dst, dst_offset, keep, bases, src, dst);
        return hipGetLastError();
    });
}

}  // namespace gsx
