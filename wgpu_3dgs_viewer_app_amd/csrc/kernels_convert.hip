// kernels_convert.hip — gsx_model_convert for gfx950 (spec/RENDER_SPEC.md §16, "Model convert"): k_extract_scatter's stable
// compaction into a model of ANOTHER pod kind.  The frame is k_merge_bake's: a workgroup of 256 owns kExtractGroup = 1024 consecutive
// source Gaussians in four rounds, the destination index comes from the keep words alone (extract_group_ranks, dst_offset + bases),
// one lane per kept source Gaussian.  Each kept Gaussian is dequantised exactly from the source kind (pod_planes.h: pod_load_cov,
// pod_load_sh; §2b) and quantised once into the destination kind (pod_encode_cov, pod_encode_sh: pod_quant.h's pack_h2 / q_snorm8);
// the position and the colour word are carried as stored bits.  A source of Sh None stands for 45 zeros; a destination of Sh None
// reads no SH plane and has no shade records.  The SoA planes are stored straight from the lane; the destination's shade records
// are staged in LDS eight words at a time (the 12-word record: whole) and leave as whole runs (stage_rows_out).  The edit planes
// travel as in the scatter.
// No arithmetic but the conversions: there is nothing here for -ffp-contract to fuse, the file is built with the Makefile's flags
// all the same.  Plane offsets are 64-bit.
// Both kinds are template parameters: the destination decides the record layout and the LDS staging, the source the loads; the
// 48-float SH array is indexed by constants only after unrolling and stays in registers (no scratch).  The diagonal (same kind) is
// not instantiated: it is k_extract_scatter.
#include "gsx_internal.h"
#include "pod_planes.h"

namespace gsx {

namespace {
// Words of a record staged per pass (stage_rows_out).  8 words are a 128-byte line: the 16-word record leaves in two passes of whole
// lines, the 8-word record in one.  The 12-word record (Sh Half + Cov3d Single, 192 B) in passes of 8 and 4 leaves 128-byte and
// 64-byte pieces 192 bytes apart; staged whole (12 words, 49 KiB of LDS, three workgroups a CU instead of four) it leaves as one run:
// measured on 10 M Gaussians that keep everything, 850 to 1260 us -> 610 to 1030 us over the seven sources.
template <uint32_t STRIDE>
constexpr uint32_t convert_chunk() { return STRIDE == 12u ? 12u : 8u; }
}

template <int DSH, int DCOV, int SSH, int SCOV>
__global__ __launch_bounds__(256) void k_convert_kind(uint64_t n_src, uint64_t n_dst, uint64_t dst_offset, const uint32_t* __restrict__ keep,
                                                       const uint32_t* __restrict__ bases, ExtractPlanes src, ExtractPlanes dst) {
    constexpr uint32_t kShWords = PodKind<DSH, DCOV>::kShWords, kStride = PodKind<DSH, DCOV>::kStride;
    constexpr uint32_t kRecWords = kStride ? kStride : 1u, kConvertChunk = convert_chunk<kStride>();
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    __shared__ uint4 s_rec[kStride ? kConvertChunk * kStagePitch : 1u];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    extract_group_ranks(keep, n_src, base, s_keep, s_before);
    if (s_before[kExtractGroupWords] == 0) return;  // (uniform)
    const uint64_t j0 = dst_offset + bases[blockIdx.x];
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t local = k * 256u + t, w = local >> 5, bit = local & 31u, word = s_keep[w];
        const bool on = (word >> bit) & 1u;  // (the keep words are clear at and above n_src)
        // the round's kept Gaussians have consecutive ranks [r_lo, r_hi)
        const uint32_t r_lo = s_before[8u * k], r_hi = s_before[8u * k + 8u];
        const uint32_t r = s_before[w] + extract_rank(word, bit);
        uint4 rec[kRecWords];
        if (on) {
            const uint64_t i = base + local, j = j0 + r;
            // ---- load, dequantised exactly ----
            const uint4 pc = src.pc[i];
            float c[6], s[48];
            pod_load_cov<SCOV>(src, i, c);
            if (DSH != GSX_SH_NONE) {  // (a destination without SH reads none)
                if (SSH == GSX_SH_NONE) {
#pragma unroll
                    for (int f = 0; f < 48; ++f) s[f] = 0.0f;  // a source of Sh None stands for 45 zeros
                } else {
                    pod_load_sh<SSH>(src, n_src, i, s);
                }
            }
            // ---- quantise once into dst's kind: the SoA planes, and the same words into the record ----
            dst.pc[j] = pc;  // position and colour word: carried
            uint4 g1, g2;
            pod_encode_cov<DCOV>(c, g1, g2);
            if (DCOV == GSX_COV3D_SINGLE) {
                dst.cov_a[j] = g1;
                dst.cov_b[j] = make_uint2(g2.x, g2.y);
            } else {
                dst.cov_h[j] = make_uint2(g1.x, g1.y);
                dst.cov_h2[j] = g1.z;
            }
#pragma unroll
            for (uint32_t q = 0; q < kRecWords; ++q) rec[q] = make_uint4(0u, 0u, 0u, 0u);  // (a record's spare words are zero, as an upload leaves them)
            pod_encode_sh<DSH>(s, rec);
            if (DSH == GSX_SH_SINGLE) {
#pragma unroll
                for (int p = 0; p < kShPlanes4; ++p) dst.sh4[(uint64_t)p * n_dst + j] = rec[p];
                dst.sh1[j] = rec[11].x;
            } else if (DSH == GSX_SH_HALF) {
#pragma unroll
                for (int p = 0; p < 6; ++p) dst.sh_h[(uint64_t)p * n_dst + j] = rec[p];
            } else if (DSH == GSX_SH_NORM8) {
#pragma unroll
                for (int p = 0; p < 3; ++p) dst.sh_q[(uint64_t)p * n_dst + j] = rec[p];
            }
            if (kStride) {
                rec[kShWords] = pc;
                rec[kShWords + 1u] = g1;
                if (DCOV == GSX_COV3D_SINGLE) rec[kShWords + 2u] = g2;
            }
            if (dst.edit_a) {
                dst.edit_a[j] = src.edit_a[i];
                dst.edit_b[j] = src.edit_b[i];
                // dst's `edited` plane starts zeroed; an OR whose result nobody reads gives the same word in any order
                if ((src.edited[i >> 5] >> bit) & 1u) atomicOr(&dst.edited[merge_bit_word(j0, r)], merge_bit_mask(j0, r));
            }
        }
        if (kStride == 0u) continue;
        // ---- the round's records: staged kConvertChunk words at a time, written as consecutive uint4s ----
        stage_rows_out<uint4, kConvertChunk, kStride>(s_rec, dst.sh_aos + (j0 + r_lo) * kStride, on, r - r_lo, r_hi - r_lo, [&](uint32_t q) { return rec[q]; });
    }
}

hipError_t launch_convert_kind(hipStream_t s, int src_sh, int src_cov, int dst_sh, int dst_cov, uint64_t n_src, uint64_t n_dst, uint64_t dst_offset,
                               const uint32_t* keep, const uint32_t* bases, const ExtractPlanes& src, const ExtractPlanes& dst) {
    const dim3 grid((uint32_t)extract_groups(n_src)), block(256);
    return dispatch_pod_kind(dst_sh, dst_cov, [&](auto dsh, auto dcov) {
        return dispatch_pod_kind(src_sh, src_cov, [&](auto ssh, auto scov) -> hipError_t {
            constexpr int DSH = decltype(dsh)::value, DCOV = decltype(dcov)::value, SSH = decltype(ssh)::value, SCOV = decltype(scov)::value;
            if constexpr (DSH == SSH && DCOV == SCOV) {
                return hipErrorInvalidValue;  // the same kind is launch_extract_scatter's: no kernel of this file exists for it
            } else {
                GSX_LAUNCH((k_convert_kind<DSH, DCOV, SSH, SCOV>), grid, block, 0, s, n_src, n_dst, dst_offset, keep, bases, src, dst);
                return hipGetLastError();
            }
        });
    });
}

}  // namespace gsx
