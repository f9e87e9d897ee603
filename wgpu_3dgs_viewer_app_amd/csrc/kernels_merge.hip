// kernels_merge.hip — the baked path of gsx_model_merge for gfx950 (spec/RENDER_SPEC.md §13, "Model merge").  A source whose model
// transform is the identity goes through k_extract_scatter with a destination offset (kernels_extract.hip); every other source goes
// through k_merge_bake here: the same keep words, bases and destination arithmetic, but each kept Gaussian is dequantised exactly
// (§2b; pod_planes.h), moved into world space and quantised again into the destination's kind (pod_quant.h).
//   position     p' = R_m (s_m * p) + t_m, each row ((R0 a0 + R1 a1) + R2 a2) + t in float32 (§3's dot product);
//   covariance   S' = M S M^T with M = R_m diag(s_m): A = M S, then S' = A M^T, every entry a §3 dot product;
//   SH           per band and channel c' = M_l c, the float32 matrices of merge_math.h, accumulated with fmaf in column order;
//   colour word  carried.
// The per-source constants arrive by value (MergeBake, 98 floats): wave-uniform, read with scalar loads.  One lane per source
// Gaussian, four rounds of 256 per workgroup as in k_extract_scatter.  The shade records of a round are staged in LDS, eight words
// of every record at a time, and leave as whole 128-byte runs: consecutive lanes write consecutive uint4s (stage_rows_out).
// Built with -ffp-contract=off; the only fused operations are the fmaf calls of the SH product.  Plane offsets are 64-bit.
#include "gsx_internal.h"
#include "pod_planes.h"

namespace gsx {

static_assert(kMergeMaxSources == GSX_MERGE_MAX_SOURCES, "merge_math.h restates the source limit");
static_assert(sizeof(MergeBake) == 4 * (15 + kMergeShFloats), "98 floats by value");

namespace {
constexpr uint32_t kRecChunk = 8;  // words of a record staged per pass (stage_rows_out)

__device__ inline float mg_dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
__device__ inline uint4 mg_u4(float a, float b, float c, float d) {
    return make_uint4(__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d));
}

// c'[band] = M_l c[band] for the three channels, in place (s: SH floats, index 3 * coefficient + channel)
template <int L>
__device__ inline void mg_rotate_band(const MergeBake& b, float* s) {
    constexpr int m = kMergeBandSize[L], c0 = kMergeBandCoeff[L], m0 = kMergeBandMatrix[L];
    float out[3 * m];
#pragma unroll
    for (int j = 0; j < m; ++j)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float acc = b.sh[m0 + j * m] * s[3 * c0 + ch];
#pragma unroll
            for (int k = 1; k < m; ++k) acc = fmaf(b.sh[m0 + j * m + k], s[3 * (c0 + k) + ch], acc);
            out[3 * j + ch] = acc;
        }
#pragma unroll
    for (int f = 0; f < 3 * m; ++f) s[3 * c0 + f] = out[f];
}
}  // namespace

template <int SH, int COV>
__global__ __launch_bounds__(256) void k_merge_bake(uint64_t n_src, uint64_t n_dst, uint64_t dst_offset, const uint32_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ bases, ExtractPlanes src, ExtractPlanes dst, MergeBake b) {
    constexpr uint32_t kShWords = PodKind<SH, COV>::kShWords, kStride = PodKind<SH, COV>::kStride;
    constexpr uint32_t kRecWords = kStride ? kStride : 1u;
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    __shared__ uint4 s_rec[kStride ? kRecChunk * kStagePitch : 1u];
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
            pod_load_cov<COV>(src, i, c);
            pod_load_sh<SH>(src, n_src, i, s);
            // ---- bake ----
            const float sx = b.s[0] * __uint_as_float(pc.x), sy = b.s[1] * __uint_as_float(pc.y), sz = b.s[2] * __uint_as_float(pc.z);
            const float px = mg_dot3(b.R[0], b.R[1], b.R[2], sx, sy, sz) + b.t[0];
            const float py = mg_dot3(b.R[3], b.R[4], b.R[5], sx, sy, sz) + b.t[1];
            const float pz = mg_dot3(b.R[6], b.R[7], b.R[8], sx, sy, sz) + b.t[2];
            float M[9], A[9];
#pragma unroll
            for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) M[rr * 3 + cc] = b.R[rr * 3 + cc] * b.s[cc];
            const float S[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
#pragma unroll
            for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) A[rr * 3 + cc] = mg_dot3(M[rr * 3], M[rr * 3 + 1], M[rr * 3 + 2], S[cc], S[3 + cc], S[6 + cc]);
            const float o0 = mg_dot3(A[0], A[1], A[2], M[0], M[1], M[2]), o1 = mg_dot3(A[0], A[1], A[2], M[3], M[4], M[5]);
            const float o2 = mg_dot3(A[0], A[1], A[2], M[6], M[7], M[8]), o3 = mg_dot3(A[3], A[4], A[5], M[3], M[4], M[5]);
            const float o4 = mg_dot3(A[3], A[4], A[5], M[6], M[7], M[8]), o5 = mg_dot3(A[6], A[7], A[8], M[6], M[7], M[8]);
            if (SH != GSX_SH_NONE) {
                mg_rotate_band<0>(b, s);
                mg_rotate_band<1>(b, s);
                mg_rotate_band<2>(b, s);
            }
            // ---- quantise into dst's kind: the SoA planes, and the same words into the record ----
            const uint4 pc_out = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), pc.w);  // (the colour word: carried)
            dst.pc[j] = pc_out;
            uint4 g1, g2 = make_uint4(0u, 0u, 0u, 0u);
            if (COV == GSX_COV3D_SINGLE) {
                g1 = mg_u4(o0, o1, o2, o3);
                g2 = make_uint4(__float_as_uint(o4), __float_as_uint(o5), 0u, 0u);
                dst.cov_a[j] = g1;
                dst.cov_b[j] = make_uint2(g2.x, g2.y);
            } else {
                g1 = make_uint4(pack_h2(o0, o1), pack_h2(o2, o3), pack_h2(o4, o5), 0u);
                dst.cov_h[j] = make_uint2(g1.x, g1.y);
                dst.cov_h2[j] = g1.z;
            }
#pragma unroll
            for (uint32_t q = 0; q < kRecWords; ++q) rec[q] = make_uint4(0u, 0u, 0u, 0u);  // (a record's spare words are zero, as an upload leaves them)
            if (SH == GSX_SH_SINGLE) {
#pragma unroll
                for (int p = 0; p < kShPlanes4; ++p) {
                    rec[p] = mg_u4(s[4 * p], s[4 * p + 1], s[4 * p + 2], s[4 * p + 3]);
                    dst.sh4[(uint64_t)p * n_dst + j] = rec[p];
                }
                rec[11] = make_uint4(__float_as_uint(s[44]), 0u, 0u, 0u);
                dst.sh1[j] = rec[11].x;
            } else if (SH == GSX_SH_HALF) {
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    uint32_t ww[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int f0 = 8 * p + 2 * q, f1 = f0 + 1;
                        ww[q] = pack_h2(f0 < 45 ? s[f0] : 0.0f, f1 < 45 ? s[f1] : 0.0f);
                    }
                    rec[p] = make_uint4(ww[0], ww[1], ww[2], ww[3]);
                    dst.sh_h[(uint64_t)p * n_dst + j] = rec[p];
                }
            } else if (SH == GSX_SH_NORM8) {
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    uint32_t ww[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t v = 0;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int f = 16 * p + 4 * q + e;
                            v |= (f < 45 ? q_snorm8(s[f]) : 0u) << (8 * e);
                        }
                        ww[q] = v;
                    }
                    rec[p] = make_uint4(ww[0], ww[1], ww[2], ww[3]);
                    dst.sh_q[(uint64_t)p * n_dst + j] = rec[p];
                }
            }
            if (kStride) {
                rec[kShWords] = pc_out;
                rec[kShWords + 1u] = g1;
                if (COV == GSX_COV3D_SINGLE) rec[kShWords + 2u] = g2;
            }
            if (dst.edit_a) {  // edits are colour operations: they do not depend on the transform
                if (src.edit_a) {
                    dst.edit_a[j] = src.edit_a[i];
                    dst.edit_b[j] = src.edit_b[i];
                    // dst's `edited` plane starts zeroed; an OR whose result nobody reads gives the same word in any order
                    if ((src.edited[i >> 5] >> bit) & 1u) atomicOr(&dst.edited[merge_bit_word(j0, r)], merge_bit_mask(j0, r));
                } else {  // a source without edit records: never edited (the bits stay clear; the records are not read)
                    dst.edit_a[j] = make_uint4(0u, 0u, 0u, 0u);
                    dst.edit_b[j] = make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
        if (kStride == 0u) continue;
        // ---- the round's records: staged kRecChunk words at a time, written as consecutive uint4s ----
        // (passes of 8 words; 4 for the 12-word record's second pass)
        stage_rows_out<uint4, kRecChunk, kStride>(s_rec, dst.sh_aos + (j0 + r_lo) * kStride, on, r - r_lo, r_hi - r_lo, [&](uint32_t q) { return rec[q]; });
    }
}

hipError_t launch_merge_bake(hipStream_t s, int sh_kind, int cov_kind, uint64_t n_src, uint64_t n_dst, uint64_t dst_offset, const uint32_t* keep,
                             const uint32_t* bases, const ExtractPlanes& src, const ExtractPlanes& dst, const MergeBake& bake) {
    const dim3 grid((uint32_t)extract_groups(n_src)), block(256);
    return dispatch_pod_kind(sh_kind, cov_kind, [&](auto sh, auto cov) {
        GSX_LAUNCH((k_merge_bake<decltype(sh)::value, decltype(cov)::value>), grid, block, 0, s, n_src, n_dst, dst_offset, keep, bases, src, dst, bake);
        return hipGetLastError();
    });
}

}  // namespace gsx
