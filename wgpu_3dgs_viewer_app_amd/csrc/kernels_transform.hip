// kernels_transform.hip — gsx_model_apply_transform for gfx950 (spec/RENDER_SPEC.md §21, "Model transform"): the kept Gaussians of
// a resident model are moved where they lie.  The arithmetic is §13's (kernels_merge.hip), restated here and shown equal by test
// (tests/test_gpu_transform.py), not shared as text:
//   position     transform_math.h: p' = R (s * (p - c)) + t + c, without the pivot §13's p' bit for bit;
//   covariance   S' = (M S) M^T with M = R diag(s), every entry a §3 dot product;
//   SH           per band and channel c' = M_l c, merge_math.h's float32 matrices, accumulated with fmaf in column order;
//   colour word  carried.
// The frame is the extract family's: 256 lanes, kExtractGroup = 1024 consecutive Gaussians a workgroup in four rounds, the keep
// words read through LDS (extract_group_ranks), a workgroup without a kept bit returns at once.  One lane owns one Gaussian and
// writes it at its own index: no atomics, the same bits on every call; a Gaussian that is not kept is neither read nor written.
// MODE (transform_math.h) is a template argument: translate neither loads nor stores a covariance or SH plane, no-rotation leaves
// the SH planes alone.  Planes are decoded by pod_planes.h's loaders and encoded by its pod_encode_cov / pod_encode_sh.
// The shade records of the kept Gaussians are rewritten from the same words.  In place the kept rows of a round are contiguous
// only when all 256 are kept, so two writers exist: each lane writing its own row (GSX_TRANSFORM_STAGED 0), or the round's rows
// staged in LDS, eight words of every row at a time, and written by consecutive lanes as runs of whole rows, the row found through
// a list of the round's kept lanes (GSX_TRANSFORM_STAGED 1; full mode only: the other modes write one to three words a row).  The
// library is built with the value below; tools/bench_transform.py builds and times both (DESIGN §4 "Model transform").
// Built with -ffp-contract=off; the only fused operations are the fmaf calls of the SH product.  Plane offsets are 64-bit.
#include "gsx_internal.h"
#include "pod_planes.h"
#include "transform_math.h"

#ifndef GSX_TRANSFORM_STAGED
#define GSX_TRANSFORM_STAGED 1
#endif

namespace gsx {

namespace {
constexpr uint32_t kTfRecChunk = 8;  // words of a record staged per pass

__device__ inline float tf_dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// c'[band] = M_l c[band] for the three channels, in place (s: SH floats, index 3 * coefficient + channel)
template <int L>
__device__ inline void tf_rotate_band(const MergeBake& b, float* s) {
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

// The staged writer in place: as stage_rows_out (gsx_internal.h), but row g of the round's `kept` rows belongs to the Gaussian
// s_idx[g] of the workgroup (rows: the workgroup's first record).  Lane `slot` of the kept lanes that are `on` is Gaussian `local`.
template <uint32_t CHUNK, uint32_t ROW_VECS, class F>
__device__ inline void tf_stage_rows_inplace(uint4* s_stage, uint16_t* s_idx, uint4* __restrict__ rows, bool on, uint32_t slot, uint32_t local,
                                             uint32_t kept, F&& vec) {
#pragma unroll
    for (uint32_t v0 = 0; v0 < ROW_VECS; v0 += CHUNK) {
        const uint32_t chunk = ROW_VECS - v0 < CHUNK ? ROW_VECS - v0 : CHUNK;  // (the last pass of a row may be shorter)
        __syncthreads();  // the copy of the pass before has read the staging area and the list
        if (on) {
            s_idx[slot] = (uint16_t)local;
#pragma unroll
            for (uint32_t q = 0; q < CHUNK; ++q)
                if (q < chunk) s_stage[q * kStagePitch + slot] = vec(v0 + q < ROW_VECS ? v0 + q : 0u);
        }
        __syncthreads();
        const uint32_t vecs = kept * chunk;
        for (uint32_t q = threadIdx.x; q < vecs; q += 256u) {
            const uint32_t g = q / chunk, ww = q % chunk;
            rows[(uint32_t)s_idx[g] * ROW_VECS + v0 + ww] = s_stage[ww * kStagePitch + g];
        }
    }
}
}  // namespace

template <int SH, int COV, int MODE>
__global__ __launch_bounds__(256) void k_transform_inplace(uint64_t n, const uint32_t* __restrict__ keep, ExtractPlanes m, TransformBake tb) {
    constexpr uint32_t kShWords = PodKind<SH, COV>::kShWords, kStride = PodKind<SH, COV>::kStride;
    constexpr uint32_t kRecWords = kStride ? kStride : 1u;
    constexpr bool kCov = MODE != kTransformTranslate;                     // the covariance planes are rewritten
    constexpr bool kSh = MODE == kTransformFull && SH != GSX_SH_NONE;      // the SH planes are rewritten
    constexpr bool kStaged = GSX_TRANSFORM_STAGED != 0 && MODE == kTransformFull && kStride != 0u;
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    __shared__ uint4 s_rec[kStaged ? kTfRecChunk * kStagePitch : 1u];
    __shared__ uint16_t s_idx[kStaged ? 256u : 1u];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    extract_group_ranks(keep, n, base, s_keep, s_before);
    if (s_before[kExtractGroupWords] == 0) return;  // (uniform)
    const MergeBake& b = tb.b;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t local = k * 256u + t, w = local >> 5, bit = local & 31u, word = s_keep[w];
        const bool on = (word >> bit) & 1u;  // (the keep words are clear at and above n)
        // the round's kept Gaussians have consecutive ranks [r_lo, r_hi)
        const uint32_t r_lo = s_before[8u * k], r_hi = s_before[8u * k + 8u];
        if (r_hi == r_lo) continue;  // (uniform)
        const uint32_t r = s_before[w] + extract_rank(word, bit);
        uint4 rec[kRecWords];
        if (on) {
            const uint64_t i = base + local;
            // ---- load, dequantised exactly: every load of the Gaussian in front of its first store (the planes are written where
            //      they are read, so the compiler keeps a load that follows a store behind it) ----
            const uint4 pc = m.pc[i];
            float c[6], s[48];
            if (kCov) pod_load_cov<COV>(m, i, c);
            if (kSh) pod_load_sh<SH>(m, n, i, s);
            // ---- position (every mode) ----
            const float p[3] = {__uint_as_float(pc.x), __uint_as_float(pc.y), __uint_as_float(pc.z)};
            float pp[3];
            transform_position(b.R, b.s, b.t, tb.c, tb.use_pivot != 0u, p, pp);
            const uint4 pc_out = make_uint4(__float_as_uint(pp[0]), __float_as_uint(pp[1]), __float_as_uint(pp[2]), pc.w);  // (the colour word: carried)
            m.pc[i] = pc_out;
            // ---- covariance: baked, quantised again ----
            uint4 g1 = make_uint4(0u, 0u, 0u, 0u), g2 = make_uint4(0u, 0u, 0u, 0u);
            if (kCov) {
                float M[9], A[9];
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) M[rr * 3 + cc] = b.R[rr * 3 + cc] * b.s[cc];
                const float S[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) A[rr * 3 + cc] = tf_dot3(M[rr * 3], M[rr * 3 + 1], M[rr * 3 + 2], S[cc], S[3 + cc], S[6 + cc]);
                const float o[6] = {tf_dot3(A[0], A[1], A[2], M[0], M[1], M[2]), tf_dot3(A[0], A[1], A[2], M[3], M[4], M[5]),
                                    tf_dot3(A[0], A[1], A[2], M[6], M[7], M[8]), tf_dot3(A[3], A[4], A[5], M[3], M[4], M[5]),
                                    tf_dot3(A[3], A[4], A[5], M[6], M[7], M[8]), tf_dot3(A[6], A[7], A[8], M[6], M[7], M[8])};
                pod_encode_cov<COV>(o, g1, g2);
                if (COV == GSX_COV3D_SINGLE) {
                    m.cov_a[i] = g1;
                    m.cov_b[i] = make_uint2(g2.x, g2.y);
                } else {
                    m.cov_h[i] = make_uint2(g1.x, g1.y);
                    m.cov_h2[i] = g1.z;
                }
            }
            // ---- SH ----
#pragma unroll
            for (uint32_t q = 0; q < kRecWords; ++q) rec[q] = make_uint4(0u, 0u, 0u, 0u);  // (a record's spare words are zero, as an upload leaves them)
            if (kSh) {
                tf_rotate_band<0>(b, s);
                tf_rotate_band<1>(b, s);
                tf_rotate_band<2>(b, s);
                pod_encode_sh<SH>(s, rec);
                if (SH == GSX_SH_SINGLE) {
#pragma unroll
                    for (int pl = 0; pl < kShPlanes4; ++pl) m.sh4[(uint64_t)pl * n + i] = rec[pl];
                    m.sh1[i] = rec[11].x;
                } else if (SH == GSX_SH_HALF) {
#pragma unroll
                    for (int pl = 0; pl < 6; ++pl) m.sh_h[(uint64_t)pl * n + i] = rec[pl];
                } else if (SH == GSX_SH_NORM8) {
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) m.sh_q[(uint64_t)pl * n + i] = rec[pl];
                }
            }
            // ---- the shade record: the same words ----
            if (kStride) {
                rec[kShWords] = pc_out;
                rec[kShWords + 1u] = g1;
                if (COV == GSX_COV3D_SINGLE) rec[kShWords + 2u] = g2;
                if (!kStaged) {  // the lane writes the words of its own row that the mode rewrites
                    uint4* __restrict__ row = m.sh_aos + i * kStride;
                    if (kSh) {
#pragma unroll
                        for (uint32_t q = 0; q < kShWords; ++q) row[q] = rec[q];
                    }
                    row[kShWords] = rec[kShWords];
                    if (kCov) {
                        row[kShWords + 1u] = rec[kShWords + 1u];
                        if (COV == GSX_COV3D_SINGLE) row[kShWords + 2u] = rec[kShWords + 2u];
                    }
                }
            }
        }
        if (kStaged)  // the round's records: staged kTfRecChunk words at a time, written as whole rows by consecutive lanes
            tf_stage_rows_inplace<kTfRecChunk, kStride>(s_rec, s_idx, m.sh_aos + base * kStride, on, r - r_lo, local, r_hi - r_lo,
                                                        [&](uint32_t q) { return rec[q]; });
    }
}

hipError_t launch_transform_inplace(hipStream_t s, int sh_kind, int cov_kind, int mode, uint64_t n, const uint32_t* keep, const ExtractPlanes& m,
                                    const TransformBake& bake) {
    if (n == 0) return hipSuccess;
    const dim3 grid((uint32_t)extract_groups(n)), block(256);
    return dispatch_pod_kind(sh_kind, cov_kind, [&](auto sh, auto cov) {
        constexpr int SH = decltype(sh)::value, COV = decltype(cov)::value;
        switch (mode) {
            case kTransformTranslate: GSX_LAUNCH((k_transform_inplace<SH, COV, kTransformTranslate>), grid, block, 0, s, n, keep, m, bake); break;
            case kTransformNoRotation: GSX_LAUNCH((k_transform_inplace<SH, COV, kTransformNoRotation>), grid, block, 0, s, n, keep, m, bake); break;
            case kTransformFull: GSX_LAUNCH((k_transform_inplace<SH, COV, kTransformFull>), grid, block, 0, s, n, keep, m, bake); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    });
}

}  // namespace gsx
