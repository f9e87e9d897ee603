// kernels_export.hip — the row kernel of gsx_model_export for gfx950 (spec/RENDER_SPEC.md §14, "Model export").  The kept set and
// the destination arithmetic are gsx_model_extract's (k_extract_keep, k_extract_scan, extract_group_ranks: kernels_extract.hip); a
// launch covers a CHUNK of the source, the workgroups [group0, group0 + gridDim.x), and writes its rows into a staging buffer that
// starts at the chunk's first kept Gaussian (row_base = bases[group0], which the host knows).
// One lane per KEPT Gaussian, up to four rounds of 256 per workgroup: the workgroup lists its kept Gaussians by rank in LDS first
// (k_extract_scatter's list), so a model that keeps 3 in 100 solves in one wave a workgroup, not in sixteen thin ones (measured:
// DESIGN §4).  A lane dequantises its Gaussian exactly
// (§2b, pod_quant.h), solves the covariance for rotation and scale and assembles its row (export_math.h), all in registers.  The
// rows of a round are contiguous in the staging buffer: they pass through LDS eight uint2 (PLY rows, 248 B: only 8-byte aligned) or
// four uint4 (gsx_gaussian records, 224 B) at a time and leave as runs of consecutive vector stores, 64 bytes a row and pass.
// Built with -ffp-contract=off.  Plane and row offsets are 64-bit.  Nothing of the model is written.
#include "export_math.h"
#include "gsx_internal.h"
#include "pod_quant.h"

namespace gsx {

static_assert(sizeof(gsx_gaussian) == 4 * kExportGaussianWords, "a record is 56 words");
static_assert(offsetof(gsx_gaussian, pos) == 4 * EXG_POS && offsetof(gsx_gaussian, color) == 4 * EXG_COLOR && offsetof(gsx_gaussian, sh) == 4 * EXG_SH &&
                  offsetof(gsx_gaussian, scale) == 4 * EXG_SCALE,
              "export_math.h restates the record's layout");

namespace {
constexpr uint32_t kRowPitch = 257;  // vectors between two staged columns: one more than the lanes (k_merge_bake's pitch)

template <int FORMAT> struct RowVec;
template <> struct RowVec<GSX_EXPORT_GAUSSIANS> {
    typedef uint4 type;
    static constexpr uint32_t kWords = kExportGaussianWords, kVecWords = 4, kChunk = 4;
    static __device__ inline uint4 make(const uint32_t* w) { return make_uint4(w[0], w[1], w[2], w[3]); }
};
template <> struct RowVec<GSX_EXPORT_PLY_VERTICES> {
    typedef uint2 type;
    static constexpr uint32_t kWords = kExportPlyWords, kVecWords = 2, kChunk = 8;
    static __device__ inline uint2 make(const uint32_t* w) { return make_uint2(w[0], w[1]); }
};
// the SH words of one Gaussian as loaded: whole uint4s (Sh Single: the stored bits; Half and Norm8: decoded first)
struct ShRegs {
    uint4 v[12];
    __device__ inline uint32_t operator()(int f) const {
        const uint4& q = v[f >> 2];
        return (f & 3) == 0 ? q.x : (f & 3) == 1 ? q.y : (f & 3) == 2 ? q.z : q.w;
    }
};
}  // namespace

template <int SH, int COV, int FORMAT>
__global__ __launch_bounds__(256) void k_export_rows(uint64_t n_src, uint32_t group0, uint32_t row_base, const uint32_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ bases, ExtractPlanes src, uint32_t* __restrict__ out) {
    typedef RowVec<FORMAT> RV;
    typedef typename RV::type Vec;
    constexpr uint32_t kRowVecs = RV::kWords / RV::kVecWords;  // 14 uint4 or 31 uint2
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    __shared__ Vec s_row[RV::kChunk * kRowPitch];
    __shared__ uint16_t s_list[kExtractGroup];  // the workgroup's kept Gaussians, by rank: index inside the workgroup
    const uint32_t t = threadIdx.x;
    const uint32_t group = group0 + blockIdx.x;
    const uint64_t base = (uint64_t)group * kExtractGroup;
    extract_group_ranks(keep, n_src, base, s_keep, s_before);
    if (s_before[kExtractGroupWords] == 0) return;  // (uniform)
    const uint32_t kept_all = s_before[kExtractGroupWords];
    const uint64_t j0 = (uint64_t)(bases[group] - row_base);  // the workgroup's first row in the staging buffer
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {  // (k_extract_scatter's list)
        const uint32_t local = k * 256u + t, w = local >> 5, bit = local & 31u, word = s_keep[w];
        if ((word >> bit) & 1u) s_list[s_before[w] + extract_rank(word, bit)] = (uint16_t)local;  // (clear at and above n_src)
    }
    __syncthreads();
    // a round takes the next 256 kept Gaussians, one a lane: a workgroup that keeps few of its 1024 solves in few waves
    for (uint32_t r_lo = 0; r_lo < kept_all; r_lo += 256u) {  // (uniform)
        const uint32_t r_hi = kept_all - r_lo < 256u ? kept_all : r_lo + 256u;
        const uint32_t r = r_lo + t;
        const bool on = r < r_hi;
        uint32_t row[RV::kWords];
        if (on) {
            const uint32_t local = s_list[r], bit = local & 31u;
            const uint64_t i = base + local;
            // ---- load, dequantised exactly ----
            const uint4 pc = src.pc[i];
            float c[6];
            ShRegs s;  // the bits of the dequantised SH floats
            if (COV == GSX_COV3D_SINGLE) {
                const uint4 a = src.cov_a[i];
                const uint2 bb = src.cov_b[i];
                c[0] = __uint_as_float(a.x); c[1] = __uint_as_float(a.y); c[2] = __uint_as_float(a.z); c[3] = __uint_as_float(a.w);
                c[4] = __uint_as_float(bb.x); c[5] = __uint_as_float(bb.y);
            } else {
                const uint2 a = src.cov_h[i];
                const uint32_t bb = src.cov_h2[i];
                c[0] = h_lo(a.x); c[1] = h_hi(a.x); c[2] = h_lo(a.y); c[3] = h_hi(a.y); c[4] = h_lo(bb); c[5] = h_hi(bb);
            }
            if (SH == GSX_SH_SINGLE) {
#pragma unroll
                for (int p = 0; p < kShPlanes4; ++p) s.v[p] = src.sh4[(uint64_t)p * n_src + i];
                s.v[11] = make_uint4(src.sh1[i], 0u, 0u, 0u);
            } else if (SH == GSX_SH_HALF) {
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    const uint4 v = src.sh_h[(uint64_t)p * n_src + i];
                    s.v[2 * p] = make_uint4(__float_as_uint(h_lo(v.x)), __float_as_uint(h_hi(v.x)), __float_as_uint(h_lo(v.y)), __float_as_uint(h_hi(v.y)));
                    s.v[2 * p + 1] = make_uint4(__float_as_uint(h_lo(v.z)), __float_as_uint(h_hi(v.z)), __float_as_uint(h_lo(v.w)), __float_as_uint(h_hi(v.w)));
                }
            } else if (SH == GSX_SH_NORM8) {
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    const uint4 v = src.sh_q[(uint64_t)p * n_src + i];
                    const uint32_t ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        s.v[4 * p + q] = make_uint4(__float_as_uint(dq_snorm8(ww[q], 0)), __float_as_uint(dq_snorm8(ww[q], 1)), __float_as_uint(dq_snorm8(ww[q], 2)),
                                                    __float_as_uint(dq_snorm8(ww[q], 3)));
                }
            }
            // ---- the edit record to bake (src.edit_a: only with GSX_EXPORT_BAKE_EDITS on a model that has edit records) ----
            gsx_gaussian_edit ed{};
            bool bake = false;
            if (src.edit_a && ((src.edited[i >> 5] >> bit) & 1u)) {
                const uint4 ea = src.edit_a[i];
                if (ea.x & GSX_EDIT_ENABLED) {
                    const uint4 eb = src.edit_b[i];
                    bake = true;
                    ed.flag = ea.x;
                    ed.color[0] = __uint_as_float(ea.y); ed.color[1] = __uint_as_float(ea.z); ed.color[2] = __uint_as_float(ea.w);
                    ed.contrast = __uint_as_float(eb.x); ed.exposure = __uint_as_float(eb.y); ed.gamma = __uint_as_float(eb.z); ed.alpha = __uint_as_float(eb.w);
                }
            }
            // ---- rotation and scale, then the row ----
            float rot[4], scale[3];
            ex_solve<ExportReal>(c, rot, scale);
            const uint32_t pos[3] = {pc.x, pc.y, pc.z};
            if (SH == GSX_SH_NONE) {
                if (FORMAT == GSX_EXPORT_GAUSSIANS) ex_row_gaussian(row, pos, pc.w, ExportShZero{}, rot, scale, bake, ed);
                else ex_row_ply(row, pos, pc.w, ExportShZero{}, rot, scale, bake, ed);
            } else {
                if (FORMAT == GSX_EXPORT_GAUSSIANS) ex_row_gaussian(row, pos, pc.w, s, rot, scale, bake, ed);
                else ex_row_ply(row, pos, pc.w, s, rot, scale, bake, ed);
            }
        }
        // ---- the round's rows: staged kChunk vectors of every row at a time, written as consecutive vectors ----
        const uint32_t kept = r_hi - r_lo;  // (uniform, 1 .. 256)
        Vec* __restrict__ d_rows = reinterpret_cast<Vec*>(out) + (j0 + r_lo) * kRowVecs;
#pragma unroll
        for (uint32_t v0 = 0; v0 < kRowVecs; v0 += RV::kChunk) {
            const uint32_t chunk = kRowVecs - v0 < RV::kChunk ? kRowVecs - v0 : RV::kChunk;
            __syncthreads();  // the copy of the pass before has read the staging area
            if (on) {
#pragma unroll
                for (uint32_t q = 0; q < RV::kChunk; ++q)
                    if (q < chunk) s_row[q * kRowPitch + (r - r_lo)] = RV::make(row + (v0 + q < kRowVecs ? v0 + q : 0u) * RV::kVecWords);
            }
            __syncthreads();
            const uint32_t vecs = kept * chunk;
            for (uint32_t q = t; q < vecs; q += 256u) {
                const uint32_t g = q / chunk, ww = q % chunk;
                d_rows[(uint64_t)g * kRowVecs + v0 + ww] = s_row[ww * kRowPitch + g];
            }
        }
    }
}

hipError_t launch_export_rows(hipStream_t s, int sh_kind, int cov_kind, uint32_t format, uint64_t n_src, uint32_t group0, uint32_t n_groups, uint32_t row_base,
                              const uint32_t* keep, const uint32_t* bases, const ExtractPlanes& src, void* out) {
    const dim3 grid(n_groups), block(256);
    uint32_t* o = static_cast<uint32_t*>(out);
#define GSX_XP_CASE(SH, COV)                                                                                                                      \
    if (sh_kind == SH && cov_kind == COV) {                                                                                                       \
        if (format == GSX_EXPORT_GAUSSIANS) {                                                                                                     \
            GSX_LAUNCH((k_export_rows<SH, COV, GSX_EXPORT_GAUSSIANS>), grid, block, 0, s, n_src, group0, row_base, keep, bases, src, o);           \
        } else {                                                                                                                                  \
            GSX_LAUNCH((k_export_rows<SH, COV, GSX_EXPORT_PLY_VERTICES>), grid, block, 0, s, n_src, group0, row_base, keep, bases, src, o);        \
        }                                                                                                                                         \
        return hipGetLastError();                                                                                                                 \
    }
    GSX_XP_CASE(GSX_SH_SINGLE, GSX_COV3D_SINGLE) GSX_XP_CASE(GSX_SH_SINGLE, GSX_COV3D_HALF)
    GSX_XP_CASE(GSX_SH_HALF, GSX_COV3D_SINGLE) GSX_XP_CASE(GSX_SH_HALF, GSX_COV3D_HALF)
    GSX_XP_CASE(GSX_SH_NORM8, GSX_COV3D_SINGLE) GSX_XP_CASE(GSX_SH_NORM8, GSX_COV3D_HALF)
    GSX_XP_CASE(GSX_SH_NONE, GSX_COV3D_SINGLE) GSX_XP_CASE(GSX_SH_NONE, GSX_COV3D_HALF)
#undef GSX_XP_CASE
    return hipErrorInvalidValue;
}

}  // namespace gsx
