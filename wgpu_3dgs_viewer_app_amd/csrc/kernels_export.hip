// kernels_export.hip — the row kernel of gsx_model_export for gfx950 (spec/RENDER_SPEC.md §14, "Model export").  The kept set and
// the destination arithmetic are gsx_model_extract's (k_extract_keep, k_extract_scan, extract_group_ranks: kernels_extract.hip); a
// launch covers a CHUNK of the source, the workgroups [group0, group0 + gridDim.x), and writes its rows into a staging buffer that
// starts at the chunk's first kept Gaussian (row_base = bases[group0], which the host knows).
// One lane per KEPT Gaussian, up to four rounds of 256 per workgroup: the workgroup lists its kept Gaussians by rank in LDS first
// (extract_group_list), so a model that keeps 3 in 100 solves in one wave a workgroup, not in sixteen thin ones (measured:
// DESIGN §4).  A lane dequantises its Gaussian exactly (§2b, pod_planes.h), solves the covariance for rotation and scale and
// assembles its row (export_math.h), all in registers.  The rows of a round are contiguous in the staging buffer: they pass through
// LDS eight uint2 (PLY rows, 248 B: only 8-byte aligned) or four uint4 (gsx_gaussian records, 224 B) at a time and leave as runs of
// consecutive vector stores, 64 bytes a row and pass (stage_rows_out).
// Built with -ffp-contract=off.  Plane and row offsets are 64-bit.  Nothing of the model is written.
#include "export_math.h"
#include "gsx_internal.h"
#include "pod_planes.h"

namespace gsx {

static_assert(sizeof(gsx_gaussian) == 4 * kExportGaussianWords, "a record is 56 words");
static_assert(offsetof(gsx_gaussian, pos) == 4 * EXG_POS && offsetof(gsx_gaussian, color) == 4 * EXG_COLOR && offsetof(gsx_gaussian, sh) == 4 * EXG_SH &&
                  offsetof(gsx_gaussian, scale) == 4 * EXG_SCALE,
              "export_math.h restates the record's layout");

namespace {
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
// the bits of the dequantised SH floats of one Gaussian (pod_load_sh), as the row assembly reads them
struct ShBits {
    const float* s;
    __device__ inline uint32_t operator()(int f) const { return __float_as_uint(s[f]); }
};
}  // namespace

template <int SH, int COV, int FORMAT>
__global__ __launch_bounds__(256) void k_export_rows(uint64_t n_src, uint32_t group0, uint32_t row_base, const uint32_t* __restrict__ keep,
                                                      const uint32_t* __restrict__ bases, ExtractPlanes src, uint32_t* __restrict__ out) {
    typedef RowVec<FORMAT> RV;
    typedef typename RV::type Vec;
    constexpr uint32_t kRowVecs = RV::kWords / RV::kVecWords;  // 14 uint4 or 31 uint2
    __shared__ uint32_t s_keep[kExtractGroupWords], s_before[kExtractGroupWords + 1];
    __shared__ Vec s_row[RV::kChunk * kStagePitch];
    __shared__ uint16_t s_list[kExtractGroup];  // the workgroup's kept Gaussians, by rank: index inside the workgroup
    const uint32_t t = threadIdx.x;
    const uint32_t group = group0 + blockIdx.x;
    const uint64_t base = (uint64_t)group * kExtractGroup;
    extract_group_ranks(keep, n_src, base, s_keep, s_before);
    if (s_before[kExtractGroupWords] == 0) return;  // (uniform)
    const uint32_t kept_all = s_before[kExtractGroupWords];
    const uint64_t j0 = (uint64_t)(bases[group] - row_base);  // the workgroup's first row in the staging buffer
    extract_group_list(s_keep, s_before, s_list);
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
            float c[6], s[48];
            pod_load_cov<COV>(src, i, c);
            pod_load_sh<SH>(src, n_src, i, s);
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
                if (FORMAT == GSX_EXPORT_GAUSSIANS) ex_row_gaussian(row, pos, pc.w, ShBits{s}, rot, scale, bake, ed);
                else ex_row_ply(row, pos, pc.w, ShBits{s}, rot, scale, bake, ed);
            }
        }
        // ---- the round's rows (r_hi - r_lo of them: uniform, 1 .. 256): staged kChunk vectors of every row at a time ----
        stage_rows_out<Vec, RV::kChunk, kRowVecs>(s_row, reinterpret_cast<Vec*>(out) + (j0 + r_lo) * kRowVecs, on, r - r_lo, r_hi - r_lo,
                                                  [&](uint32_t q) { return RV::make(row + q * RV::kVecWords); });
    }
}

hipError_t launch_export_rows(hipStream_t s, int sh_kind, int cov_kind, uint32_t format, uint64_t n_src, uint32_t group0, uint32_t n_groups, uint32_t row_base,
                              const uint32_t* keep, const uint32_t* bases, const ExtractPlanes& src, void* out) {
    const dim3 grid(n_groups), block(256);
    uint32_t* o = static_cast<uint32_t*>(out);
    return dispatch_pod_kind(sh_kind, cov_kind, [&](auto sh, auto cov) {
        constexpr int SH = decltype(sh)::value, COV = decltype(cov)::value;
        if (format == GSX_EXPORT_GAUSSIANS) {
            GSX_LAUNCH((k_export_rows<SH, COV, GSX_EXPORT_GAUSSIANS>), grid, block, 0, s, n_src, group0, row_base, keep, bases, src, o);
        } else {
            GSX_LAUNCH((k_export_rows<SH, COV, GSX_EXPORT_PLY_VERTICES>), grid, block, 0, s, n_src, group0, row_base, keep, bases, src, o);
        }
        return hipGetLastError();
    });
}

}  // namespace gsx
