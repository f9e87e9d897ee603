// kernels_import.hip — the row kernel of gsx_model_import_ply and gsx_model_upload_ply_rows for gfx950 (spec/RENDER_SPEC.md §15,
// "PLY import").  One lane per Gaussian, kImportGroup = 128 rows a workgroup.  The write side is k_convert's (pod_store.h:
// store_gaussian, coalesced plane stores, shade records included; the pod kind is a runtime value as it is there).  The read side:
//   kImportSlab     the canonical layout (stride 248, property k at byte 4 k): the workgroup's rows are one contiguous slab of at most
//                   31 744 bytes, loaded once with 16-byte non-temporal loads into LDS; a lane then reads its row as 31 uint2.  A
//                   row is 62 dwords = 31 qwords: an odd qword stride, so the 32 lanes of a half wave cover all 64 banks once
//                   (the 8-byte read is banked modulo 64 dwords) — no padding, and the 16-byte LDS stores stay whole.
//   kImportDirect   the canonical layout, every lane reading its own row at a 248-byte stride from global memory (31 non-temporal
//                   uint2 loads): the plain shape, kept for the comparison of DESIGN §4 (tools/bench_import.py).
//   kImportGeneral  any stride up to 1024 and any offsets: the same slab staging where 128 rows fit in the slab (stride <= 248), rows
//                   read in place otherwise; properties as whole words when the stride and every offset are multiples of 4, from
//                   bytes otherwise.  Correct first: it reads nothing outside [rows, rows + n * stride).
// `rows` is 16-byte aligned (a staging buffer's start); 128 x stride is a multiple of 16, so every workgroup's slab starts aligned.
// Built with -ffp-contract=off.  Plane and row offsets are 64-bit.
#include "gsx_internal.h"
#include "import_math.h"
#include "pod_store.h"

namespace gsx {

namespace {
typedef uint32_t imp_u4v __attribute__((ext_vector_type(4)));
typedef uint32_t imp_u2v __attribute__((ext_vector_type(2)));
constexpr uint32_t kImportSlabBytes = kImportGroup * kImportCanonicalStride;  // 31 744: five workgroups a CU

// the workgroup's `bytes` bytes at src (16-byte aligned) into s_slab: whole 16-byte pieces, then the last bytes one by one
__device__ inline void import_load_slab(const uint8_t* __restrict__ src, uint32_t bytes, uint32_t* s_slab) {
    const uint32_t t = threadIdx.x, n16 = bytes >> 4;
    const imp_u4v* s4 = reinterpret_cast<const imp_u4v*>(src);
    imp_u4v* d4 = reinterpret_cast<imp_u4v*>(s_slab);
    for (uint32_t q = t; q < n16; q += kImportGroup) d4[q] = __builtin_nontemporal_load(s4 + q);
    if (t < (bytes & 15u)) reinterpret_cast<uint8_t*>(s_slab)[(n16 << 4) + t] = src[(n16 << 4) + t];
    __syncthreads();
}
}  // namespace

template <int READ>
__global__ __launch_bounds__(kImportGroup) void k_import_rows(const uint8_t* __restrict__ rows, uint64_t n, uint64_t start, uint64_t model_n,
                                                               PodPlanes pod, ImportLayout lay) {
    __shared__ __attribute__((aligned(16))) uint32_t s_slab[READ == kImportDirect ? 4 : kImportSlabBytes / 4];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kImportGroup;  // the workgroup's first row (base < n: the grid is ceil(n / 128))
    const uint32_t in_group = n - base < kImportGroup ? (uint32_t)(n - base) : kImportGroup;
    const uint32_t stride = READ == kImportGeneral ? lay.stride : kImportCanonicalStride;
    const uint8_t* slab = rows + base * stride;
    const bool staged = READ == kImportSlab || (READ == kImportGeneral && stride <= kImportCanonicalStride);
    if (staged) import_load_slab(slab, in_group * stride, s_slab);  // (uniform)
    if (t >= in_group) return;
    float v[kImportProps];
    if (READ == kImportSlab) {
        const uint2* row = reinterpret_cast<const uint2*>(s_slab) + t * (kImportCanonicalStride / 8);
#pragma unroll
        for (int q = 0; q < kImportProps / 2; ++q) {
            const uint2 w = row[q];
            v[2 * q] = __uint_as_float(w.x);
            v[2 * q + 1] = __uint_as_float(w.y);
        }
    } else if (READ == kImportDirect) {
        const imp_u2v* row = reinterpret_cast<const imp_u2v*>(slab + (uint64_t)t * kImportCanonicalStride);
#pragma unroll
        for (int q = 0; q < kImportProps / 2; ++q) {
            const imp_u2v w = __builtin_nontemporal_load(row + q);
            v[2 * q] = __uint_as_float(w.x);
            v[2 * q + 1] = __uint_as_float(w.y);
        }
    } else {
        // (a generic pointer: LDS when the slab was staged, the caller's rows otherwise)
        const uint8_t* row = staged ? reinterpret_cast<const uint8_t*>(s_slab) + t * stride : slab + (uint64_t)t * stride;
        if (im_is_word_aligned(lay)) im_fetch_words(reinterpret_cast<const uint32_t*>(row), lay, v);  // (uniform)
        else im_fetch_bytes(row, lay, v);
    }
    gsx_gaussian g;
    im_row_to_gaussian(v, &g);
    store_gaussian(pod, model_n, start + base + t, g);
}

hipError_t launch_import_rows(hipStream_t s, const void* d_rows, uint64_t n, uint64_t start, uint64_t model_n, const PodPlanes& pod,
                              const ImportLayout& lay, int read) {
    if (n == 0) return hipSuccess;
    if (lay.stride == 0 || lay.stride > kImportMaxStride) return hipErrorInvalidValue;
    const bool canonical = im_is_canonical(lay);
    if (read == kImportAuto) read = canonical ? kImportSlab : kImportGeneral;
    if (read != kImportGeneral && !canonical) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n + kImportGroup - 1) / kImportGroup)), block(kImportGroup);
    const uint8_t* r = static_cast<const uint8_t*>(d_rows);
    switch (read) {
        case kImportSlab: GSX_LAUNCH(k_import_rows<kImportSlab>, grid, block, 0, s, r, n, start, model_n, pod, lay); break;
        case kImportDirect: GSX_LAUNCH(k_import_rows<kImportDirect>, grid, block, 0, s, r, n, start, model_n, pod, lay); break;
        case kImportGeneral: GSX_LAUNCH(k_import_rows<kImportGeneral>, grid, block, 0, s, r, n, start, model_n, pod, lay); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gsx
