// pod_quant.h — the scalar conversions of compressed pods (spec/RENDER_SPEC.md §2b), written once: the upload conversion and the
// projection pass (kernels_project.hip), the shading of shade records (shade_quads.h), the bake of gsx_model_merge (kernels_merge.hip)
// and the per-kind plane decode of the model operations (pod_planes.h: pod_load_cov, pod_load_sh) all store and read Half and Norm8
// values through these.  Build-internal, device code.
//   f16: IEEE binary16, round to nearest even (what `half::f16::from_f32` does; v_cvt_f16_f32); decoding is exact.
//   snorm8: q = floor(clamp(v,-1,1) * 127 + 0.5) as int8; decode = max(q / 127, -1) (WGSL unpack4x8snorm).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsx {

__device__ inline uint32_t pack_h2(float a, float b) {
    return (uint32_t)__half_as_ushort(__float2half_rn(a)) | ((uint32_t)__half_as_ushort(__float2half_rn(b)) << 16);
}
__device__ inline uint32_t q_snorm8(float v) {
    float c = fminf(fmaxf(v, -1.0f), 1.0f);
    return (uint32_t)(int)floorf(c * 127.0f + 0.5f) & 0xFFu;
}

__device__ inline float h_lo(uint32_t u) { return __half2float(__ushort_as_half((unsigned short)(u & 0xFFFFu))); }
__device__ inline float h_hi(uint32_t u) { return __half2float(__ushort_as_half((unsigned short)(u >> 16))); }
__device__ inline float dq_snorm8(uint32_t word, int byte) {
    int q = (int)(signed char)((word >> (8 * byte)) & 0xFFu);
    return fmaxf((float)q * (1.0f / 127.0f), -1.0f);
}

}  // namespace gsx
