// pod_store.h — the write side of an upload, written once for the kernels that fill the resident pod planes from Gaussians
// (k_convert and k_pack_pod in kernels_project.hip, k_import_rows in kernels_import.hip): the plane stores of a pod kind
// (spec/RENDER_SPEC.md §2b; the scalar conversions are pod_quant.h's), shade records included, and the record -> planes step of §2
// (store_gaussian: what gaussians_buffer.update_range does to one gs::Gaussian).  Device only, build-internal.
// Built with -ffp-contract=off: the covariance is the same bits wherever it is computed.
#pragma once
#include "gsx_internal.h"
#include "pod_quant.h"

namespace gsx {

__device__ inline float ddot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// ---- quantisation (spec/RENDER_SPEC.md §2b) ----
// pack_h2, q_snorm8 and their decoders: pod_quant.h (shared with kernels_merge.hip)

__device__ inline void store_sh(const PodPlanes& pod, uint64_t model_n, uint64_t i, const float* s45) {
    if (pod.sh_kind == GSX_SH_SINGLE) {
#pragma unroll
        for (int p = 0; p < kShPlanes4; ++p) {
            const float4 v = make_float4(s45[4 * p], s45[4 * p + 1], s45[4 * p + 2], s45[4 * p + 3]);
            pod.sh4[(uint64_t)p * model_n + i] = v;
            if (pod.sh_aos) pod.sh_aos[i * pod.aos_stride + p] = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));
        }
        pod.sh1[i] = s45[44];
        if (pod.sh_aos) pod.sh_aos[i * pod.aos_stride + 11] = make_uint4(__float_as_uint(s45[44]), 0u, 0u, 0u);
    } else if (pod.sh_kind == GSX_SH_HALF) {
        for (int p = 0; p < 6; ++p) {
            uint32_t w[4];
            for (int k = 0; k < 4; ++k) {
                int f0 = 8 * p + 2 * k, f1 = f0 + 1;
                w[k] = pack_h2(f0 < 45 ? s45[f0] : 0.0f, f1 < 45 ? s45[f1] : 0.0f);
            }
            pod.sh_h[(uint64_t)p * model_n + i] = make_uint4(w[0], w[1], w[2], w[3]);
            if (pod.sh_aos) pod.sh_aos[i * pod.aos_stride + p] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else if (pod.sh_kind == GSX_SH_NORM8) {
        for (int p = 0; p < 3; ++p) {
            uint32_t w[4];
            for (int k = 0; k < 4; ++k) {
                uint32_t v = 0;
                for (int b = 0; b < 4; ++b) {
                    int f = 16 * p + 4 * k + b;
                    v |= (f < 45 ? q_snorm8(s45[f]) : 0u) << (8 * b);
                }
                w[k] = v;
            }
            pod.sh_q[(uint64_t)p * model_n + i] = make_uint4(w[0], w[1], w[2], w[3]);
            if (pod.sh_aos) pod.sh_aos[i * pod.aos_stride + p] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// the shade record's geometry words: position + colour word and the covariance (as the pod stores it) beside the SH words
__device__ inline void store_aos_geometry(const PodPlanes& pod, uint64_t i, float4 pc, float c0, float c1, float c2, float c3, float c4,
                                          float c5) {
    if (!pod.sh_aos || !pod.aos_geo) return;
    uint4* r = pod.sh_aos + i * pod.aos_stride + pod.aos_geo;
    r[0] = make_uint4(__float_as_uint(pc.x), __float_as_uint(pc.y), __float_as_uint(pc.z), __float_as_uint(pc.w));
    if (pod.cov_kind == GSX_COV3D_SINGLE) {
        r[1] = make_uint4(__float_as_uint(c0), __float_as_uint(c1), __float_as_uint(c2), __float_as_uint(c3));
        r[2] = make_uint4(__float_as_uint(c4), __float_as_uint(c5), 0u, 0u);
    } else {
        r[1] = make_uint4(pack_h2(c0, c1), pack_h2(c2, c3), pack_h2(c4, c5), 0u);  // (the same halves store_cov writes)
    }
}

__device__ inline void store_cov(const PodPlanes& pod, uint64_t i, float c0, float c1, float c2, float c3, float c4, float c5) {
    if (pod.cov_kind == GSX_COV3D_SINGLE) {
        pod.cov_a[i] = make_float4(c0, c1, c2, c3);
        pod.cov_b[i] = make_float2(c4, c5);
    } else {
        pod.cov_h[i] = make_uint2(pack_h2(c0, c1), pack_h2(c2, c3));
        pod.cov_h2[i] = pack_h2(c4, c5);
    }
}

// One gs::Gaussian into Gaussian i of the planes (spec §2): covariance R diag(s)^2 R^T in float32, the colour word, position, SH.
__device__ inline void store_gaussian(const PodPlanes& pod, uint64_t model_n, uint64_t i, const gsx_gaussian& g) {
    float x = g.rot[0], y = g.rot[1], z = g.rot[2], w = g.rot[3];
    float x2 = x + x, y2 = y + y, z2 = z + z;
    float xx = x * x2, xy = x * y2, xz = x * z2;
    float yy = y * y2, yz = y * z2, zz = z * z2;
    float wx = w * x2, wy = w * y2, wz = w * z2;
    float R[9] = {1.0f - (yy + zz), xy - wz, xz + wy, xy + wz, 1.0f - (xx + zz), yz - wx, xz - wy, yz + wx,
                  1.0f - (xx + yy)};
    float M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r * 3 + c] = R[r * 3 + c] * g.scale[c];
    float c0 = ddot3(M[0], M[1], M[2], M[0], M[1], M[2]);
    float c1 = ddot3(M[0], M[1], M[2], M[3], M[4], M[5]);
    float c2 = ddot3(M[0], M[1], M[2], M[6], M[7], M[8]);
    float c3 = ddot3(M[3], M[4], M[5], M[3], M[4], M[5]);
    float c4 = ddot3(M[3], M[4], M[5], M[6], M[7], M[8]);
    float c5 = ddot3(M[6], M[7], M[8], M[6], M[7], M[8]);
    uint32_t col = (uint32_t)g.color[0] | ((uint32_t)g.color[1] << 8) | ((uint32_t)g.color[2] << 16) |
                   ((uint32_t)g.color[3] << 24);
    pod.pc[i] = make_float4(g.pos[0], g.pos[1], g.pos[2], __uint_as_float(col));
    store_cov(pod, i, c0, c1, c2, c3, c4, c5);
    store_aos_geometry(pod, i, make_float4(g.pos[0], g.pos[1], g.pos[2], __uint_as_float(col)), c0, c1, c2, c3, c4, c5);
    store_sh(pod, model_n, i, &g.sh[0][0]);
}

}  // namespace gsx
