// pod_planes.h — a stored Gaussian by pod kind, written once for the model operations that read the resident planes back
// (k_extract_scatter, k_merge_bake, k_export_rows, k_convert_kind): the record sizes of a kind, the exact dequantisation of a
// Gaussian's covariance and SH planes (spec/RENDER_SPEC.md §2b; the scalar conversions are pod_quant.h's), the encoders that turn
// decoded values in registers into the words of a kind (pod_encode_cov, pod_encode_sh: k_convert_kind), and the launch dispatch over
// the eight (sh_kind, cov_kind) pairs.  Build-internal.
#pragma once
#include <type_traits>

#include "gsx_internal.h"
#include "pod_quant.h"

namespace gsx {

// the shade record of a kind (aos_layout, gsx_internal.h), as constants
template <int SH, int COV>
struct PodKind {
    static constexpr uint32_t word(bool stride) {
        uint32_t s = 0, g = 0;
        aos_layout(SH, COV, &s, &g);
        return stride ? s : g;
    }
    static constexpr uint32_t kShWords = word(false);  // uint4 words of SH in front of a record's pc word: 12, 6, 3, 0
    static constexpr uint32_t kStride = word(true);    // uint4 words of a record: 16, 12 or 8, 8; 0 = an Sh None pod has none
};

// the six covariance floats xx, xy, xz, yy, yz, zz of Gaussian i (Single: the stored bits; Half: decoded, exact)
template <int COV>
__device__ inline void pod_load_cov(const ExtractPlanes& src, uint64_t i, float c[6]) {
    if (COV == GSX_COV3D_SINGLE) {
        const uint4 a = src.cov_a[i];
        const uint2 b = src.cov_b[i];
        c[0] = __uint_as_float(a.x); c[1] = __uint_as_float(a.y); c[2] = __uint_as_float(a.z); c[3] = __uint_as_float(a.w);
        c[4] = __uint_as_float(b.x); c[5] = __uint_as_float(b.y);
    } else {
        const uint2 a = src.cov_h[i];
        const uint32_t b = src.cov_h2[i];
        c[0] = h_lo(a.x); c[1] = h_hi(a.x); c[2] = h_lo(a.y); c[3] = h_hi(a.y); c[4] = h_lo(b); c[5] = h_hi(b);
    }
}

// the SH floats of Gaussian i, index 3 * coefficient + channel (Single: the stored bits, s[45 .. 47] zero; Half and Norm8: decoded,
// exact, s[45 .. 47] the decoded spare values of the last word); None: nothing is written
template <int SH>
__device__ inline void pod_load_sh(const ExtractPlanes& src, uint64_t n_src, uint64_t i, float s[48]) {
    if (SH == GSX_SH_SINGLE) {
#pragma unroll
        for (int p = 0; p < kShPlanes4; ++p) {
            const uint4 v = src.sh4[(uint64_t)p * n_src + i];
            s[4 * p] = __uint_as_float(v.x); s[4 * p + 1] = __uint_as_float(v.y); s[4 * p + 2] = __uint_as_float(v.z); s[4 * p + 3] = __uint_as_float(v.w);
        }
        s[44] = __uint_as_float(src.sh1[i]);
        s[45] = s[46] = s[47] = 0.0f;
    } else if (SH == GSX_SH_HALF) {
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const uint4 v = src.sh_h[(uint64_t)p * n_src + i];
            const uint32_t ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s[8 * p + 2 * q] = h_lo(ww[q]);
                s[8 * p + 2 * q + 1] = h_hi(ww[q]);
            }
        }
    } else if (SH == GSX_SH_NORM8) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const uint4 v = src.sh_q[(uint64_t)p * n_src + i];
            const uint32_t ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[16 * p + 4 * q + e] = dq_snorm8(ww[q], e);
        }
    }
}

// ---- the write side, in registers (k_convert_kind): the words a pod of the kind stores for decoded values, quantised once ----
// The covariance c[0 .. 5] as the words of kind COV.  Single: g1 = {xx, xy, xz, yy} (cov_a), g2 = {yz, zz, 0, 0} (cov_b = its first
// two words); Half: g1 = {xx|xy, xz|yy, yz|zz, 0} (cov_h = its first two words, cov_h2 the third), g2 zero.  g1, then for Single g2,
// are also the covariance words of a shade record.
template <int COV>
__device__ inline void pod_encode_cov(const float c[6], uint4& g1, uint4& g2) {
    if (COV == GSX_COV3D_SINGLE) {
        g1 = make_uint4(__float_as_uint(c[0]), __float_as_uint(c[1]), __float_as_uint(c[2]), __float_as_uint(c[3]));
        g2 = make_uint4(__float_as_uint(c[4]), __float_as_uint(c[5]), 0u, 0u);
    } else {
        g1 = make_uint4(pack_h2(c[0], c[1]), pack_h2(c[2], c[3]), pack_h2(c[4], c[5]), 0u);
        g2 = make_uint4(0u, 0u, 0u, 0u);
    }
}

// The SH floats s[0 .. 44] as the words of kind SH: rec[p] is plane p's word of the Gaussian and word p of its shade record (Single:
// rec[0 .. 10] the sh4 planes, rec[11] = {float 44, 0, 0, 0}, whose first word is the sh1 plane's; Half: rec[0 .. 5]; Norm8:
// rec[0 .. 2]).  The spare slots at floats 45 and above are zero whatever s holds there.  None: nothing is written.
template <int SH>
__device__ inline void pod_encode_sh(const float s[48], uint4* rec) {
    if (SH == GSX_SH_SINGLE) {
#pragma unroll
        for (int p = 0; p < kShPlanes4; ++p)
            rec[p] = make_uint4(__float_as_uint(s[4 * p]), __float_as_uint(s[4 * p + 1]), __float_as_uint(s[4 * p + 2]), __float_as_uint(s[4 * p + 3]));
        rec[11] = make_uint4(__float_as_uint(s[44]), 0u, 0u, 0u);
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
        }
    }
}

// f(sh, cov) with the pod kind as two std::integral_constant<int, ...>: the one ladder over the kinds a launcher instantiates
template <class F>
inline hipError_t dispatch_pod_kind(int sh_kind, int cov_kind, F&& f) {
    auto with_sh = [&](auto sh) -> hipError_t {
        if (cov_kind == GSX_COV3D_SINGLE) return f(sh, std::integral_constant<int, GSX_COV3D_SINGLE>{});
        if (cov_kind == GSX_COV3D_HALF) return f(sh, std::integral_constant<int, GSX_COV3D_HALF>{});
        return hipErrorInvalidValue;
    };
    switch (sh_kind) {
        case GSX_SH_SINGLE: return with_sh(std::integral_constant<int, GSX_SH_SINGLE>{});
        case GSX_SH_HALF: return with_sh(std::integral_constant<int, GSX_SH_HALF>{});
        case GSX_SH_NORM8: return with_sh(std::integral_constant<int, GSX_SH_NORM8>{});
        case GSX_SH_NONE: return with_sh(std::integral_constant<int, GSX_SH_NONE>{});
    }
    return hipErrorInvalidValue;
}

}  // namespace gsx
