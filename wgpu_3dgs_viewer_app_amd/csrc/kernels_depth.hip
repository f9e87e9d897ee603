// kernels_depth.hip — the caller's depth buffer as per-pixel limits and per-tile depth bounds (gfx950).
//
// The reference draws its splats with a depth test against what the mask gizmos and the measurement lines wrote before them
// (MultiModelViewer::new_with(.., Some(DepthStencilState { Depth32Float, depth_write_enabled: false, Less }), ..),
// src/tab/scene.rs:1969-1980; SceneCallback::paint, scene.rs:2283-2314).  Here the test is made in the depth-key domain
// (spec §6, "Depth test"): with a projection whose third and fourth rows depend on view z alone (P32 = -1), NDC depth
// z_ndc = P23 / d - P22 of a splat at view depth d is < D(p) exactly when d < P23 / (D(p) + P22).  So every pixel gets the
// limit key bits(P23 / (D + P22)) once per frame, and the compositor compares one key per (record, pixel).
// Per 16x16 tile the maximum of its pixels' limits is the depth bound: no record at or behind it can touch any pixel of the
// tile, so it caps the tile's window (admission, binning) and such records never enter the depth sort.
// Bandwidth-trivial: 4 bytes read and 4 written per pixel (8 MB at 1080p), one workgroup per tile.
#include <algorithm>

#include "gsx_internal.h"

namespace gsx {

// (kDepthNoLimit and depth_limit_key live in gsx_internal.h: the overlay raster, kernels_overlay.hip, makes the same keys from E(p))

// one 256-lane workgroup per tile, one pixel per lane.  Behind the w x h limits, one word per tile: 1 when no pixel of the tile has a
// limit (the minimum of its pixels' limits is "none") — the compositors take such a tile through their loop without the compare.
__global__ __launch_bounds__(256) void k_depth_limits(const float* __restrict__ depth, uint64_t pitch_bytes, uint32_t w, uint32_t h,
                                                       uint32_t tiles_x, float p22, float p23, uint32_t* __restrict__ lim,
                                                       uint2* __restrict__ window) {
    __shared__ uint32_t s_max[4], s_min[4];
    const uint32_t tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const uint32_t x = tx * kTile + (threadIdx.x & 15u), y = ty * kTile + (threadIdx.x >> 4);
    uint32_t l = 0u;  // (outside the image: no pixel to keep open)
    const bool in = x < w && y < h;
    if (in) {
        const float d = reinterpret_cast<const float*>(reinterpret_cast<const char*>(depth) + (size_t)y * pitch_bytes)[x];
        l = depth_limit_key(d, p22, p23);
        lim[(size_t)y * w + x] = l;
    }
    uint32_t m = l, mn = in ? l : kDepthNoLimit;  // (outside the image: nothing to limit either)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
        s_max[threadIdx.x >> 6] = m;
        s_min[threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        window[tile] = make_uint2(0u, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
        lim[(size_t)w * h + tile] = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3])) == kDepthNoLimit ? 1u : 0u;
    }
}

hipError_t launch_depth_limits(hipStream_t s, const float* depth, uint64_t pitch_bytes, uint32_t w, uint32_t h, float p22, float p23,
                               uint32_t* lim, uint2* window) {
    const uint32_t tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    if (!tiles_x || !tiles_y) return hipSuccess;
    GSX_LAUNCH(k_depth_limits, dim3(tiles_x * tiles_y), dim3(256), 0, s, depth, pitch_bytes, w, h, tiles_x, p22, p23, lim, window);
    return hipGetLastError();
}

}  // namespace gsx
