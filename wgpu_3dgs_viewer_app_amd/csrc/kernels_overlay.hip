// kernels_overlay.hip — the app's mask gizmos and measurement lines, drawn with depth write in front of the splats (gfx950).
//
// SceneCallback::paint draws each model's mask gizmos (src/tab/scene.rs:2283-2293), then the measurement lines, before the splats, `Less`
// with depth write on and alpha blending (scene.rs:2144-2162; src/renderer/measurement.rs:99-116).  A line is six vertices per HitPair
// (measurement.rs:170-174) placed by src/shader/measurement.wgsl:22-67: spec/RENDER_SPEC.md §9 restates that pass.  A gizmo is a
// wireframe of such lines — 12 edges of a box, three 64-chord circles of an ellipsoid — clipped at the near plane first: §10.
//   k_gizmo_setup     one lane per (shape, segment): gizmo_math.h makes the clipped ends, overlay_record the record;
//   k_overlay_setup   one lane per line: the four screen-space corners, the ends' depths, the clamped pixel box, the colour;
//                     both also write one pixel box per batch of 64 records, the union of its drawn records' boxes;
//   k_overlay_raster  one 256-lane workgroup per 16x16 tile, one pixel per lane (the shape of k_depth_limits): every lane walks the
//                     records in array order (gizmos, then lines) — order is program order, no atomics — and keeps its pixel's colour
//                     and depth in registers.  Records come 64 at a time: every wave ballots the 64 boxes against the tile's (the same
//                     ballot in all four waves), a batch nothing of which touches the tile is never staged, the others go through LDS.
//                     Above that, 64 batch boxes are balloted at a time, so a tile reads 16 bytes, not 2 KiB, of a batch far from it.
//                     For a depth-tested frame the launch then does k_depth_limits' work on E(p), from registers.
// Colour is written only for tiles some drawn record's box touches (a flag word per tile says which): a frame with a few lines pays
// the effective depth, 4 bytes a pixel — what k_depth_limits pays for its limits — and a handful of tiles of colour.
#include <algorithm>

#include "gsx_internal.h"

namespace gsx {

constexpr uint32_t kOverlayBatch = 64;                    // records per ballot: one per lane of a wave
constexpr uint32_t kOverlayRecVec = sizeof(OverlayRec) / 16;  // uint4 per record

__device__ __forceinline__ float4 mat_vec(const float* m, float x, float y, float z, float w) {  // column-major
    return make_float4(m[0] * x + m[4] * y + m[8] * z + m[12] * w, m[1] * x + m[5] * y + m[9] * z + m[13] * w,
                       m[2] * x + m[6] * y + m[10] * z + m[14] * w, m[3] * x + m[7] * y + m[11] * z + m[15] * w);
}

// §9's projection of one segment, from its clip-space and view-space ends: the record the raster walks.  Lines and gizmo segments share it.
__device__ __forceinline__ OverlayRec overlay_record(const float4 c0, const float4 v0, const float4 c1, const float4 v1, float cr, float cg,
                                                     float cb, float ca, float line_width, uint32_t w, uint32_t h) {
    const float W = (float)w, H = (float)h;
    OverlayRec r{};
    r.r = cr;
    r.g = cg;
    r.b = cb;
    r.a = ca;
    bool drawn = c0.w > 0.0f && c1.w > 0.0f;  // (hardware would clip an end at w <= 0 in homogeneous space: a stated deviation)
    float dx = (c0.x / c0.w - c1.x / c1.w) * W, dy = (c0.y / c0.w - c1.y / c1.w) * H;
    const float len = sqrtf(dx * dx + dy * dy);
    dx /= len;
    dy /= len;
    drawn = drawn && isfinite(dx) && isfinite(dy);
    const float s = 0.01f * line_width, aspect = H / W;
    const float nx = dy, ny = -dx;
    float minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // end 1 -, end 1 +, end 0 -, end 0 +
        const bool end1 = k < 2;
        const float4 c = end1 ? c1 : c0, v = end1 ? v1 : v0;
        const float sn = (k & 1) ? 1.0f : -1.0f, e = end1 ? -1.0f : 1.0f;
        const float scale = c.w / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
        const float ox = (nx * sn * s + dx * e * s) * aspect * scale, oy = (ny * sn * s + dy * e * s) * scale;
        const float ndx = (c.x + ox) / c.w, ndy = (c.y + oy) / c.w;
        const float px = (ndx * 0.5f + 0.5f) * W, py = (0.5f - ndy * 0.5f) * H;
        r.cx[k] = px;
        r.cy[k] = py;
        drawn = drawn && isfinite(px) && isfinite(py);
        minx = fminf(minx, px);
        maxx = fmaxf(maxx, px);
        miny = fminf(miny, py);
        maxy = fmaxf(maxy, py);
    }
    r.z0 = c0.z / c0.w;
    r.z1 = c1.z / c1.w;
    // both triangles interpolate the same affine function: z1 on the edge through the corners of end 1, z0 on the parallel edge of end 0
    const float ux = dx, uy = -dy;  // the line's direction in pixels (row 0 at the top)
    const float span = (r.cx[2] - r.cx[0]) * ux + (r.cy[2] - r.cy[0]) * uy;
    const float grad = (r.z0 - r.z1) / span;
    r.gx = grad * ux;
    r.gy = grad * uy;
    drawn = drawn && isfinite(r.gx) && isfinite(r.gy) && isfinite(r.z0) && isfinite(r.z1);
    if (drawn) {  // pixel centres x + 0.5 in [minx, maxx]; clamped as floats first (a corner may lie far outside the viewport)
        r.bx0 = (int32_t)fminf(fmaxf(floorf(minx - 0.5f), 0.0f), W);
        r.by0 = (int32_t)fminf(fmaxf(floorf(miny - 0.5f), 0.0f), H);
        r.bx1 = (int32_t)fminf(fmaxf(floorf(maxx + 0.5f) + 1.0f, 0.0f), W);
        r.by1 = (int32_t)fminf(fmaxf(floorf(maxy + 0.5f) + 1.0f, 0.0f), H);
        drawn = r.bx0 < r.bx1 && r.by0 < r.by1;
    }
    r.drawn = drawn ? 1u : 0u;
    return r;
}

// The pixel box of one batch of 64 records — the union of its drawn records' boxes, empty when none is drawn — from the wave that made
// them: the raster's outer level tests it against the tile before it looks at any of the 64.  Every lane of the wave calls this.
__device__ __forceinline__ void overlay_batch_box(const OverlayRec& r, uint32_t batch, uint32_t n_batches, int4* __restrict__ boxes) {
    int x0 = r.drawn ? r.bx0 : INT32_MAX, y0 = r.drawn ? r.by0 : INT32_MAX, x1 = r.drawn ? r.bx1 : INT32_MIN, y1 = r.drawn ? r.by1 : INT32_MIN;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64));
        y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64));
        y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    if ((threadIdx.x & 63u) == 0u && batch < n_batches) boxes[batch] = make_int4(x0, y0, x1, y1);
}

// one lane per line; rec / boxes: where the lines' records and batch boxes start (behind the gizmos', on a batch boundary)
__global__ __launch_bounds__(256) void k_overlay_setup(const gsx_overlay_line* __restrict__ lines, uint32_t n, OverlayCamera cam, uint32_t w,
                                                        uint32_t h, OverlayRec* __restrict__ rec, int4* __restrict__ boxes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    OverlayRec r{};
    if (i < n) {
        const uint4 q0 = reinterpret_cast<const uint4*>(lines)[2 * i], q1 = reinterpret_cast<const uint4*>(lines)[2 * i + 1];
        const float4 v0 = mat_vec(cam.view, __uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z), 1.0f);
        const float4 v1 = mat_vec(cam.view, __uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z), 1.0f);
        const float4 c0 = mat_vec(cam.proj, v0.x, v0.y, v0.z, v0.w), c1 = mat_vec(cam.proj, v1.x, v1.y, v1.z, v1.w);
        r = overlay_record(c0, v0, c1, v1, (float)(q0.w & 255u) / 255.0f, (float)((q0.w >> 8) & 255u) / 255.0f,
                           (float)((q0.w >> 16) & 255u) / 255.0f, (float)(q0.w >> 24) / 255.0f, __uint_as_float(q1.w), w, h);
        rec[i] = r;
    }
    if (boxes) overlay_batch_box(r, i / kOverlayBatch, (n + kOverlayBatch - 1) / kOverlayBatch, boxes);
}

// Mask gizmos (spec §10): one lane per (shape, segment).  buf: the circle table, the shapes' first-record offsets (n_shapes + 1 words,
// host-computed: 12 records a box, 192 an ellipsoid) and the shapes (gizmo_buffer_layout, gsx_internal.h).  Records [n_segs, n_rec) pad
// the region to whole batches with drawn = 0.  gizmo_math.h makes the segment, its world ends and the near clip; the rest is §9.
__global__ __launch_bounds__(256) void k_gizmo_setup(const uint8_t* __restrict__ buf, uint32_t n_shapes, uint32_t n_segs, uint32_t n_rec,
                                                      OverlayCamera cam, uint32_t w, uint32_t h, OverlayRec* __restrict__ rec,
                                                      int4* __restrict__ boxes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    OverlayRec r{};
    if (i < n_segs) {
        const float(*cs)[2] = reinterpret_cast<const float(*)[2]>(buf);
        const uint32_t* off = reinterpret_cast<const uint32_t*>(buf + kGizmoOffsetsAt);
        uint32_t lo = 0, hi = n_shapes;  // the shape whose records hold i: off[lo] <= i < off[lo + 1]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid;
            else hi = mid;
        }
        const gsx_mask_gizmo& g = reinterpret_cast<const gsx_mask_gizmo*>(buf + kGizmoShapesAt)[lo];
        GizmoVec3 qa, qb;
        gizmo_segment(g.kind, i - off[lo], cs, &qa, &qb);
        float rot[9];
        gizmo_quat_rows(g.quat_xyzw, rot);
        const GizmoVec3 pa = gizmo_to_world(g.pos, rot, g.scale, qa), pb = gizmo_to_world(g.pos, rot, g.scale, qb);
        GizmoVec4 v0 = gizmo_mat_vec(cam.view, pa.x, pa.y, pa.z, 1.0f), v1 = gizmo_mat_vec(cam.view, pb.x, pb.y, pb.z, 1.0f);
        GizmoVec4 c0 = gizmo_mat_vec(cam.proj, v0.x, v0.y, v0.z, v0.w), c1 = gizmo_mat_vec(cam.proj, v1.x, v1.y, v1.z, v1.w);
        if (gizmo_near_clip(&c0, &v0, &c1, &v1))
            r = overlay_record(make_float4(c0.x, c0.y, c0.z, c0.w), make_float4(v0.x, v0.y, v0.z, v0.w), make_float4(c1.x, c1.y, c1.z, c1.w),
                               make_float4(v1.x, v1.y, v1.z, v1.w), g.color[0], g.color[1], g.color[2], g.color[3], g.line_width, w, h);
    }
    if (i < n_rec) rec[i] = r;
    if (boxes) overlay_batch_box(r, i / kOverlayBatch, n_rec / kOverlayBatch, boxes);
}

// is p inside edge a -> b of a triangle whose winding sign is s (top-left fill rule; y grows downwards)?  e: the edge function at p
__device__ __forceinline__ bool edge_in(float s, float e, float ex, float ey) {
    e *= s;
    ex *= s;
    ey *= s;
    return e > 0.0f || (e == 0.0f && (ey < 0.0f || (ey == 0.0f && ex > 0.0f)));
}
__device__ __forceinline__ float edge_fn(float ax, float ay, float ex, float ey, float px, float py) { return ex * (py - ay) - ey * (px - ax); }
__device__ __forceinline__ float sign_of(float a) { return a > 0.0f ? 1.0f : (a < 0.0f ? -1.0f : 0.0f); }

template <bool kLimits>
__global__ __launch_bounds__(256) void k_overlay_raster(const OverlayRec* __restrict__ rec, uint32_t n, const int4* __restrict__ boxes,
                                                         const float* __restrict__ depth, uint64_t pitch_bytes, uint32_t w, uint32_t h,
                                                         uint32_t tiles_x, float p22, float p23, float4* __restrict__ rgba,
                                                         uint32_t* __restrict__ tile_flags, float* __restrict__ eff, uint32_t* __restrict__ lim,
                                                         uint2* __restrict__ window) {
    __shared__ uint4 s_rec[kOverlayBatch * kOverlayRecVec];
    __shared__ uint32_t s_max[4], s_min[4];
    const uint32_t tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const uint32_t x = tx * kTile + (threadIdx.x & 15u), y = ty * kTile + (threadIdx.x >> 4);
    const bool in = x < w && y < h;
    float E = 1.0f;
    if (in && depth) E = reinterpret_cast<const float*>(reinterpret_cast<const char*>(depth) + (size_t)y * pitch_bytes)[x];
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, ca = 0.0f;
    const int32_t tx0 = (int32_t)(tx * kTile), ty0 = (int32_t)(ty * kTile);
    const int32_t tx1 = min(tx0 + kTile, (int32_t)w), ty1 = min(ty0 + kTile, (int32_t)h);
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const uint32_t lane = threadIdx.x & 63u;
    bool touched = false;
    // The outer level: lane j of every wave tests the box of batch g0 + j against the tile — again the same ballot in all four waves — and
    // the walk visits the batches it lists, in order.  Without boxes (GSX_OVERLAY_BATCH_BOXES=0) every batch is listed: the flat walk.
    const uint32_t n_batches = (n + kOverlayBatch - 1) / kOverlayBatch;
    for (uint32_t g0 = 0; g0 < n_batches; g0 += 64u) {
        unsigned long long batches;
        if (boxes) {
            bool near = false;
            if (g0 + lane < n_batches) {
                const int4 b = boxes[g0 + lane];
                near = b.x < tx1 && b.z > tx0 && b.y < ty1 && b.w > ty0;
            }
            batches = __ballot(near);
        } else {
            batches = n_batches - g0 >= 64u ? ~0ull : (1ull << (n_batches - g0)) - 1ull;
        }
        while (batches) {
            const uint32_t base = (g0 + (uint32_t)__ffsll((long long)batches) - 1u) * kOverlayBatch;
            batches &= batches - 1ull;
            bool hit = false;
            if (base + lane < n) {
                const uint4* g = reinterpret_cast<const uint4*>(rec + base + lane);
                const uint4 box = g[3];  // bx0, by0, bx1, by1
                hit = g[5].x != 0u && (int32_t)box.x < tx1 && (int32_t)box.z > tx0 && (int32_t)box.y < ty1 && (int32_t)box.w > ty0;
            }
            unsigned long long mask = __ballot(hit);  // the same in every wave of the workgroup: the barriers below are taken by all or none
            if (!mask) continue;
            touched = true;
            __syncthreads();  // (the batch staged before this one has been read)
            const uint32_t vecs = min(kOverlayBatch, n - base) * kOverlayRecVec;
            for (uint32_t k = threadIdx.x; k < vecs; k += 256u) s_rec[k] = reinterpret_cast<const uint4*>(rec + base)[k];
            __syncthreads();
            while (mask) {
                const uint32_t j = (uint32_t)__ffsll((long long)mask) - 1u;
                mask &= mask - 1ull;
                const OverlayRec& r = *reinterpret_cast<const OverlayRec*>(&s_rec[j * kOverlayRecVec]);
                if ((int32_t)x < r.bx0 || (int32_t)x >= r.bx1 || (int32_t)y < r.by0 || (int32_t)y >= r.by1) continue;
                // corners A = end 1 -, B = end 1 +, C = end 0 -, D = end 0 +; triangles (A, B, C) and (C, B, D) share the diagonal B - C, whose edge
                // function is computed once and used with either sign: a pixel centre on it belongs to exactly one of the two
                const float ax = r.cx[0], ay = r.cy[0], bx = r.cx[1], by = r.cy[1], qx = r.cx[2], qy = r.cy[2], dx = r.cx[3], dy = r.cy[3];
                const float bcx = qx - bx, bcy = qy - by;
                const float d = edge_fn(bx, by, bcx, bcy, px, py);
                const float abx = bx - ax, aby = by - ay, cax = ax - qx, cay = ay - qy;
                const float s1 = sign_of(edge_fn(ax, ay, abx, aby, qx, qy));
                bool cover = s1 != 0.0f && edge_in(s1, d, bcx, bcy) && edge_in(s1, edge_fn(ax, ay, abx, aby, px, py), abx, aby) &&
                             edge_in(s1, edge_fn(qx, qy, cax, cay, px, py), cax, cay);
                if (!cover) {
                    const float bdx = dx - bx, bdy = dy - by, dcx = qx - dx, dcy = qy - dy;
                    const float s2 = sign_of(-edge_fn(bx, by, bcx, bcy, dx, dy));
                    cover = s2 != 0.0f && edge_in(s2, -d, -bcx, -bcy) && edge_in(s2, edge_fn(bx, by, bdx, bdy, px, py), bdx, bdy) &&
                            edge_in(s2, edge_fn(dx, dy, dcx, dcy, px, py), dcx, dcy);
                }
                if (!cover) continue;
                const float z = r.z1 + r.gx * (px - ax) + r.gy * (py - ay);
                if (!(z >= 0.0f && z <= 1.0f && z < E)) continue;  // outside [0, 1]: discarded; then `Less`, with depth write
                E = z;
                const float a = r.a, k = 1.0f - a;
                cr = a * r.r + k * cr;
                cg = a * r.g + k * cg;
                cb = a * r.b + k * cb;
                ca = a + k * ca;
            }
        }
    }
    if (in) {
        eff[(size_t)y * w + x] = E;
        if (touched) rgba[(size_t)y * w + x] = make_float4(cr, cg, cb, ca);
    }
    if (threadIdx.x == 0) tile_flags[tile] = touched ? 1u : 0u;
    if (kLimits) {  // k_depth_limits' work, on E(p)
        uint32_t l = 0u;
        if (in) {
            l = depth_limit_key(E, p22, p23);
            lim[(size_t)y * w + x] = l;
        }
        uint32_t m = l, mn = in ? l : kDepthNoLimit;
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
}

// (premultiplied rgb, T) over the overlay over a background colour -> RGBA8 UNORM; k_resolve_rgba8's rounding
__global__ __launch_bounds__(256) void k_resolve_rgba8_overlay(const float4* __restrict__ fb, uint32_t first, uint32_t n, uint32_t w,
                                                                uint32_t tiles_x, float br, float bg, float bb,
                                                                const float4* __restrict__ overlay, const uint32_t* __restrict__ tile_flags,
                                                                uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t px = first + i, x = px % w, y = px / w;
    const float4 p = fb[px];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tile_flags[(y / kTile) * tiles_x + x / kTile]) o = overlay[px];
    const float k = 1.0f - o.w;
    float r = fminf(fmaxf(fmaf(p.w, fmaf(k, br, o.x), p.x), 0.0f), 1.0f);
    float g = fminf(fmaxf(fmaf(p.w, fmaf(k, bg, o.y), p.y), 0.0f), 1.0f);
    float b = fminf(fmaxf(fmaf(p.w, fmaf(k, bb, o.z), p.z), 0.0f), 1.0f);
    float a = fminf(fmaxf(1.0f - p.w * k, 0.0f), 1.0f);
    uint32_t R = (uint32_t)floorf(r * 255.0f + 0.5f), G = (uint32_t)floorf(g * 255.0f + 0.5f);
    uint32_t B = (uint32_t)floorf(b * 255.0f + 0.5f), A = (uint32_t)floorf(a * 255.0f + 0.5f);
    out[i] = R | (G << 8) | (B << 16) | (A << 24);
}

hipError_t launch_overlay(hipStream_t s, const OverlayGizmos& gz, const gsx_overlay_line* lines, uint32_t n, const OverlayCamera& cam,
                          const float* depth, uint64_t pitch_bytes, uint32_t w, uint32_t h, float p22, float p23, OverlayRec* rec, int4* boxes,
                          float4* rgba, uint32_t* tile_flags, float* eff, uint32_t* lim, uint2* window) {
    const uint32_t tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    if (!tiles_x || !tiles_y) return hipSuccess;
    const uint32_t gz_batches = gz.n_rec / kOverlayBatch, n_rec = gz.n_rec + n;  // (the gizmos' records end on a batch boundary)
    if (n_rec <= kOverlayBatch) boxes = nullptr;  // one batch: its own ballot is the cull, a box in front of it one more dependent load
    if (gz.n_rec) GSX_LAUNCH(k_gizmo_setup, dim3((gz.n_rec + 255) / 256), dim3(256), 0, s, gz.buf, gz.n_shapes, gz.n_segs, gz.n_rec, cam, w, h, rec, boxes);
    if (n) GSX_LAUNCH(k_overlay_setup, dim3((n + 255) / 256), dim3(256), 0, s, lines, n, cam, w, h, rec + gz.n_rec, boxes ? boxes + gz_batches : nullptr);
    if (lim)
        GSX_LAUNCH(k_overlay_raster<true>, dim3(tiles_x * tiles_y), dim3(256), 0, s, rec, n_rec, boxes, depth, pitch_bytes, w, h, tiles_x, p22, p23,
                   rgba, tile_flags, eff, lim, window);
    else
        GSX_LAUNCH(k_overlay_raster<false>, dim3(tiles_x * tiles_y), dim3(256), 0, s, rec, n_rec, boxes, depth, pitch_bytes, w, h, tiles_x, p22, p23,
                   rgba, tile_flags, eff, lim, window);
    return hipGetLastError();
}

hipError_t launch_resolve_rgba8_overlay(hipStream_t s, const float4* fb, uint32_t first, uint32_t n_px, uint32_t w, float bg_r, float bg_g,
                                        float bg_b, const float4* overlay_rgba, const uint32_t* tile_flags, uint32_t* out_rgba8) {
    if (!n_px) return hipSuccess;
    GSX_LAUNCH(k_resolve_rgba8_overlay, dim3((n_px + 255) / 256), dim3(256), 0, s, fb, first, n_px, w, (w + kTile - 1) / kTile, bg_r, bg_g, bg_b,
               overlay_rgba, tile_flags, out_rgba8);
    return hipGetLastError();
}

}  // namespace gsx
