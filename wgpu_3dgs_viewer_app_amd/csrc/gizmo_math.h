// gizmo_math.h — the mask gizmos' wireframe (spec/RENDER_SPEC.md §10, "Mask gizmos"), written once: k_gizmo_setup
// (kernels_overlay.hip) and the host restatement of tests/gizmo_driver.cpp both include it, so the two cannot drift.
// It holds segment k of a shape in the shape frame, the shape-to-world transform of §2c and the clip against the near plane;
// everything after that is §9's projection (overlay_record, kernels_overlay.hip).
// Plain float32 arithmetic, <math.h> only; no HIP include (the functions are __host__ __device__ under hipcc).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GSX_GZ_HD __host__ __device__
#else
#define GSX_GZ_HD
#endif

namespace gsx {

constexpr uint32_t kGizmoCircleSegs = 64;                    // GSX_GIZMO_CIRCLE_SEGMENTS: chords per circle
constexpr uint32_t kGizmoBoxSegs = 12;                       // the edges of the box
constexpr uint32_t kGizmoEllipsoidSegs = 3 * kGizmoCircleSegs;  // three circles
constexpr uint32_t kGizmoKindBox = 0, kGizmoKindEllipsoid = 1;  // gsx_mask_shape_kind

struct GizmoVec3 {
    float x, y, z;
};
struct GizmoVec4 {
    float x, y, z, w;
};
// (cos, sin) of 2 pi j / 64, evaluated in float64 and rounded to float32 — on the host, once: the table is data wherever it is used
struct GizmoCircle {
    float cs[kGizmoCircleSegs][2];
};
inline void gizmo_circle_table(GizmoCircle* t) {
    for (uint32_t j = 0; j < kGizmoCircleSegs; ++j) {
        const double a = 2.0 * 3.14159265358979323846 * (double)j / (double)kGizmoCircleSegs;
        t->cs[j][0] = (float)cos(a);
        t->cs[j][1] = (float)sin(a);
    }
}

GSX_GZ_HD inline uint32_t gizmo_segment_count(uint32_t kind) { return kind == kGizmoKindBox ? kGizmoBoxSegs : kGizmoEllipsoidSegs; }

// corner i of the box: bit 0 of i is the sign of x, bit 1 of y, bit 2 of z (clear: -1, set: +1)
GSX_GZ_HD inline GizmoVec3 gizmo_box_corner(uint32_t i) {
    return GizmoVec3{(i & 1u) ? 1.0f : -1.0f, (i & 2u) ? 1.0f : -1.0f, (i & 4u) ? 1.0f : -1.0f};
}

// Segment k of a shape, in the shape frame (the boundary of the set of §2c: the unit box, the unit ball).
// Box: four edges along x, then four along y, then four along z; within an axis by ascending lower corner, ends in ascending corner index.
// Ellipsoid: the unit circles in the planes q_z = 0, q_x = 0, q_y = 0, chord j of each from angle 2 pi j / 64 to 2 pi (j + 1) / 64:
//   q_z = 0: (cos, sin, 0)     q_x = 0: (0, cos, sin)     q_y = 0: (sin, 0, cos)
GSX_GZ_HD inline void gizmo_segment(uint32_t kind, uint32_t k, const float (*cs)[2], GizmoVec3* a, GizmoVec3* b) {
    if (kind == kGizmoKindBox) {
        const uint32_t axis = k >> 2, j = k & 3u, step = 1u << axis;
        // the four corners whose bit `axis` is clear, ascending: the low bits of j below the axis bit, the rest above it
        const uint32_t lo = (j & (step - 1u)) | ((j & ~(step - 1u)) << 1);
        *a = gizmo_box_corner(lo);
        *b = gizmo_box_corner(lo + step);
        return;
    }
    const uint32_t plane = k / kGizmoCircleSegs, j0 = k % kGizmoCircleSegs, j1 = (j0 + 1u) % kGizmoCircleSegs;
    const float c0 = cs[j0][0], s0 = cs[j0][1], c1 = cs[j1][0], s1 = cs[j1][1];
    if (plane == 0) {
        *a = GizmoVec3{c0, s0, 0.0f};
        *b = GizmoVec3{c1, s1, 0.0f};
    } else if (plane == 1) {
        *a = GizmoVec3{0.0f, c0, s0};
        *b = GizmoVec3{0.0f, c1, s1};
    } else {
        *a = GizmoVec3{s0, 0.0f, c0};
        *b = GizmoVec3{s1, 0.0f, c1};
    }
}

// the rotation of a quaternion (x, y, z, w), row-major: quat_to_rows' arithmetic (the mask's, kernels_project.hip)
GSX_GZ_HD inline void gizmo_quat_rows(const float q[4], float r[9]) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float x2 = x + x, y2 = y + y, z2 = z + z;
    const float xx = x * x2, xy = x * y2, xz = x * z2;
    const float yy = y * y2, yz = y * z2, zz = z * z2;
    const float wx = w * x2, wy = w * y2, wz = w * z2;
    r[0] = 1.0f - (yy + zz);
    r[1] = xy - wz;
    r[2] = xz + wy;
    r[3] = xy + wz;
    r[4] = 1.0f - (xx + zz);
    r[5] = yz - wx;
    r[6] = xz - wy;
    r[7] = yz + wx;
    r[8] = 1.0f - (xx + yy);
}

// p_w = pos_s + R_s (scale_s (.) q): the inverse of the map §2c tests with
GSX_GZ_HD inline GizmoVec3 gizmo_to_world(const float pos[3], const float rot[9], const float scale[3], GizmoVec3 q) {
    const float sx = scale[0] * q.x, sy = scale[1] * q.y, sz = scale[2] * q.z;
    return GizmoVec3{((rot[0] * sx + rot[1] * sy) + rot[2] * sz) + pos[0], ((rot[3] * sx + rot[4] * sy) + rot[5] * sz) + pos[1],
                     ((rot[6] * sx + rot[7] * sy) + rot[8] * sz) + pos[2]};
}

// m (column-major, as gsx_update_camera takes it) times (x, y, z, w)
GSX_GZ_HD inline GizmoVec4 gizmo_mat_vec(const float* m, float x, float y, float z, float w) {
    return GizmoVec4{m[0] * x + m[4] * y + m[8] * z + m[12] * w, m[1] * x + m[5] * y + m[9] * z + m[13] * w,
                     m[2] * x + m[6] * y + m[10] * z + m[14] * w, m[3] * x + m[7] * y + m[11] * z + m[15] * w};
}

GSX_GZ_HD inline GizmoVec4 gizmo_lerp(GizmoVec4 a, GizmoVec4 b, float t) {
    return GizmoVec4{a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z), a.w + t * (b.w - a.w)};
}

// The clip against the near plane, c.z >= 0 (z in [0, w]: wgpu's clip volume), of the segment with clip-space ends c0, c1 and view-space
// ends v0, v1.  An end outside is replaced by the point at t = c0.z / (c0.z - c1.z) of both.  Returns 0: both ends outside (or a z that
// is not a number), not drawn; 1: untouched; 2: end 0 was replaced; 3: end 1 was.
GSX_GZ_HD inline uint32_t gizmo_near_clip(GizmoVec4* c0, GizmoVec4* v0, GizmoVec4* c1, GizmoVec4* v1) {
    const bool in0 = c0->z >= 0.0f, in1 = c1->z >= 0.0f;
    if (in0 && in1) return 1u;
    if (!in0 && !in1) return 0u;
    const float t = c0->z / (c0->z - c1->z);
    const GizmoVec4 c = gizmo_lerp(*c0, *c1, t), v = gizmo_lerp(*v0, *v1, t);
    if (!in0) {
        *c0 = c;
        *v0 = v;
        return 2u;
    }
    *c1 = c;
    *v1 = v;
    return 3u;
}

}  // namespace gsx
