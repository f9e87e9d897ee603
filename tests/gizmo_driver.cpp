// gizmo_driver.cpp — the mask gizmos' wireframe on the CPU: every segment of the records on stdin through csrc/gizmo_math.h, the header
// k_gizmo_setup compiles (tests/test_gizmo_cpu.py; built with the address and undefined-behaviour sanitizers).  Input, one per line:
//   view  m0 .. m15        column-major, as gsx_update_camera takes it
//   proj  m0 .. m15
//   gizmo kind px py pz qx qy qz qw sx sy sz       (colour and width play no part before the projection)
// Output, one line per segment, in draw order:
//   seg <shape> <k> <status> <world end 0: x y z> <world end 1: x y z> <clip end 0: x y z w> <clip end 1: x y z w>
// status: gizmo_near_clip's (0 not drawn, 1 whole, 2 end 0 clipped, 3 end 1 clipped); the clip-space ends are the clipped ones.
#include <cstdio>
#include <cstring>

#include "gizmo_math.h"

using namespace gsx;

static bool read_floats(const char* s, float* out, int n) {
    for (int i = 0; i < n; ++i) {
        int used = 0;
        if (sscanf(s, "%f%n", &out[i], &used) != 1) return false;
        s += used;
    }
    return true;
}

int main() {
    float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, proj[16];
    memcpy(proj, view, sizeof proj);
    GizmoCircle circle;
    gizmo_circle_table(&circle);
    char line[1024];
    unsigned shape = 0;
    while (fgets(line, sizeof line, stdin)) {
        char cmd[32] = "";
        if (sscanf(line, "%31s", cmd) != 1) continue;
        const char* rest = strstr(line, cmd) + strlen(cmd);
        if (!strcmp(cmd, "view") && read_floats(rest, view, 16)) continue;
        if (!strcmp(cmd, "proj") && read_floats(rest, proj, 16)) continue;
        unsigned kind = 0;
        int used = 0;
        float f[10];
        if (!strcmp(cmd, "gizmo") && sscanf(rest, "%u%n", &kind, &used) == 1 && kind <= kGizmoKindEllipsoid && read_floats(rest + used, f, 10)) {
            float rot[9];
            gizmo_quat_rows(f + 3, rot);
            for (uint32_t k = 0; k < gizmo_segment_count(kind); ++k) {
                GizmoVec3 qa, qb;
                gizmo_segment(kind, k, circle.cs, &qa, &qb);
                const GizmoVec3 pa = gizmo_to_world(f, rot, f + 7, qa), pb = gizmo_to_world(f, rot, f + 7, qb);
                GizmoVec4 v0 = gizmo_mat_vec(view, pa.x, pa.y, pa.z, 1.0f), v1 = gizmo_mat_vec(view, pb.x, pb.y, pb.z, 1.0f);
                GizmoVec4 c0 = gizmo_mat_vec(proj, v0.x, v0.y, v0.z, v0.w), c1 = gizmo_mat_vec(proj, v1.x, v1.y, v1.z, v1.w);
                const uint32_t status = gizmo_near_clip(&c0, &v0, &c1, &v1);
                printf("seg %u %u %u %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", shape, k, status, pa.x, pa.y, pa.z,
                       pb.x, pb.y, pb.z, c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w);
            }
            ++shape;
            continue;
        }
        fprintf(stderr, "bad line: %s", line);
        return 2;
    }
    return 0;
}
