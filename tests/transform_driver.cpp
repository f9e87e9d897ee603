// tests/transform_driver.cpp — csrc/transform_math.h played on the host, for tests/test_transform_cpu.py: a stand-alone program, built
// with -fsanitize=address,undefined and -ffp-contract=off and run as a child process.  Commands on stdin, one a line; floats travel as
// the eight hex digits of their bits, so nothing is lost in print:
//   mode  <pos 3> <quat 4> <scale 3>                 -> "mode <0..3>" (transform_mode), "rot <0|1>" (transform_rotation_is_identity)
//   valid <pos 3> <quat 4> <scale 3> <pivot 3>       -> "valid <0|1>" (transform_is_valid), "pivot0 <0|1>" (transform_pivot_is_zero)
//   xf    <R 9> <scale 3> <pos 3> <pivot 3>          -> sets the transform of the following points; prints nothing
//   p     <x y z>                                    -> "o <x' y' z'>" (transform_position; the pivot rule from transform_pivot_is_zero)
//   desc                                             -> "desc <sizeof> <offsets of filter flags pos quat scale pivot reserved>"
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

#include "gsx.h"
#include "transform_math.h"

static_assert(sizeof(gsx_transform_desc) == 64, "gsx_transform_desc is 64 bytes");

static bool read_floats(std::istringstream& in, float* out, int n) {
    for (int k = 0; k < n; ++k) {
        std::string tok;
        if (!(in >> tok)) return false;
        const uint32_t u = (uint32_t)strtoul(tok.c_str(), nullptr, 16);
        memcpy(&out[k], &u, 4);
    }
    return true;
}
static void print_floats(const char* tag, const float* v, int n) {
    printf("%s", tag);
    for (int k = 0; k < n; ++k) {
        uint32_t u;
        memcpy(&u, &v[k], 4);
        printf(" %08x", u);
    }
    printf("\n");
}

int main() {
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, s[3] = {1, 1, 1}, t[3] = {0, 0, 0}, c[3] = {0, 0, 0};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        float pos[3], quat[4], scale[3], pivot[3];
        if (cmd == "mode") {
            if (!read_floats(in, pos, 3) || !read_floats(in, quat, 4) || !read_floats(in, scale, 3)) return 2;
            printf("mode %d\nrot %d\n", gsx::transform_mode(pos, quat, scale), (int)gsx::transform_rotation_is_identity(quat));
        } else if (cmd == "valid") {
            if (!read_floats(in, pos, 3) || !read_floats(in, quat, 4) || !read_floats(in, scale, 3) || !read_floats(in, pivot, 3)) return 2;
            printf("valid %d\npivot0 %d\n", (int)gsx::transform_is_valid(pos, quat, scale, pivot), (int)gsx::transform_pivot_is_zero(pivot));
        } else if (cmd == "xf") {
            if (!read_floats(in, R, 9) || !read_floats(in, s, 3) || !read_floats(in, t, 3) || !read_floats(in, c, 3)) return 2;
        } else if (cmd == "p") {
            float p[3], o[3];
            if (!read_floats(in, p, 3)) return 2;
            gsx::transform_position(R, s, t, c, !gsx::transform_pivot_is_zero(c), p, o);
            print_floats("o", o, 3);
        } else if (cmd == "desc") {
            printf("desc %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gsx_transform_desc), offsetof(gsx_transform_desc, filter), offsetof(gsx_transform_desc, flags),
                   offsetof(gsx_transform_desc, pos), offsetof(gsx_transform_desc, quat), offsetof(gsx_transform_desc, scale),
                   offsetof(gsx_transform_desc, pivot), offsetof(gsx_transform_desc, reserved));
        } else {
            fprintf(stderr, "unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
