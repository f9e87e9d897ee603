// export_driver.cpp — plays csrc/export_math.h on the host for tests/test_export_cpu.py: the header the export kernel includes,
// compiled stand-alone with the address and undefined-behaviour sanitizers and -ffp-contract=off, run as a child process.
// stdin: one request per line, every number a hexadecimal 32-bit word (the bits of a float32 where a float is meant):
//   s c0 .. c5                      the float32 solve of the covariance (xx, xy, xz, yy, yz, zz)  -> "s rot[4] scale[3]"
//   d c0 .. c5                      the same solve with a float64 scalar                            -> "d rot[4] scale[3]"
//   g | p  c0..c5 pos[3] color has_sh sh[45] bake edit[8]
//                                   a gsx_gaussian record (g) or a PLY row (p) of that Gaussian   -> "g 56 words" | "p 62 words"
// stdout: one answer per request, in order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "export_math.h"

using namespace gsx;

static_assert(sizeof(gsx_gaussian) == 4 * kExportGaussianWords, "a record is 56 words");
static_assert(sizeof(gsx_gaussian_edit) == 32, "an edit record is 8 words");

static float as_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main() {
    char* line = nullptr;
    size_t cap = 0;
    std::vector<uint32_t> w;
    std::string out;
    while (getline(&line, &cap, stdin) > 0) {
        const char mode = line[0];
        w.clear();
        char* p = line + 1;
        for (;;) {
            char* end = nullptr;
            const unsigned long v = strtoul(p, &end, 16);
            if (end == p) break;
            w.push_back((uint32_t)v);
            p = end;
        }
        const size_t need = (mode == 's' || mode == 'd') ? 6u : 6u + 3u + 1u + 1u + 45u + 1u + 8u;
        if ((mode != 's' && mode != 'd' && mode != 'g' && mode != 'p') || w.size() != need) {
            fprintf(stderr, "bad request '%c' with %zu words\n", mode, w.size());
            return 2;
        }
        float c[6], rot[4], scale[3];
        for (int k = 0; k < 6; ++k) c[k] = as_float(w[k]);
        if (mode == 'd') ex_solve<double>(c, rot, scale);
        else ex_solve<ExportReal>(c, rot, scale);
        uint32_t row[kExportPlyWords];
        uint32_t words = 7;
        if (mode == 's' || mode == 'd') {
            for (int k = 0; k < 4; ++k) row[k] = ex_bits(rot[k]);
            for (int k = 0; k < 3; ++k) row[4 + k] = ex_bits(scale[k]);
        } else {
            const uint32_t* pos = &w[6];
            const uint32_t color = w[9];
            const bool has_sh = w[10] != 0, bake = w[56] != 0;
            const ExportShWords sh{&w[11]};
            gsx_gaussian_edit e;
            memcpy(&e, &w[57], sizeof e);
            if (mode == 'g') {
                words = kExportGaussianWords;
                if (has_sh) ex_row_gaussian(row, pos, color, sh, rot, scale, bake, e);
                else ex_row_gaussian(row, pos, color, ExportShZero{}, rot, scale, bake, e);
            } else {
                words = kExportPlyWords;
                if (has_sh) ex_row_ply(row, pos, color, sh, rot, scale, bake, e);
                else ex_row_ply(row, pos, color, ExportShZero{}, rot, scale, bake, e);
            }
        }
        out.assign(1, mode);
        char buf[16];
        for (uint32_t k = 0; k < words; ++k) {
            snprintf(buf, sizeof buf, " %x", row[k]);
            out += buf;
        }
        puts(out.c_str());
    }
    free(line);
    return 0;
}
