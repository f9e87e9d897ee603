// bounds_driver.cpp — csrc/bounds_math.h (the trimmed box of gsx_model_bounds) played on the host, for tests/test_bounds_cpu.py:
// a stand-alone program the test builds with the address and undefined-behaviour sanitizers.
// stdin:  "k <K>", then one "v <float32 as %a>" per value of ONE axis (all finite).
// stdout: "axis <live> <lo> <hi> <width>"        the axis over [min, max] of the values
//         "bins <bin of each value>"              (live axes only)
//         "edges <edge 0> ... <edge 2048>"        (live axes only)
//         "scan <pos_lo> <before_lo> <pos_hi> <before_hi>"   bounds_scan over the histogram from both ends (live axes only)
//         "trim <trim_min> <trim_max>"
//         "empty <18 floats>"                     the float fields of a call that counted nothing
// Floats are printed as %a: exact.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bounds_math.h"

int main() {
    unsigned long long k = 0;
    std::vector<float> values;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        double d;
        if (sscanf(line, "k %llu", &k) == 1) continue;
        if (sscanf(line, "v %la", &d) == 1) values.push_back((float)d);
    }
    if (values.empty()) {
        fprintf(stderr, "no values\n");
        return 2;
    }
    float lo = values[0], hi = values[0];
    for (float v : values) {
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    const gsx::BoundsAxis ax = gsx::bounds_axis(lo, hi);
    printf("axis %d %a %a %a\n", ax.live ? 1 : 0, (double)ax.lo, (double)ax.hi, (double)ax.width);
    uint32_t pos_lo = gsx::kBoundsBins, pos_hi = gsx::kBoundsBins;
    if (ax.live) {
        std::vector<uint32_t> hist(gsx::kBoundsBins, 0u);
        printf("bins");
        for (float v : values) {
            const uint32_t b = gsx::bounds_bin(ax, v);
            if (b >= gsx::kBoundsBins) {
                fprintf(stderr, "bin %u out of range\n", b);
                return 3;
            }
            hist[b] += 1;
            printf(" %u", b);
        }
        printf("\nedges");
        for (uint32_t b = 0; b <= gsx::kBoundsBins; ++b) printf(" %a", (double)gsx::bounds_edge(ax, b));
        uint64_t before_lo = 0, before_hi = 0;
        pos_lo = gsx::bounds_scan(hist.data(), gsx::kBoundsBins, false, k, &before_lo);
        pos_hi = gsx::bounds_scan(hist.data(), gsx::kBoundsBins, true, k, &before_hi);
        printf("\nscan %u %llu %u %llu\n", pos_lo, (unsigned long long)before_lo, pos_hi, (unsigned long long)before_hi);
    }
    printf("trim %a %a\n", (double)gsx::bounds_trim_lo(ax, pos_lo), (double)gsx::bounds_trim_hi(ax, pos_hi));
    float empty[18];
    memset(empty, 0xFF, sizeof empty);
    gsx::bounds_empty(empty);
    printf("empty");
    for (float f : empty) printf(" %a", (double)f);
    printf("\n");
    return 0;
}
