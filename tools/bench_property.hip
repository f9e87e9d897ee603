// tools/bench_property.hip — the kernel frame of the model properties (csrc/kernels_property.hip) on planes of its own, timed with HIP
// events around the launches.  The kernel file is included as source; nothing of libgsx is linked.  Not part of the product;
// tools/bench_property.py builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_property.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_property_kernels
//   tools/bench_property_kernels <n> [samples=5] [reps=10]
// Rows: class (pc = properties 0..9 from the 16-byte element; cov_single / cov_half = the scales) x mode (values, reduce, hist at 256
// and 4096 bins over a uniform and over a one-bin-concentrated property, select), ms per launch: the median of `samples` windows
// of `reps` launches (each with its one-workgroup finish), every sample listed; and the bytes the launch has to move / that time.
// Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_property.hip"

using namespace gsx;
#define CK(x)                                                       \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) {                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            exit(1);                                                \
        }                                                           \
    } while (0)

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}
static uint16_t half_bits(float f) {  // (positive normal values only: what the covariances below hold)
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)((((u >> 23) - 112u) << 10) | ((u >> 13) & 0x3FFu));
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <n> [samples] [reps]\n", argv[0]);
        return 2;
    }
    const uint64_t n = strtoull(argv[1], nullptr, 10);
    const int samples = argc > 2 ? atoi(argv[2]) : 5, reps = argc > 3 ? atoi(argv[3]) : 10;
    if (n == 0 || samples < 1 || reps < 1 || (uint64_t)(reps + 2) * n > 0xFFFFFFFFull) {  // (a window's counts add up in 32 bits)
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    const size_t words = (size_t)((n + 31) / 32);
    std::mt19937 gen(11);
    auto unit = [&]() { return (float)(gen() >> 8) / 16777216.0f; };
    // x uniform in [-4, 4]; y = 1 (every value in one bin); alpha uniform, red constant; a covariance with three distinct scales, turned
    std::vector<uint4> h_pc(n), h_cov_a(n);
    std::vector<uint2> h_cov_b(n), h_cov_h(n);
    std::vector<uint32_t> h_cov_h2(n), h_sel(words);
    for (uint64_t i = 0; i < n; ++i) {
        const float x = 8.0f * unit() - 4.0f, y = 1.0f, z = unit();
        const uint32_t color = 0x40u | ((gen() & 0xFFFFu) << 8) | ((gen() & 0xFFu) << 24);
        memcpy(&h_pc[i].x, &x, 4);
        memcpy(&h_pc[i].y, &y, 4);
        memcpy(&h_pc[i].z, &z, 4);
        h_pc[i].w = color;
        const float a = 0.01f + 0.1f * unit(), b = 0.01f + 0.05f * unit(), c = 0.011f + 0.01f * unit(), t = 6.2831853f * unit();
        const float cs = cosf(t), sn = sinf(t);  // a turn about z: S = R diag(a^2, b^2, c^2) R^T
        const float cov[6] = {cs * cs * a * a + sn * sn * b * b, cs * sn * (a * a - b * b), 0.0f, sn * sn * a * a + cs * cs * b * b, 0.0f, c * c};
        memcpy(&h_cov_a[i], cov, 16);
        memcpy(&h_cov_b[i], cov + 4, 8);
        const float pos[6] = {cov[0], fabsf(cov[1]) + 1e-4f, 1e-4f, cov[3], 1e-4f, cov[5]};  // (strictly positive for half_bits)
        h_cov_h[i] = make_uint2(half_bits(pos[0]) | ((uint32_t)half_bits(pos[1]) << 16), half_bits(pos[2]) | ((uint32_t)half_bits(pos[3]) << 16));
        h_cov_h2[i] = half_bits(pos[4]) | ((uint32_t)half_bits(pos[5]) << 16);
    }
    for (auto& w : h_sel) w = gen();
    ExtractPlanes src{};
    uint32_t *sel, *ws;
    float* values;
    CK(hipMalloc(&src.pc, 16 * n));
    CK(hipMalloc(&src.cov_a, 16 * n));
    CK(hipMalloc(&src.cov_b, 8 * n));
    CK(hipMalloc(&src.cov_h, 8 * n));
    CK(hipMalloc(&src.cov_h2, 4 * n));
    CK(hipMalloc(&sel, 4 * words));
    CK(hipMalloc(&values, 4 * n));
    CK(hipMalloc(&ws, 4 * (kPropResultWords + kPropMaxBins + kPropPartialWords * kPropMaxGroups)));
    CK(hipMemcpy(src.pc, h_pc.data(), 16 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(src.cov_a, h_cov_a.data(), 16 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(src.cov_b, h_cov_b.data(), 8 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(src.cov_h, h_cov_h.data(), 8 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(src.cov_h2, h_cov_h2.data(), 4 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(sel, h_sel.data(), 4 * words, hipMemcpyHostToDevice));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const ModelFilter none{};

    struct Row {
        std::string name;
        uint32_t mode, property, bins;
        float lo, hi;
        int cov_kind;
        double bytes;
    };
    std::vector<Row> rows;
    const double pc_bytes = 16.0 * (double)n, word_bytes = 4.0 * (double)words;
    const struct { const char* name; int cov; uint32_t property; double bytes; float lo, hi; } cls[3] = {
        {"pc", GSX_COV3D_SINGLE, GSX_PROP_POS_X, pc_bytes, -4.0f, 4.0f},
        {"cov_single", GSX_COV3D_SINGLE, GSX_PROP_SCALE_MAX, 24.0 * (double)n, 0.0f, 0.12f},
        {"cov_half", GSX_COV3D_HALF, GSX_PROP_SCALE_MAX, 12.0 * (double)n, 0.0f, 0.12f}};
    for (const auto& c : cls) {
        rows.push_back({std::string(c.name) + "/values", kPropValues, c.property, 0, 0, 0, c.cov, c.bytes + 4.0 * (double)n});
        rows.push_back({std::string(c.name) + "/reduce", kPropReduce, c.property, 0, 0, 0, c.cov, c.bytes});
        rows.push_back({std::string(c.name) + "/hist256", kPropHist, c.property, 256, c.lo, c.hi, c.cov, c.bytes});
        rows.push_back({std::string(c.name) + "/hist4096", kPropHist, c.property, 4096, c.lo, c.hi, c.cov, c.bytes});
        rows.push_back({std::string(c.name) + "/select", kPropSelect, c.property, 0, c.lo * 0.5f, c.hi * 0.5f, c.cov, c.bytes + 2.0 * word_bytes});
    }
    // every value in one bin: y = 1 in [0, 2], red = 0x40 / 255 in [0, 1]; opacity uniform over 256 values
    rows.push_back({"pc/hist256_one_bin", kPropHist, GSX_PROP_POS_Y, 256, 0.0f, 2.0f, GSX_COV3D_SINGLE, pc_bytes});
    rows.push_back({"pc/hist4096_one_bin", kPropHist, GSX_PROP_POS_Y, 4096, 0.0f, 2.0f, GSX_COV3D_SINGLE, pc_bytes});
    rows.push_back({"pc/hist256_red_one_bin", kPropHist, GSX_PROP_RED, 256, 0.0f, 1.0f, GSX_COV3D_SINGLE, pc_bytes});
    rows.push_back({"pc/hist256_opacity", kPropHist, GSX_PROP_OPACITY, 256, 0.0f, 1.0f, GSX_COV3D_SINGLE, pc_bytes});
    rows.push_back({"pc/hist16_opacity", kPropHist, GSX_PROP_OPACITY, 16, 0.0f, 1.0f, GSX_COV3D_SINGLE, pc_bytes});
    rows.push_back({"pc/hist256_hue", kPropHist, GSX_PROP_HUE, 256, 0.0f, 1.0f, GSX_COV3D_SINGLE, pc_bytes});

    auto launch = [&](const Row& r) {
        PropertyJob job{};
        job.property = r.property;
        job.lo = r.lo;
        job.hi = r.hi;
        job.bins = r.bins;
        job.values = values;
        job.result = ws;
        job.hist = ws + kPropResultWords;
        job.partials = ws + kPropResultWords + kPropMaxBins;
        job.sel = SelectionWrite{GSX_SELECTION_SET, 1u, sel, job.partials};
        CK(launch_property(s, r.mode, r.cov_kind, n, none, src, job));
    };
    printf("{\"tool\": \"bench_property_kernels\", \"n\": %llu, \"samples\": %d, \"reps\": %d, \"rows\": {", (unsigned long long)n, samples, reps);
    bool first = true;
    for (const Row& r : rows) {
        CK(launch_property_reset(s, ws, ws + kPropResultWords, kPropMaxBins));
        launch(r);  // warm-up
        launch(r);
        CK(hipStreamSynchronize(s));
        std::vector<double> ms;
        for (int k = 0; k < samples; ++k) {
            CK(launch_property_reset(s, ws, ws + kPropResultWords, kPropMaxBins));  // (outside the window: a window's counts add up)
            CK(hipEventRecord(e0, s));
            for (int j = 0; j < reps; ++j) launch(r);
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            float t = 0.0f;
            CK(hipEventElapsedTime(&t, e0, e1));
            ms.push_back((double)t / reps);
        }
        uint32_t h_res[kPropResultWords];
        CK(hipMemcpy(h_res, ws, sizeof h_res, hipMemcpyDeviceToHost));
        const double med = median(ms);
        printf("%s\"%s\": {\"ms\": %.5f, \"ms_all\": [", first ? "" : ", ", r.name.c_str(), med);
        for (int k = 0; k < samples; ++k) printf("%s%.5f", k ? ", " : "", ms[k]);
        printf("], \"bytes\": %.0f, \"TBps\": %.3f, \"count\": %u}", r.bytes, r.bytes / (med * 1e-3) / 1e12,
               r.mode == kPropSelect ? h_res[kPropHit] : (r.mode == kPropReduce ? h_res[kPropAutoCount] : h_res[kPropCount]));
        first = false;
    }
    printf("}}\n");
    return 0;
}
