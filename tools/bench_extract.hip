// tools/bench_extract.hip — the three kernels of gsx_model_extract (csrc/kernels_extract.hip) on a model-sized set of planes, each
// timed with HIP events around its launches, for four keep patterns.  The kernel file is included as source; nothing of libgsx is
// linked.  Not part of the product; tools/bench_extract.py builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_extract.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_extract_kernels
//   tools/bench_extract_kernels <n> <sh kind 0..3> <cov3d kind 0..1> [reps=10]
// The planes hold a seeded byte pattern (a copy does not care what it moves); the mask decides what is kept:
//   all          every Gaussian: a plain copy
//   first_half   [0, n / 2): contiguous
//   p50, p03     each Gaussian with probability 0.5 / 0.03, seeded
// Per pattern: the kept count, microseconds per launch of keep / scan / scatter (median of `reps` after two warm-up launches), and
// the scatter's algorithmic bytes per second: kept rows read plus kept rows written over every carried plane (no edit planes here).
// `memcpy`: hipMemcpyAsync device to device of one model's planes (the bytes of pattern `all`), the runtime's own copy, beside it.
// Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_extract.hip"

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

template <class F>
static double time_us(int reps, F&& launch) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::vector<double> us;
    for (int r = 0; r < reps + 2; ++r) {
        CK(hipEventRecord(a, 0));
        launch();
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        float ms = 0.0f;
        CK(hipEventElapsedTime(&ms, a, b));
        if (r >= 2) us.push_back(1e3 * ms);
    }
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    return median(us);
}

struct Plane {
    void** slot;
    size_t bytes_per_gaussian;
};

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <n> <sh kind> <cov3d kind> [reps]\n", argv[0]);
        return 2;
    }
    const uint64_t n = strtoull(argv[1], nullptr, 10);
    const int sh = atoi(argv[2]), cov = atoi(argv[3]), reps = argc > 4 ? atoi(argv[4]) : 10;
    if (n == 0 || n >= 0xFFFFFFF0ull || sh < 0 || sh > GSX_SH_NONE || cov < 0 || cov > GSX_COV3D_HALF || reps < 1) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    uint32_t stride = 0, geo = 0;
    aos_layout(sh, cov, &stride, &geo);
    ExtractPlanes src{}, dst{};
    auto planes_of = [&](ExtractPlanes& p) {
        std::vector<Plane> v;
        v.push_back({(void**)&p.pc, 16});
        if (cov == GSX_COV3D_SINGLE) {
            v.push_back({(void**)&p.cov_a, 16});
            v.push_back({(void**)&p.cov_b, 8});
        } else {
            v.push_back({(void**)&p.cov_h, 8});
            v.push_back({(void**)&p.cov_h2, 4});
        }
        if (sh == GSX_SH_SINGLE) {
            v.push_back({(void**)&p.sh4, 16 * (size_t)kShPlanes4});
            v.push_back({(void**)&p.sh1, 4});
        } else if (sh == GSX_SH_HALF) {
            v.push_back({(void**)&p.sh_h, 16 * 6});
        } else if (sh == GSX_SH_NORM8) {
            v.push_back({(void**)&p.sh_q, 16 * 3});
        }
        if (stride) v.push_back({(void**)&p.sh_aos, 16 * (size_t)stride});
        return v;
    };
    size_t per_gaussian = 0;
    const std::vector<Plane> sp = planes_of(src), dp = planes_of(dst);
    for (size_t k = 0; k < sp.size(); ++k) {
        CK(hipMalloc(sp[k].slot, sp[k].bytes_per_gaussian * n));
        CK(hipMalloc(dp[k].slot, dp[k].bytes_per_gaussian * n));
        CK(hipMemset(*sp[k].slot, 0x5A + (int)k, sp[k].bytes_per_gaussian * n));
        CK(hipMemset(*dp[k].slot, 0, dp[k].bytes_per_gaussian * n));
        per_gaussian += sp[k].bytes_per_gaussian;
    }
    const uint64_t words = (n + 31) / 32, groups = extract_groups(n);
    uint32_t *mask, *keep, *partials, *bases;
    uint64_t* total;
    CK(hipMalloc(&mask, 4 * words));
    CK(hipMalloc(&keep, 4 * words));
    CK(hipMalloc(&partials, 4 * groups));
    CK(hipMalloc(&bases, 4 * groups));
    CK(hipMalloc(&total, 8));

    std::string json = "{\"tool\": \"bench_extract_kernels\", \"n\": " + std::to_string(n) + ", \"sh\": " + std::to_string(sh) + ", \"cov3d\": " + std::to_string(cov) +
                       ", \"bytes_per_gaussian\": " + std::to_string(per_gaussian) + ", \"reps\": " + std::to_string(reps);
    const char* names[4] = {"all", "first_half", "p50", "p03"};
    std::vector<uint32_t> h_mask(words);
    for (int pat = 0; pat < 4; ++pat) {
        std::mt19937 rng(100 + pat);
        uint64_t want = 0;
        for (uint64_t w = 0; w < words; ++w) {
            uint32_t word = 0;
            for (uint32_t b = 0; b < 32u; ++b) {
                const uint64_t i = w * 32u + b;
                const bool on = pat == 0 || (pat == 1 && i < n / 2) || (pat == 2 && (rng() & 1u)) || (pat == 3 && rng() % 100u < 3u);
                if (on) word |= 1u << b;
                if (on && i < n) ++want;
            }
            h_mask[w] = word;  // (pattern `all` leaves bits above n set: the kernel clears them)
        }
        CK(hipMemcpy(mask, h_mask.data(), 4 * words, hipMemcpyHostToDevice));
        ModelFilter f{};
        f.mask = mask;
        const double keep_us = time_us(reps, [&] { CK(launch_extract_keep(0, n, f, keep, partials)); });
        const double scan_us = time_us(reps, [&] { CK(launch_extract_scan(0, partials, groups, bases, total)); });
        uint64_t count = 0;
        CK(hipMemcpy(&count, total, 8, hipMemcpyDeviceToHost));
        if (count != want) {
            fprintf(stderr, "pattern %s: the scan counted %llu, the host %llu\n", names[pat], (unsigned long long)count, (unsigned long long)want);
            return 1;
        }
        const double scatter_us = time_us(reps, [&] { CK(launch_extract_scatter(0, sh, cov, n, count, 0, keep, bases, src, dst)); });
        const double bytes = 2.0 * (double)per_gaussian * (double)count;
        char row[512];
        snprintf(row, sizeof row, ", \"%s\": {\"kept\": %llu, \"keep_us\": %.2f, \"scan_us\": %.2f, \"scatter_us\": %.2f, \"scatter_bytes\": %.0f, \"scatter_TBps\": %.4f}",
                 names[pat], (unsigned long long)count, keep_us, scan_us, scatter_us, bytes, bytes / scatter_us * 1e-6);
        json += row;
    }
    const double memcpy_us = time_us(reps, [&] {
        for (size_t k = 0; k < sp.size(); ++k) CK(hipMemcpyAsync(*dp[k].slot, *sp[k].slot, sp[k].bytes_per_gaussian * n, hipMemcpyDeviceToDevice, 0));
    });
    char row[256];
    snprintf(row, sizeof row, ", \"memcpy\": {\"us\": %.2f, \"TBps\": %.4f}}", memcpy_us, 2.0 * (double)per_gaussian * (double)n / memcpy_us * 1e-6);
    json += row;
    printf("%s\n", json.c_str());
    return 0;
}
