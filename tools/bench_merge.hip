// tools/bench_merge.hip — the kernels of gsx_model_merge (csrc/kernels_extract.hip, csrc/kernels_merge.hip) on four sources of n / 4
// Gaussians each that keep everything, merged into one model of n, each stage timed with HIP events around its four launches.  The
// kernel files are included as source; nothing of libgsx is linked.  Not part of the product; tools/bench_merge.py builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_merge.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_merge_kernels
//   tools/bench_merge_kernels <n> <sh kind 0..3> <cov3d kind 0..1> [reps=10]
// The source planes hold small finite values (the bake computes with them); the destination offsets are the sources' counts, so
// three of the four are no multiple of 32 when n / 4 is not.  Per stage: microseconds for the four launches (median of `reps` after
// two warm-ups).  `identity`: k_extract_scatter with a destination offset; `extract_whole`: the same kernel on ONE source of n
// Gaussians (what tools/bench_extract_kernels times as pattern `all`), for the same bytes; `baked`: k_merge_bake.  Bytes moved:
// identity reads and writes every carried plane, shade records included; the bake reads the SoA planes and writes the SoA planes
// and the shade records.  `memcpy`: the runtime's device-to-device copy of one model's planes.  Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_extract.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_merge.hip"

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
    size_t offset;  // of the pointer inside ExtractPlanes
    size_t bytes_per_gaussian;
    bool aos;
};

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <n> <sh kind> <cov3d kind> [reps]\n", argv[0]);
        return 2;
    }
    const uint64_t n = strtoull(argv[1], nullptr, 10);
    const int sh = atoi(argv[2]), cov = atoi(argv[3]), reps = argc > 4 ? atoi(argv[4]) : 10;
    constexpr int kSources = 4;
    if (n < kSources || n >= 0xFFFFFFF0ull || sh < 0 || sh > GSX_SH_NONE || cov < 0 || cov > GSX_COV3D_HALF || reps < 1) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    uint32_t stride = 0, geo = 0;
    aos_layout(sh, cov, &stride, &geo);
    std::vector<Plane> planes;
    planes.push_back({offsetof(ExtractPlanes, pc), 16, false});
    if (cov == GSX_COV3D_SINGLE) {
        planes.push_back({offsetof(ExtractPlanes, cov_a), 16, false});
        planes.push_back({offsetof(ExtractPlanes, cov_b), 8, false});
    } else {
        planes.push_back({offsetof(ExtractPlanes, cov_h), 8, false});
        planes.push_back({offsetof(ExtractPlanes, cov_h2), 4, false});
    }
    if (sh == GSX_SH_SINGLE) {
        planes.push_back({offsetof(ExtractPlanes, sh4), 16 * (size_t)kShPlanes4, false});
        planes.push_back({offsetof(ExtractPlanes, sh1), 4, false});
    } else if (sh == GSX_SH_HALF) {
        planes.push_back({offsetof(ExtractPlanes, sh_h), 16 * 6, false});
    } else if (sh == GSX_SH_NORM8) {
        planes.push_back({offsetof(ExtractPlanes, sh_q), 16 * 3, false});
    }
    if (stride) planes.push_back({offsetof(ExtractPlanes, sh_aos), 16 * (size_t)stride, true});
    size_t per_gaussian = 0, per_gaussian_soa = 0;
    for (const Plane& p : planes) {
        per_gaussian += p.bytes_per_gaussian;
        if (!p.aos) per_gaussian_soa += p.bytes_per_gaussian;
    }
    auto alloc = [&](ExtractPlanes& e, uint64_t count, bool fill) {
        for (const Plane& p : planes) {
            void* d = nullptr;
            CK(hipMalloc(&d, p.bytes_per_gaussian * count));
            // 0x3C3C3C3C is the float 0.0115, 0x3C3C the half 1.06, 0x3C the snorm8 0.47: finite whatever the kind reads them as
            CK(hipMemset(d, fill ? 0x3C : 0, p.bytes_per_gaussian * count));
            memcpy(reinterpret_cast<char*>(&e) + p.offset, &d, sizeof d);
        }
    };
    uint64_t counts[kSources], offs[kSources];
    ExtractPlanes src[kSources], whole{}, dst{};
    uint32_t *keep[kSources], *partials[kSources], *bases[kSources], *keep_w, *partials_w, *bases_w;
    uint64_t* totals;
    CK(hipMalloc(&totals, 8 * (kSources + 1)));
    uint64_t at = 0;
    for (int s = 0; s < kSources; ++s) {
        counts[s] = s + 1 < kSources ? n / kSources : n - at;
        offs[s] = at;
        at += counts[s];
        src[s] = ExtractPlanes{};
        alloc(src[s], counts[s], true);
        CK(hipMalloc(&keep[s], 4 * ((counts[s] + 31) / 32)));
        CK(hipMalloc(&partials[s], 4 * extract_groups(counts[s])));
        CK(hipMalloc(&bases[s], 4 * extract_groups(counts[s])));
    }
    alloc(whole, n, true);
    alloc(dst, n, false);
    CK(hipMalloc(&keep_w, 4 * ((n + 31) / 32)));
    CK(hipMalloc(&partials_w, 4 * extract_groups(n)));
    CK(hipMalloc(&bases_w, 4 * extract_groups(n)));

    ModelFilter f{};  // no mask: all pass
    const double keep_us = time_us(reps, [&] {
        for (int s = 0; s < kSources; ++s) CK(launch_extract_keep(0, counts[s], f, keep[s], partials[s]));
    });
    const double scan_us = time_us(reps, [&] {
        for (int s = 0; s < kSources; ++s) CK(launch_extract_scan(0, partials[s], extract_groups(counts[s]), bases[s], totals + s));
    });
    CK(launch_extract_keep(0, n, f, keep_w, partials_w));
    CK(launch_extract_scan(0, partials_w, extract_groups(n), bases_w, totals + kSources));
    uint64_t h_totals[kSources + 1];
    CK(hipMemcpy(h_totals, totals, sizeof h_totals, hipMemcpyDeviceToHost));
    for (int s = 0; s < kSources; ++s)
        if (h_totals[s] != counts[s] || h_totals[kSources] != n) {
            fprintf(stderr, "source %d: the scan counted %llu of %llu\n", s, (unsigned long long)h_totals[s], (unsigned long long)counts[s]);
            return 1;
        }
    const double identity_us = time_us(reps, [&] {
        for (int s = 0; s < kSources; ++s) CK(launch_extract_scatter(0, sh, cov, counts[s], n, offs[s], keep[s], bases[s], src[s], dst));
    });
    const double whole_us = time_us(reps, [&] { CK(launch_extract_scatter(0, sh, cov, n, n, 0, keep_w, bases_w, whole, dst)); });
    MergeBake b{};
    const float q[4] = {0.18257418f, 0.36514837f, 0.54772256f, 0.73029674f};
    const float R[9] = {0.13333333f, -0.66666667f, 0.73333333f, 0.93333333f, 0.33333333f, 0.13333333f, -0.33333333f, 0.66666667f, 0.66666667f};
    memcpy(b.R, R, sizeof R);
    b.s[0] = 1.3f, b.s[1] = -0.7f, b.s[2] = 0.9f;
    b.t[0] = 0.3f, b.t[1] = -0.2f, b.t[2] = 0.5f;
    merge_sh_matrices(q, b.sh);
    const double baked_us = time_us(reps, [&] {
        for (int s = 0; s < kSources; ++s) CK(launch_merge_bake(0, sh, cov, counts[s], n, offs[s], keep[s], bases[s], src[s], dst, b));
    });
    const double memcpy_us = time_us(reps, [&] {
        for (const Plane& p : planes) {
            void *d, *s;
            memcpy(&d, reinterpret_cast<char*>(&dst) + p.offset, sizeof d);
            memcpy(&s, reinterpret_cast<char*>(&whole) + p.offset, sizeof s);
            CK(hipMemcpyAsync(d, s, p.bytes_per_gaussian * n, hipMemcpyDeviceToDevice, 0));
        }
    });
    const double copy_bytes = 2.0 * (double)per_gaussian * (double)n, bake_bytes = (double)(per_gaussian_soa + per_gaussian) * (double)n;
    printf("{\"tool\": \"bench_merge_kernels\", \"n\": %llu, \"sources\": %d, \"sh\": %d, \"cov3d\": %d, \"bytes_per_gaussian\": %zu, \"bytes_per_gaussian_soa\": %zu, "
           "\"reps\": %d, \"keep_us\": %.2f, \"scan_us\": %.2f, \"identity_us\": %.2f, \"identity_TBps\": %.4f, \"extract_whole_us\": %.2f, "
           "\"extract_whole_TBps\": %.4f, \"baked_us\": %.2f, \"baked_bytes\": %.0f, \"baked_TBps\": %.4f, \"memcpy\": {\"us\": %.2f, \"TBps\": %.4f}}\n",
           (unsigned long long)n, kSources, sh, cov, per_gaussian, per_gaussian_soa, reps, keep_us, scan_us, identity_us, copy_bytes / identity_us * 1e-6, whole_us,
           copy_bytes / whole_us * 1e-6, baked_us, bake_bytes, bake_bytes / baked_us * 1e-6, memcpy_us, copy_bytes / memcpy_us * 1e-6);
    return 0;
}
