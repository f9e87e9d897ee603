// tools/bench_export.hip — the row kernel of gsx_model_export (csrc/kernels_export.hip) alone, writing into device memory: one launch
// over a whole model of n Gaussians, timed with HIP events, for two keep patterns (`all`, and `p03`: 3 in 100 at random) and both row
// formats.  The kernel files are included as source; nothing of libgsx is linked.  Not part of the product; tools/bench_export.py
// builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_export.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_export_kernels
//   tools/bench_export_kernels <n> <sh kind 0..3> <cov3d kind 0..1> [reps=10]
// The covariance planes hold 4096 different covariances of random rotations and log-uniform scales (e^-6 .. e^0), repeated, so the
// eigen-solve does what it does on a scene (a constant fill would make every lane skip the same rotations); the other planes hold
// a finite byte pattern.  Per pattern and format: the kept count, microseconds per launch (median of `reps` after two warm-ups) and
// the algorithmic bytes per second: the SoA planes of the kept Gaussians read plus their rows written.  Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_extract.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_export.hip"

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

constexpr uint32_t kTable = 4096;

// Gaussian i takes covariance i % kTable of the table (6 floats each), in the model's covariance kind
__global__ void k_fill_cov(uint64_t n, const float* __restrict__ table, int cov_kind, ExtractPlanes p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = table + 6 * (i % kTable);
    if (cov_kind == GSX_COV3D_SINGLE) {
        p.cov_a[i] = make_uint4(__float_as_uint(c[0]), __float_as_uint(c[1]), __float_as_uint(c[2]), __float_as_uint(c[3]));
        p.cov_b[i] = make_uint2(__float_as_uint(c[4]), __float_as_uint(c[5]));
    } else {
        p.cov_h[i] = make_uint2(pack_h2(c[0], c[1]), pack_h2(c[2], c[3]));
        p.cov_h2[i] = pack_h2(c[4], c[5]);
    }
}

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
    ExtractPlanes src{};
    size_t per_gaussian = 0;
    auto plane = [&](auto** slot, size_t bytes_per_gaussian) {
        CK(hipMalloc(reinterpret_cast<void**>(slot), bytes_per_gaussian * n));
        // 0x3C3C3C3C is the float 0.0115, 0x3C3C the half 1.06, 0x3C the snorm8 0.47: finite whatever the kind reads them as
        CK(hipMemset(*slot, 0x3C, bytes_per_gaussian * n));
        per_gaussian += bytes_per_gaussian;
    };
    plane(&src.pc, 16);
    if (cov == GSX_COV3D_SINGLE) {
        plane(&src.cov_a, 16);
        plane(&src.cov_b, 8);
    } else {
        plane(&src.cov_h, 8);
        plane(&src.cov_h2, 4);
    }
    if (sh == GSX_SH_SINGLE) {
        plane(&src.sh4, 16 * (size_t)kShPlanes4);
        plane(&src.sh1, 4);
    } else if (sh == GSX_SH_HALF) {
        plane(&src.sh_h, 16 * 6);
    } else if (sh == GSX_SH_NORM8) {
        plane(&src.sh_q, 16 * 3);
    }
    // the covariance table: S = R diag(s^2) R^T
    std::mt19937 rng(7);
    std::normal_distribution<float> gauss;
    std::uniform_real_distribution<float> logs(-6.0f, 0.0f);
    std::vector<float> table(6 * kTable);
    for (uint32_t k = 0; k < kTable; ++k) {
        float q[4], len = 0.0f, s2[3];
        for (float& c : q) {
            c = gauss(rng);
            len += c * c;
        }
        for (float& c : q) c /= std::sqrt(len);
        for (float& s : s2) {
            const float e = std::exp(logs(rng));
            s = e * e;
        }
        const float x = q[0], y = q[1], z = q[2], w = q[3];
        const float R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                            2 * (y * z - w * x),     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
        const int idx[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
        for (int e = 0; e < 6; ++e) {
            float acc = 0.0f;
            for (int j = 0; j < 3; ++j) acc += R[idx[e][0] * 3 + j] * s2[j] * R[idx[e][1] * 3 + j];
            table[6 * k + e] = acc;
        }
    }
    float* d_table;
    CK(hipMalloc(&d_table, 4 * table.size()));
    CK(hipMemcpy(d_table, table.data(), 4 * table.size(), hipMemcpyHostToDevice));
    k_fill_cov<<<dim3((uint32_t)((n + 255) / 256)), dim3(256)>>>(n, d_table, cov, src);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());

    const uint64_t words = (n + 31) / 32, groups = extract_groups(n);
    uint32_t *mask, *keep, *partials, *bases;
    uint64_t* total;
    void* rows;
    CK(hipMalloc(&mask, 4 * words));
    CK(hipMalloc(&keep, 4 * words));
    CK(hipMalloc(&partials, 4 * groups));
    CK(hipMalloc(&bases, 4 * groups));
    CK(hipMalloc(&total, 8));
    CK(hipMalloc(&rows, 248 * n));

    std::string json = "{\"tool\": \"bench_export_kernels\", \"n\": " + std::to_string(n) + ", \"sh\": " + std::to_string(sh) + ", \"cov3d\": " + std::to_string(cov) +
                       ", \"pod_bytes_per_gaussian\": " + std::to_string(per_gaussian) + ", \"reps\": " + std::to_string(reps);
    const char* names[2] = {"all", "p03"};
    std::vector<uint32_t> h_mask(words);
    for (int pat = 0; pat < 2; ++pat) {
        std::mt19937 mrng(103);  // (bench_extract's seed for its p03 pattern)
        for (uint64_t w = 0; w < words; ++w) {
            uint32_t word = 0;
            for (uint32_t b = 0; b < 32u; ++b)
                if (pat == 0 || mrng() % 100u < 3u) word |= 1u << b;
            h_mask[w] = word;
        }
        CK(hipMemcpy(mask, h_mask.data(), 4 * words, hipMemcpyHostToDevice));
        ModelFilter f{};
        f.mask = mask;
        CK(launch_extract_keep(0, n, f, keep, partials));
        CK(launch_extract_scan(0, partials, groups, bases, total));
        uint64_t count = 0;
        CK(hipMemcpy(&count, total, 8, hipMemcpyDeviceToHost));
        for (uint32_t format = 0; format < 2u; ++format) {
            const double row_bytes = format == GSX_EXPORT_GAUSSIANS ? 224.0 : 248.0;
            const double us = time_us(reps, [&] { CK(launch_export_rows(0, sh, cov, format, n, 0, (uint32_t)groups, 0, keep, bases, src, rows)); });
            const double bytes = ((double)per_gaussian + row_bytes) * (double)count;
            char row[512];
            snprintf(row, sizeof row, ", \"%s_%s\": {\"kept\": %llu, \"rows_us\": %.2f, \"bytes\": %.0f, \"TBps\": %.4f}", names[pat],
                     format == GSX_EXPORT_GAUSSIANS ? "gaussians" : "ply", (unsigned long long)count, us, bytes, bytes / us * 1e-6);
            json += row;
        }
    }
    json += "}";
    printf("%s\n", json.c_str());
    return 0;
}
