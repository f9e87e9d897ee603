// tools/bench_import.hip — the row kernel of gsx_model_import_ply (csrc/kernels_import.hip) alone, reading canonical PLY rows from
// device memory: one launch over a whole model of n Gaussians, timed with HIP events, for each read side (the LDS slab, the per-lane
// direct read, and the general kernel on the same canonical rows), beside k_convert (csrc/kernels_project.hip) over the same count
// of gsx_gaussian records.  The kernel files are included as source; nothing of libgsx is linked.  Not part of the product;
// tools/bench_import.py builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_import.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_import_kernels
//   tools/bench_import_kernels <n> <sh kind 0..3> <cov3d kind 0..1> [reps=10]
// The rows hold 4096 different rows (uniform positions, f_dc, f_rest, opacity in [-9, 9], log-scales in [-9, 2], normal quaternions),
// repeated.  The variants are timed alternately, `reps` rounds after two warm-up rounds; per variant: the median microseconds per
// launch, the smallest and largest, and the algorithmic bytes per second: 248 B (or the 224 B record for k_convert) read plus the
// resident bytes written per Gaussian of the pod kind, shade record included.  Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_import.hip"

using namespace gsx;
#define CK(x)                                                       \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) {                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            exit(1);                                                \
        }                                                           \
    } while (0)

// k_convert (csrc/kernels_project.hip), restated: its body is store_gaussian, which this file shares with it through pod_store.h
__global__ __launch_bounds__(256) void k_bench_convert(const gsx_gaussian* __restrict__ src, uint64_t n, uint64_t start, uint64_t model_n, PodPlanes pod) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    store_gaussian(pod, model_n, start + t, src[t]);
}

constexpr uint32_t kTable = 4096;

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
    PodPlanes pod{};
    pod.sh_kind = sh;
    pod.cov_kind = cov;
    aos_layout(sh, cov, &pod.aos_stride, &pod.aos_geo);
    size_t per_gaussian = 0;
    auto plane = [&](auto** slot, size_t bytes_per_gaussian) {
        CK(hipMalloc(reinterpret_cast<void**>(slot), bytes_per_gaussian * n));
        per_gaussian += bytes_per_gaussian;
    };
    plane(&pod.pc, 16);
    if (cov == GSX_COV3D_SINGLE) {
        plane(&pod.cov_a, 16);
        plane(&pod.cov_b, 8);
    } else {
        plane(&pod.cov_h, 8);
        plane(&pod.cov_h2, 4);
    }
    if (sh == GSX_SH_SINGLE) {
        plane(&pod.sh4, 16 * (size_t)kShPlanes4);
        plane(&pod.sh1, 4);
    } else if (sh == GSX_SH_HALF) {
        plane(&pod.sh_h, 16 * 6);
    } else if (sh == GSX_SH_NORM8) {
        plane(&pod.sh_q, 16 * 3);
    }
    if (pod.aos_stride) plane(&pod.sh_aos, 16 * (size_t)pod.aos_stride);

    // the rows, and the records the host reader's arithmetic makes of them (what k_convert would be given)
    std::mt19937 rng(7);
    std::normal_distribution<float> gauss;
    std::uniform_real_distribution<float> pos(-5.0f, 5.0f), fdc(-2.0f, 2.0f), op(-9.0f, 9.0f), logs(-9.0f, 2.0f);
    std::vector<float> table(62 * (size_t)kTable);
    std::vector<gsx_gaussian> recs(kTable);
    for (uint32_t k = 0; k < kTable; ++k) {
        float* v = &table[62 * (size_t)k];
        for (int j = 0; j < 3; ++j) v[IMP_X + j] = pos(rng);
        for (int j = 3; j < 6; ++j) v[j] = 0.0f;
        for (int j = 0; j < 3; ++j) v[IMP_FDC + j] = fdc(rng);
        for (int j = 0; j < 45; ++j) v[IMP_REST + j] = 0.3f * gauss(rng);
        v[IMP_OPACITY] = op(rng);
        for (int j = 0; j < 3; ++j) v[IMP_SCALE + j] = logs(rng);
        for (int j = 0; j < 4; ++j) v[IMP_ROT + j] = gauss(rng);
        im_row_to_gaussian(v, &recs[k]);
    }
    std::vector<float> h_rows(62 * n);
    std::vector<gsx_gaussian> h_recs(n);
    for (uint64_t i = 0; i < n; ++i) {
        memcpy(&h_rows[62 * i], &table[62 * (i % kTable)], 248);
        h_recs[i] = recs[i % kTable];
    }
    void *d_rows, *d_recs;
    CK(hipMalloc(&d_rows, 248 * n));
    CK(hipMalloc(&d_recs, sizeof(gsx_gaussian) * n));
    CK(hipMemcpy(d_rows, h_rows.data(), 248 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_recs, h_recs.data(), sizeof(gsx_gaussian) * n, hipMemcpyHostToDevice));

    gsx_ply_header h{};
    h.vertex_bytes = 248;
    for (int k = 0; k < 62; ++k) h.offsets[k] = 4 * k;
    const ImportLayout lay = im_layout(h);
    const char* names[4] = {"slab", "direct", "general", "k_convert"};
    const int reads[3] = {kImportSlab, kImportDirect, kImportGeneral};
    std::vector<double> us[4];
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int r = 0; r < reps + 2; ++r)
        for (int k = 0; k < 4; ++k) {  // (alternating: what drifts on the machine drifts for all four)
            CK(hipEventRecord(a, 0));
            if (k < 3) {
                CK(launch_import_rows(0, d_rows, n, 0, n, pod, lay, reads[k]));
            } else {
                k_bench_convert<<<dim3((uint32_t)((n + 255) / 256)), dim3(256)>>>(static_cast<const gsx_gaussian*>(d_recs), n, 0, n, pod);
                CK(hipGetLastError());
            }
            CK(hipEventRecord(b, 0));
            CK(hipEventSynchronize(b));
            float ms = 0.0f;
            CK(hipEventElapsedTime(&ms, a, b));
            if (r >= 2) us[k].push_back(1e3 * ms);
        }
    std::string json = "{\"tool\": \"bench_import_kernels\", \"n\": " + std::to_string(n) + ", \"sh\": " + std::to_string(sh) + ", \"cov3d\": " + std::to_string(cov) +
                       ", \"resident_bytes_per_gaussian\": " + std::to_string(per_gaussian) + ", \"reps\": " + std::to_string(reps);
    for (int k = 0; k < 4; ++k) {
        std::sort(us[k].begin(), us[k].end());
        const double med = us[k].size() % 2 ? us[k][us[k].size() / 2] : 0.5 * (us[k][us[k].size() / 2 - 1] + us[k][us[k].size() / 2]);
        const double bytes = ((double)per_gaussian + (k < 3 ? 248.0 : 224.0)) * (double)n;
        char row[512];
        snprintf(row, sizeof row, ", \"%s\": {\"us\": %.2f, \"us_min\": %.2f, \"us_max\": %.2f, \"bytes\": %.0f, \"TBps\": %.4f}", names[k], med, us[k].front(),
                 us[k].back(), bytes, bytes / med * 1e-6);
        json += row;
    }
    json += "}";
    printf("%s\n", json.c_str());
    return 0;
}
