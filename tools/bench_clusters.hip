// tools/bench_clusters.hip — the passes of the model clusters (csrc/kernels_clusters.hip on the grid of csrc/kernels_neighbors.hip) on
// a file of position + colour elements, each timed with HIP events.  The kernel files are included as source; nothing of libgsx is
// linked.  Not part of the product; tools/bench_clusters.py builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_clusters.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_clusters_kernels
//   tools/bench_clusters_kernels <pc file: n x 16 bytes> <n> <samples> <radius>:<grid_bits (0: the library's)> ...
// Per job the passes run in their order, an event between every two: reset (the memsets and the seeds: one Gaussian in 1024
// selected), reduce, cell, scan, scatter, then query — gsx_model_neighbors' query with max_count 4095, which walks the same pairs as
// the hook: the yardstick — then init, hook, label, stats and the select in its three modes.  ms per pass: the median of `samples` runs
// after one warm-up, every sample listed.  Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_extract.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_neighbors.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_clusters.hip"

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

int main(int argc, char** argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s <pc file> <n> <samples> <radius>:<grid_bits> ...\n", argv[0]);
        return 2;
    }
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    const int samples = atoi(argv[3]);
    if (n == 0 || n > 0xFFFFFFFFull || samples < 1) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    std::vector<uint4> h_pc(n);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(h_pc.data(), 16, n, f) != n) {
        fprintf(stderr, "cannot read %llu elements from %s\n", (unsigned long long)n, argv[1]);
        return 2;
    }
    fclose(f);
    const size_t words = (size_t)((n + 31) / 32), groups = (size_t)extract_groups(n);
    const size_t table_words = size_t(1) << kNbMaxBits, blocks = table_words / kNbScanBlock;
    uint4 *pc, *records;
    uint32_t *head, *partials, *participants, *table, *sums, *bases, *counts, *selection, *seeds, *label, *size, *sizes, *seeded;
    CK(hipMalloc(&pc, 16 * n));
    CK(hipMalloc(&records, 16 * n));
    CK(hipMalloc(&head, 4 * (kNbResultWords + kNbMaxCount + 1u) + 8));  // the result block, the bins, the scan's total
    CK(hipMalloc(&partials, 4 * kNbPartialWords * groups));
    CK(hipMalloc(&participants, 4 * words));
    CK(hipMalloc(&table, 4 * table_words));
    CK(hipMalloc(&sums, 4 * blocks));
    CK(hipMalloc(&bases, 4 * blocks));
    CK(hipMalloc(&counts, 4 * n));
    CK(hipMalloc(&selection, 4 * words));
    CK(hipMalloc(&seeds, 4 * words));
    CK(hipMalloc(&label, 4 * n));
    CK(hipMalloc(&size, 4 * n));
    CK(hipMalloc(&sizes, 4 * n));
    CK(hipMalloc(&seeded, 4 * n));
    CK(hipMemcpy(pc, h_pc.data(), 16 * n, hipMemcpyHostToDevice));
    {
        std::vector<uint32_t> h_seeds(words, 0u);
        for (size_t w = 0; w < words; w += 32) h_seeds[w] = 1u;  // one Gaussian in 1024
        CK(hipMemcpy(seeds, h_seeds.data(), 4 * words, hipMemcpyHostToDevice));
    }
    hipStream_t s;
    CK(hipStreamCreate(&s));
    constexpr int kPasses = 13;
    const char* names[kPasses] = {"reset", "reduce", "cell", "scan", "scatter", "query", "init", "hook", "label", "stats",
                                  "select_by_size", "select_largest", "select_seeded"};
    hipEvent_t ev[kPasses + 1];
    for (auto& e : ev) CK(hipEventCreate(&e));
    const ModelFilter none{};
    const uint32_t blocks256 = (uint32_t)((n + 255u) / 256u);

    printf("{\"tool\": \"bench_clusters_kernels\", \"n\": %llu, \"samples\": %d, \"jobs\": [", (unsigned long long)n, samples);
    for (int a = 4; a < argc; ++a) {
        float radius = 0.0f;
        unsigned bits = 0;
        if (sscanf(argv[a], "%f:%u", &radius, &bits) != 2 || !nb_radius_ok(radius) || bits > kNbMaxBits) {
            fprintf(stderr, "bad job %s\n", argv[a]);
            return 2;
        }
        const NbGrid g = nb_grid(radius);
        ClusterJob job{};
        job.nb.r2 = g.r2;
        job.nb.inv_h = g.inv_h;
        job.nb.bits = bits ? bits : nb_auto_bits(n);
        job.nb.max_count = kNbMaxCount;
        job.nb.result = head;
        job.nb.hist = head + kNbResultWords;
        job.nb.scan_total = reinterpret_cast<uint64_t*>(head + kNbResultWords + kNbMaxCount + 1u);
        job.nb.partials = partials;
        job.nb.participants = participants;
        job.nb.table = table;
        job.nb.scan_sums = sums;
        job.nb.scan_bases = bases;
        job.nb.counts = counts;
        job.nb.records = records;
        job.nb.sel = SelectionWrite{GSX_SELECTION_ADD, 1u, selection, partials};
        job.label = label;
        job.size = size;
        job.sizes = sizes;
        job.seeded = seeded;
        job.seeds = 1u;
        std::vector<double> ms[kPasses];
        uint32_t h_res[kNbResultWords] = {0}, hits[3] = {0, 0, 0};
        for (int k = -1; k < samples; ++k) {  // (-1: the warm-up)
            CK(hipEventRecord(ev[0], s));
            CK(hipMemsetAsync(head, 0, 4 * (kNbResultWords + kNbMaxCount + 1u) + 8, s));
            CK(hipMemsetAsync(table, 0, 4 * (size_t(1) << job.nb.bits), s));
            CK(hipMemsetAsync(size, 0, 4 * n, s));
            CK(hipMemsetAsync(seeded, 0, 4 * n, s));
            CK(hipMemcpyAsync(selection, seeds, 4 * words, hipMemcpyDeviceToDevice, s));
            CK(hipEventRecord(ev[1], s));
            CK(launch_neighbors_reduce(s, n, none, pc, job.nb));
            CK(hipEventRecord(ev[2], s));
            CK(launch_neighbors_cell(s, n, none, pc, job.nb));
            CK(hipEventRecord(ev[3], s));
            CK(launch_neighbors_scan(s, job.nb));
            CK(hipEventRecord(ev[4], s));
            CK(launch_neighbors_scatter(s, n, pc, job.nb));
            CK(hipEventRecord(ev[5], s));
            CK(launch_neighbors_query(s, n, job.nb));
            CK(hipEventRecord(ev[6], s));
            GSX_LAUNCH(k_cl_init, dim3(blocks256), dim3(256), 0, s, n, job.nb.counts);
            CK(hipEventRecord(ev[7], s));
            GSX_LAUNCH(k_cl_hook, dim3(blocks256), dim3(256), 0, s, n, job.nb);
            CK(hipEventRecord(ev[8], s));
            CK(launch_clusters_label(s, n, job));
            CK(hipEventRecord(ev[9], s));
            CK(launch_clusters_stats(s, n, job));
            CK(hipEventRecord(ev[10], s));
            for (uint32_t mode = 0; mode < 3u; ++mode) {
                job.mode = mode;
                job.size_lo = mode == kClBySize ? 1u : 0u;
                job.size_hi = mode == kClBySize ? 4u : 0u;  // debris below 5
                CK(launch_clusters_select(s, n, job));
                CK(hipEventRecord(ev[11 + mode], s));
                if (k == samples - 1) {
                    CK(hipStreamSynchronize(s));
                    CK(hipMemcpy(h_res, head, sizeof h_res, hipMemcpyDeviceToHost));
                    hits[mode] = h_res[kNbHit];
                }
            }
            CK(hipEventSynchronize(ev[kPasses]));
            CK(hipGetLastError());
            if (k < 0) continue;
            for (int p = 0; p < kPasses; ++p) {
                float t = 0.0f;
                CK(hipEventElapsedTime(&t, ev[p], ev[p + 1]));
                ms[p].push_back((double)t);
            }
        }
        CK(hipMemcpy(h_res, head, sizeof h_res, hipMemcpyDeviceToHost));
        printf("%s{\"radius\": %.9g, \"grid_bits\": %u, \"count\": %u, \"clusters\": %u, \"largest\": %u, \"hit\": [%u, %u, %u], \"passes\": {", a > 4 ? ", " : "",
               (double)radius, job.nb.bits, h_res[kNbCount], h_res[kClClusters], h_res[kClKey + 1u], hits[0], hits[1], hits[2]);
        double total = 0.0;
        for (int p = 0; p < kPasses; ++p) {
            const double med = median(ms[p]);
            total += med;
            printf("%s\"%s\": {\"ms\": %.5f, \"ms_all\": [", p ? ", " : "", names[p], med);
            for (int k = 0; k < samples; ++k) printf("%s%.5f", k ? ", " : "", ms[p][k]);
            printf("]}");
        }
        printf("}, \"sum_ms\": %.5f, \"hook_over_query\": %.3f}", total, median(ms[7]) / median(ms[5]));
    }
    printf("]}\n");
    return 0;
}
