// tools/bench_neighbors.hip — the passes of the neighbour counts (csrc/kernels_neighbors.hip) on a file of position + colour elements,
// each timed with HIP events.  The kernel files are included as source; nothing of libgsx is linked.  Not part of the product;
// tools/bench_neighbors.py builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_neighbors.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_neighbors_kernels
//   tools/bench_neighbors_kernels <pc file: n x 16 bytes> <n> <samples> <radius>:<max_count>:<grid_bits (0: the library's)> ...
// Per job the passes run in their order (reset, reduce, cell, scan, scatter, query, select: each needs the one before), an event
// between every two; ms per pass: the median of `samples` runs after one warm-up, every sample listed.  Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_extract.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_neighbors.hip"

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
        fprintf(stderr, "usage: %s <pc file> <n> <samples> <radius>:<max_count>:<grid_bits> ...\n", argv[0]);
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
    uint32_t *head, *partials, *participants, *table, *sums, *bases, *counts, *selection;
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
    CK(hipMemcpy(pc, h_pc.data(), 16 * n, hipMemcpyHostToDevice));
    CK(hipMemset(selection, 0, 4 * words));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    constexpr int kPasses = 7;
    const char* names[kPasses] = {"reset", "reduce", "cell", "scan", "scatter", "query", "select"};
    hipEvent_t ev[kPasses + 1];
    for (auto& e : ev) CK(hipEventCreate(&e));
    const ModelFilter none{};

    printf("{\"tool\": \"bench_neighbors_kernels\", \"n\": %llu, \"samples\": %d, \"jobs\": [", (unsigned long long)n, samples);
    for (int a = 4; a < argc; ++a) {
        float radius = 0.0f;
        unsigned max_count = 0, bits = 0;
        if (sscanf(argv[a], "%f:%u:%u", &radius, &max_count, &bits) != 3 || !nb_radius_ok(radius) || max_count < 1 || max_count > kNbMaxCount || bits > kNbMaxBits) {
            fprintf(stderr, "bad job %s\n", argv[a]);
            return 2;
        }
        const NbGrid g = nb_grid(radius);
        NeighborJob job{};
        job.r2 = g.r2;
        job.inv_h = g.inv_h;
        job.bits = bits ? bits : nb_auto_bits(n);
        job.max_count = max_count;
        job.count_lo = 0;
        job.count_hi = max_count - 1u;  // the floaters recipe
        job.result = head;
        job.hist = head + kNbResultWords;
        job.scan_total = reinterpret_cast<uint64_t*>(head + kNbResultWords + kNbMaxCount + 1u);
        job.partials = partials;
        job.participants = participants;
        job.table = table;
        job.scan_sums = sums;
        job.scan_bases = bases;
        job.counts = counts;
        job.records = records;
        job.sel = SelectionWrite{GSX_SELECTION_SET, 1u, selection, partials};
        std::vector<double> ms[kPasses];
        uint32_t h_res[kNbResultWords] = {0};
        for (int k = -1; k < samples; ++k) {  // (-1: the warm-up)
            CK(hipEventRecord(ev[0], s));
            CK(hipMemsetAsync(head, 0, 4 * (kNbResultWords + kNbMaxCount + 1u) + 8, s));
            CK(hipMemsetAsync(table, 0, 4 * (size_t(1) << job.bits), s));
            CK(hipEventRecord(ev[1], s));
            CK(launch_neighbors_reduce(s, n, none, pc, job));
            CK(hipEventRecord(ev[2], s));
            CK(launch_neighbors_cell(s, n, none, pc, job));
            CK(hipEventRecord(ev[3], s));
            CK(launch_neighbors_scan(s, job));
            CK(hipEventRecord(ev[4], s));
            CK(launch_neighbors_scatter(s, n, pc, job));
            CK(hipEventRecord(ev[5], s));
            CK(launch_neighbors_query(s, n, job));
            CK(hipEventRecord(ev[6], s));
            CK(launch_neighbors_select(s, n, job));
            CK(hipEventRecord(ev[7], s));
            CK(hipEventSynchronize(ev[7]));
            if (k < 0) continue;
            for (int p = 0; p < kPasses; ++p) {
                float t = 0.0f;
                CK(hipEventElapsedTime(&t, ev[p], ev[p + 1]));
                ms[p].push_back((double)t);
            }
        }
        CK(hipMemcpy(h_res, head, sizeof h_res, hipMemcpyDeviceToHost));
        printf("%s{\"radius\": %.9g, \"max_count\": %u, \"grid_bits\": %u, \"count\": %u, \"hit\": %u, \"passes\": {", a > 4 ? ", " : "", (double)radius, max_count,
               job.bits, h_res[kNbCount], h_res[kNbHit]);
        double total = 0.0;
        for (int p = 0; p < kPasses; ++p) {
            const double med = median(ms[p]);
            total += med;
            printf("%s\"%s\": {\"ms\": %.5f, \"ms_all\": [", p ? ", " : "", names[p], med);
            for (int k = 0; k < samples; ++k) printf("%s%.5f", k ? ", " : "", ms[p][k]);
            printf("]}");
        }
        printf("}, \"sum_ms\": %.5f}", total);
    }
    printf("]}\n");
    return 0;
}
