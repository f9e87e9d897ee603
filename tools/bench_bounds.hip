// tools/bench_bounds.hip — the kernels of gsx_model_bounds (csrc/kernels_bounds.hip) and their yardstick k_mask_evaluate
// (csrc/kernels_mask.hip) on one position plane, timed with HIP events around the launches.  Both kernel files are included as
// source; nothing of libgsx is linked.  Not part of the product; tools/bench_bounds.py builds and runs it.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/bench_bounds.hip -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude \
//         -o tools/bench_bounds_kernels
//   tools/bench_bounds_kernels <pc.bin: n x float4 = x, y, z, rgba8 | - : seeded uniform positions> <n> [blocks=6] [reps=20]
// Rows (ms per call, median over the blocks of a run; two runs, blocks of the four rows alternating):
//   reduce        k_bounds_reduce, filter 0
//   reduce_all    k_bounds_reduce with mask, selection and stored edits present and all three flags set
//   trim          k_bounds_hist + k_bounds_trim at 20 permille, filter 0 (the trimmed passes alone, without the clear of the histograms)
//   mask_evaluate k_mask_evaluate with a one-box program: streams the same 16 B plane, more arithmetic per Gaussian
//   finish        k_bounds_finish alone (one workgroup over the partials)
// Prints one JSON line.
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_bounds.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_mask.hip"

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
    if (argc < 3) {
        fprintf(stderr, "usage: %s <pc.bin> <n> [blocks] [reps]\n", argv[0]);
        return 2;
    }
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    const int blocks = argc > 3 ? atoi(argv[3]) : 6, reps = argc > 4 ? atoi(argv[4]) : 20;
    if (n == 0 || n > 0xFFFFFFFFull || blocks < 1 || reps < 1 || (uint64_t)(reps + 3) * n > 0xFFFFFFFFull) {  // (a block's histogram counts add up in 32 bits)
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    std::vector<float4> h_pc(n);
    if (!strcmp(argv[1], "-")) {  // no file: seeded positions, uniform in [-4, 4]^3
        std::mt19937 gen(11);
        for (auto& p : h_pc) p = make_float4(8.0f * (gen() >> 8) / 16777216.0f - 4.0f, 8.0f * (gen() >> 8) / 16777216.0f - 4.0f,
                                             8.0f * (gen() >> 8) / 16777216.0f - 4.0f, 0.0f);
    } else {
        FILE* fp = fopen(argv[1], "rb");
        if (!fp || fread(h_pc.data(), sizeof(float4), n, fp) != n) {
            fprintf(stderr, "cannot read %llu positions from %s\n", (unsigned long long)n, argv[1]);
            return 2;
        }
        fclose(fp);
    }
    const size_t words = (size_t)((n + 31) / 32);
    std::mt19937 rng(7);
    std::vector<uint32_t> h_sel(words), h_edited(words);
    std::vector<float4> h_edit_a(n);
    for (size_t w = 0; w < words; ++w) {
        h_sel[w] = rng() | rng();        // three quarters selected
        h_edited[w] = rng() & rng();     // a quarter carries a stored edit ...
    }
    for (uint64_t i = 0; i < n; ++i) {   // ... half of which hide their Gaussian
        const uint32_t flag = GSX_EDIT_ENABLED | ((i & 1u) ? GSX_EDIT_HIDDEN : 0u);
        memcpy(&h_edit_a[i].x, &flag, 4);
        h_edit_a[i].y = h_edit_a[i].z = h_edit_a[i].w = 1.0f;
    }
    float4 *pc, *edit_a;
    uint32_t *mask, *sel, *edited, *hist;
    BoundsPartial* partials;
    gsx_model_bounds_t* out;
    CK(hipMalloc(&pc, sizeof(float4) * n));
    CK(hipMalloc(&edit_a, sizeof(float4) * n));
    CK(hipMalloc(&mask, 4 * words + 8));
    CK(hipMalloc(&sel, 4 * words));
    CK(hipMalloc(&edited, 4 * words));
    CK(hipMalloc(&hist, 4 * 3 * kBoundsBins));
    CK(hipMalloc(&partials, sizeof(BoundsPartial) * kBoundsMaxGroups));
    CK(hipMalloc(&out, 128));
    CK(hipMemcpy(pc, h_pc.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(edit_a, h_edit_a.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(sel, h_sel.data(), 4 * words, hipMemcpyHostToDevice));
    CK(hipMemcpy(edited, h_edited.data(), 4 * words, hipMemcpyHostToDevice));
    // the yardstick's program: one box of half-size 3 about the origin, identity model transform
    MaskProgram prog{};
    prog.m_rot[0] = prog.m_rot[4] = prog.m_rot[8] = 1.0f;
    prog.m_scale[0] = prog.m_scale[1] = prog.m_scale[2] = 1.0f;
    prog.n_shapes = 1;
    prog.n_ops = 1;
    prog.shapes[0].kind = GSX_MASK_BOX;
    prog.shapes[0].rot[0] = prog.shapes[0].rot[4] = prog.shapes[0].rot[8] = 1.0f;
    for (int c = 0; c < 3; ++c) {
        prog.shapes[0].scale[c] = 3.0f;
        prog.shapes[0].box_lim[c] = mask_box_limit(3.0f);
    }
    prog.ops[0].opcode = GSX_MASK_OP_SHAPE;
    prog.ops[0].arg = 0;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const ModelFilter none{};
    const ModelFilter all{mask, sel, edited, edit_a};
    const uint32_t groups = bounds_reduce_groups(n);
    auto row = [&](int r) {
        switch (r) {
            case 0: CK(launch_bounds_reduce(s, pc, n, none, partials)); break;
            case 1: CK(launch_bounds_reduce(s, pc, n, all, partials)); break;
            case 4: CK(launch_bounds_finish(s, partials, groups, false, out, hist)); break;
            case 2: CK(launch_bounds_trim(s, pc, n, none, 20u, out, hist)); break;
            default: CK(launch_mask_evaluate(s, pc, (uint32_t)n, prog, mask)); break;
        }
    };
    constexpr int kRows = 5;
    const char* names[kRows] = {"reduce", "reduce_all", "trim", "mask_evaluate", "finish"};
    // the mask first (reduce_all reads it), then filter 0's result: the check below, and the box the trimmed passes lay their bins over
    row(3);
    row(0);
    row(4);
    CK(hipStreamSynchronize(s));
    gsx_model_bounds_t h_out;
    CK(hipMemcpy(&h_out, out, sizeof h_out, hipMemcpyDeviceToHost));
    CK(hipMemsetAsync(hist, 0, 4 * 3 * kBoundsBins, s));
    for (int r = 0; r < kRows; ++r)
        for (int k = 0; k < 3; ++k) row(r);  // warm-up
    CK(hipStreamSynchronize(s));
    double med[2][kRows];
    for (int run = 0; run < 2; ++run) {
        std::vector<double> ms[kRows];
        for (int b = 0; b < blocks; ++b)
            for (int r = 0; r < kRows; ++r) {
                if (r == 2 || r == 4) row(0);  // filter 0's partials (outside the timed window) ...
                if (r == 2) row(4);            // ... and the box the histogram is laid over
                // the clear of the histograms is the library's k_bounds_finish's, so it stays outside the window: within a block the
                // counts of the calls add up (hence the 32-bit check on reps * n above); the passes do the same work on any counts
                if (r == 2) CK(hipMemsetAsync(hist, 0, 4 * 3 * kBoundsBins, s));
                CK(hipEventRecord(e0, s));
                for (int k = 0; k < reps; ++k) row(r);
                CK(hipEventRecord(e1, s));
                CK(hipEventSynchronize(e1));
                float t = 0.0f;
                CK(hipEventElapsedTime(&t, e0, e1));
                ms[r].push_back((double)t / reps);
            }
        for (int r = 0; r < kRows; ++r) med[run][r] = median(ms[r]);
    }
    const double plane = 16.0 * (double)n, planes = 3.0 * 4.0 * (double)words;
    printf("{\"tool\": \"bench_bounds_kernels\", \"n\": %llu, \"blocks\": %d, \"reps\": %d, \"count\": %llu, \"box\": [%g, %g, %g, %g, %g, %g]",
           (unsigned long long)n, blocks, reps, (unsigned long long)h_out.count, h_out.min[0], h_out.min[1], h_out.min[2], h_out.max[0],
           h_out.max[1], h_out.max[2]);
    for (int r = 0; r < kRows; ++r) {
        const double bytes = r == 4 ? 64.0 * groups : plane + (r == 1 ? planes : 0.0) + (r == 3 ? (double)n / 8.0 : 0.0);
        const double best = std::min(med[0][r], med[1][r]);
        printf(", \"%s_ms\": [%.5f, %.5f], \"%s_fraction_of_8TBps\": %.4f", names[r], med[0][r], med[1][r], names[r], bytes / (best * 1e-3) / 8e12);
    }
    printf("}\n");
    return 0;
}
