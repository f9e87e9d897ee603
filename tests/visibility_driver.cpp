// visibility_driver.cpp — the visibility calls (spec section 24) through the C++ gs:: facade (include/gsx.hpp), for
// tests/test_gpu_visibility_driver.py: one case — reset, two views accumulated, select — on tools/frame_driver.cpp's LCG scene.
// The driver checks what can be checked exactly on its own (accumulation against the single views, the select against the downloaded
// planes, two calls against each other) and prints the figures the test compares with the Python facade's:
//   "visibility_driver n=<n> views=<v> seen_a=<..> seen_b=<..> seen=<..> pairs_a=<..> pairs_b=<..> never=<hit> selected=<..> ok"
#include <cstdio>
#include <cstring>

#include "../include/gsx.hpp"

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
static float u01(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

static std::vector<gs::Gaussian> make_scene(size_t n, uint32_t seed) {  // tools/frame_driver.cpp's
    std::vector<gs::Gaussian> g(n);
    uint32_t s = seed;
    for (auto& x : g) {
        float q[4];
        float l = 0;
        for (float& c : q) { c = u01(s) * 2 - 1; l += c * c; }
        l = std::sqrt(l);
        for (int k = 0; k < 4; ++k) x.rot[k] = q[k] / l;
        for (int k = 0; k < 3; ++k) x.pos[k] = u01(s) * 6 - 3;
        for (int k = 0; k < 4; ++k) x.color[k] = (uint8_t)(lcg(s) >> 24);
        for (int c = 0; c < 15; ++c)
            for (int ch = 0; ch < 3; ++ch) x.sh[c][ch] = (u01(s) - 0.5f) * 0.3f;
        for (int k = 0; k < 3; ++k) x.scale[k] = 0.02f + 0.2f * u01(s);
    }
    return g;
}

#define REQUIRE(cond)                                                               \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "visibility_driver: %s (line %d)\n", #cond, __LINE__); \
            return 7;                                                               \
        }                                                                           \
    } while (0)

int main(int argc, char** argv) {
    try {
        const size_t n = argc > 1 ? (size_t)atol(argv[1]) : 3000;
        const uint32_t w = 96, h = 64;
        auto g = make_scene(n, 12345u);
        auto viewer = gs::MultiModelViewer::new_with(0, {1, 1});
        auto& model = viewer.add_model("a", g.size());
        model.gaussian_buffers.gaussians_buffer.update_range(0, g.data(), g.size());
        viewer.update_gaussian_transform(1.0f, gs::GaussianDisplayMode::Splat, *gs::GaussianShDegree::new_(3), false);
        gs::CameraOrbitControl cams[2];
        cams[0].pos = {2.0f, 1.5f, -6.0f};
        cams[1].pos = {-5.0f, 0.5f, 3.0f};

        // the single views
        std::vector<float> peak[2], peak_again;
        std::vector<double> weight[2];
        std::vector<uint32_t> pixels[2];
        gsx_visibility_stats_t single[2];
        for (int k = 0; k < 2; ++k) {
            viewer.update_camera(cams[k], {w, h});
            single[k] = model.visibility(false, &peak[k], &weight[k], &pixels[k]);
            REQUIRE(single[k].views == 1 && single[k].n_pairs > 0);
        }
        const gsx_visibility_stats_t again = model.visibility(false, &peak_again);
        REQUIRE(memcmp(peak_again.data(), peak[1].data(), 4 * n) == 0 && again.n_pairs == single[1].n_pairs && again.weight_fixed == single[1].weight_fixed);

        // reset, two views accumulated
        model.visibility_reset();
        std::vector<float> acc_peak;
        std::vector<double> acc_weight;
        std::vector<uint32_t> acc_pixels;
        gsx_visibility_stats_t acc{};
        for (int k = 0; k < 2; ++k) {
            viewer.update_camera(cams[k], {w, h});
            acc = model.visibility(true, &acc_peak, &acc_weight, &acc_pixels);
        }
        REQUIRE(acc.views == 2);
        uint64_t seen = 0, never = 0;
        for (size_t i = 0; i < n; ++i) {
            REQUIRE(acc_peak[i] == std::max(peak[0][i], peak[1][i]));
            REQUIRE(acc_weight[i] == weight[0][i] + weight[1][i] && acc_pixels[i] == pixels[0][i] + pixels[1][i]);
            seen += acc_peak[i] > 0.0f;
            never += acc_peak[i] == 0.0f;
        }
        REQUIRE(acc.n_seen == seen && seen > 0 && never > 0);

        // select: never seen
        gsx_visibility_select_desc sd{};
        gsx_visibility_select_desc_default(&sd);
        sd.lo = sd.hi = 0.0;
        const auto hit = model.select_visibility(sd);
        REQUIRE(hit.first == never && hit.second == never);
        uint64_t bits = 0;
        const std::vector<uint32_t> words = model.gaussian_buffers.selection_buffer.download(n);
        for (size_t i = 0; i < n; ++i) {
            const bool sel = (words[i >> 5] >> (i & 31)) & 1u;
            REQUIRE(sel == (acc_peak[i] == 0.0f));
            bits += sel;
        }
        // the orbit helper, from raw matrices: the same planes
        {
            const auto va = cams[0].view(), vb = cams[1].view();
            const auto pa = cams[0].projection((float)w / (float)h), pb = cams[1].projection((float)w / (float)h);
            const gsx_visibility_stats_t orbit = model.visibility_orbit({{va.data(), pa.data()}, {vb.data(), pb.data()}}, w, h);
            REQUIRE(orbit.views == 2 && orbit.n_seen == seen);
        }
        // a refusal is a gs::Error
        model.visibility_reset();
        try { model.select_visibility(sd); return 2; } catch (const gs::Error& e) { if (e.status != GSX_ERR_INVALID_ARG) return 3; }
        printf("visibility_driver n=%zu views=%u seen_a=%llu seen_b=%llu seen=%llu pairs_a=%llu pairs_b=%llu never=%llu selected=%llu ok\n", n, acc.views,
               (unsigned long long)single[0].n_seen, (unsigned long long)single[1].n_seen, (unsigned long long)seen, (unsigned long long)single[0].n_pairs,
               (unsigned long long)single[1].n_pairs, (unsigned long long)hit.first, (unsigned long long)bits);
        return 0;
    } catch (const gs::Error& e) {
        fprintf(stderr, "gs::Error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
}
