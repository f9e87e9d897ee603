// depthmap_driver.cpp — the depth map calls (spec section 25) through the C++ gs:: facade (include/gsx.hpp), for
// tests/test_gpu_depthmap_driver.py: one case — two models, the planes, the device pointers, unproject — on tools/frame_driver.cpp's
// LCG scene.  The driver checks what can be checked exactly on its own (the transmittance against the rendered frame, two calls
// against each other, the statistics against the planes, the refusal) and prints the figures the test compares with the Python
// facade's:
//   "depthmap_driver n=<n> models=<m> covered=<..> crossed=<..> layer0=<..> layer1=<..> front=<crossed at threshold 1> ok"
#include <cmath>
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

#define REQUIRE(cond)                                                             \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "depthmap_driver: %s (line %d)\n", #cond, __LINE__); \
            return 7;                                                             \
        }                                                                         \
    } while (0)

int main(int argc, char** argv) {
    try {
        const size_t n = argc > 1 ? (size_t)atol(argv[1]) : 3000;
        const uint32_t w = 96, h = 64;
        const size_t npx = (size_t)w * h, half = n / 2;
        auto g = make_scene(n, 12345u);
        auto viewer = gs::MultiModelViewer::new_with(0, {1, 1});
        viewer.add_model("a", half).gaussian_buffers.gaussians_buffer.update_range(0, g.data(), half);
        viewer.add_model("b", n - half).gaussian_buffers.gaussians_buffer.update_range(0, g.data() + half, n - half);
        viewer.update_gaussian_transform(1.0f, gs::GaussianDisplayMode::Splat, *gs::GaussianShDegree::new_(3), false);
        gs::CameraOrbitControl cam;
        cam.pos = {2.0f, 1.5f, -6.0f};
        viewer.update_camera(cam, {w, h});
        const std::vector<std::string> keys{"a", "b"};

        // the rendered frame
        for (const auto& k : keys) {
            viewer.preprocessor.preprocess(k);
            viewer.radix_sorter.sort(k);
        }
        viewer.renderer.render(keys);
        const std::vector<float> fb = viewer.download_framebuffer();

        // the depth map, twice
        std::vector<float> surface, sum, alpha, trans, surface2;
        std::vector<uint32_t> index, layer, index2;
        const gsx_depth_map_stats_t st = viewer.render_depth_map(keys, 0.5f, true, &surface, &sum, &alpha, &trans, &index, &layer);
        const gsx_depth_map_stats_t st2 = viewer.render_depth_map(keys, 0.5f, true, &surface2, nullptr, nullptr, nullptr, &index2);
        REQUIRE(memcmp(&st, &st2, sizeof st) == 0 && memcmp(surface.data(), surface2.data(), 4 * npx) == 0 && index == index2);
        REQUIRE(st.models == 2 && st.reserved == 0);
        uint64_t covered = 0, crossed = 0, by_layer[2] = {0, 0};
        float lo = INFINITY, hi = 0.0f;
        for (size_t i = 0; i < npx; ++i) {
            REQUIRE(memcmp(&trans[i], &fb[4 * i + 3], 4) == 0);  // the frame's T, bit for bit
            covered += alpha[i] > 0.0f;
            const bool x = index[i] != 0xFFFFFFFFu;
            REQUIRE(x == (layer[i] != 0xFFFFFFFFu) && x == std::isfinite(surface[i]));
            if (x) {
                REQUIRE(layer[i] < 2 && index[i] < (layer[i] == 0 ? half : n - half));
                REQUIRE(alpha[i] > 0.0f && sum[i] > 0.0f && trans[i] < 0.5f);
                crossed += 1;
                by_layer[layer[i]] += 1;
                lo = std::min(lo, surface[i]);
                hi = std::max(hi, surface[i]);
            }
        }
        REQUIRE(st.n_covered == covered && st.n_crossed == crossed && crossed > 0 && st.surface_min == lo && st.surface_max == hi);

        // the device pointers, and a surface point taken back to the world: it lies at that view depth
        const auto ptrs = viewer.depth_map_device_ptrs();
        REQUIRE(ptrs.surface && ptrs.sum && ptrs.alpha && ptrs.transmittance && ptrs.index && ptrs.layer && ptrs.ndc && ptrs.size.x == w && ptrs.size.y == h);
        {
            size_t at = 0;
            while (index[at] == 0xFFFFFFFFu) ++at;
            const auto view = cam.view();
            const auto proj = cam.projection((float)w / (float)h);
            const auto p = gs::MultiModelViewer::depth_map_unproject(view.data(), proj.data(), {w, h}, (float)(at % w) + 0.5f, (float)(at / w) + 0.5f, surface[at]);
            const float z = view[2] * p[0] + view[6] * p[1] + view[10] * p[2] + view[14];
            REQUIRE(std::fabs(-z - surface[at]) <= 1e-4f * std::max(1.0f, surface[at]));
        }
        // the front surface
        const gsx_depth_map_stats_t front = viewer.render_depth_map(keys, 1.0f);
        REQUIRE(front.n_crossed >= crossed && front.n_covered == covered);
        REQUIRE(viewer.depth_map_device_ptrs().ndc == nullptr);
        // a refusal is a gs::Error
        try { viewer.render_depth_map({"a", "a"}); return 2; } catch (const gs::Error& e) { if (e.status != GSX_ERR_INVALID_ARG) return 3; }
        try { viewer.render_depth_map({"a", "nobody"}); return 4; } catch (const gs::Error& e) { if (e.status != GSX_ERR_NOT_FOUND) return 5; }
        printf("depthmap_driver n=%zu models=%u covered=%llu crossed=%llu layer0=%llu layer1=%llu front=%llu ok\n", n, st.models, (unsigned long long)covered,
               (unsigned long long)crossed, (unsigned long long)by_layer[0], (unsigned long long)by_layer[1], (unsigned long long)front.n_crossed);
        return 0;
    } catch (const gs::Error& e) {
        fprintf(stderr, "gs::Error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
}
