// gsx.hpp — C++ host-side mirror of the `wgpu-3dgs-viewer` (gs::) surface the app uses for the render
// path, header-only over the C ABI of gsx.h.
//
// The reference's host language is Rust; there is no Rust toolchain in the build image, so this is the
// compiled-language facade (INTEGRATION.md shows the equivalent Rust binding).  Names, argument order and
// error behaviour follow the reference call sites (file:line under /root/reference/src):
//   gs::MultiModelViewer::new_with                       tab/scene.rs:1969-1980
//   viewer.models[key].gaussian_buffers.gaussians_buffer.update_range / len     tab/scene.rs:2083-2084, 608
//   viewer.update_camera / update_model_transform / update_gaussian_transform   tab/scene.rs:795-809
//   viewer.preprocessor.preprocess / radix_sorter.sort / renderer.render        tab/scene.rs:856-869, 2302-2314
//   device.poll(Maintain::Wait)                                                 tab/scene.rs:873
//   gs::CameraTrait {view, projection}, Mat4::look_at_rh / perspective_rh       app.rs:1236-1244
//   Quat::from_euler(EulerRot::ZYX, ..)                                         app.rs:1123-1130
// Fallible calls throw gs::Error (the reference returns Result<_, gs::Error>, app.rs:548).
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gsx.h"

namespace gs {

struct Error : std::runtime_error {
    gsx_status status;
    Error(gsx_status s, const char* msg) : std::runtime_error(msg), status(s) {}
};
inline void check(gsx_status s) {
    if (s != GSX_OK) throw Error(s, gsx_last_error_string());
}

using Gaussian = gsx_gaussian;  // {rot, pos, color, sh, scale}
using Vec3 = std::array<float, 3>;
using Quat = std::array<float, 4>;   // x, y, z, w
using Mat4 = std::array<float, 16>;  // column-major (glam to_cols_array)
struct UVec2 { uint32_t x, y; };

enum class GaussianDisplayMode : int { Splat = 0, Ellipse = 1, Point = 2 };  // app.rs:1147
enum class ShCompression : int { Single = 0, Half = 1, Norm8 = 2, Remove = 3 };  // app.rs:386-403
enum class Cov3dCompression : int { Single = 0, Half = 1 };                      // app.rs:405-418

class GaussianShDegree {  // transform.rs:139: `new` is None above 3
    uint32_t deg_;
    explicit GaussianShDegree(uint32_t d) : deg_(d) {}
public:
    static std::optional<GaussianShDegree> new_(uint32_t d) { return d <= 3 ? std::optional<GaussianShDegree>(GaussianShDegree(d)) : std::nullopt; }
    static GaussianShDegree new_unchecked(uint32_t d) { return GaussianShDegree(d); }
    uint32_t degree() const { return deg_; }
};

// ---- glam 0.29.2 restated in float32 ----
inline Vec3 sub(Vec3 a, Vec3 b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
inline float dot(Vec3 a, Vec3 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline Vec3 cross(Vec3 a, Vec3 b) { return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}; }
inline Vec3 normalize(Vec3 a) { float l = std::sqrt(dot(a, a)); return {a[0] / l, a[1] / l, a[2] / l}; }
inline Mat4 look_to_rh(Vec3 eye, Vec3 dir, Vec3 up) {
    Vec3 f = normalize(dir), s = normalize(cross(f, up)), u = cross(s, f);
    return {s[0], u[0], -f[0], 0, s[1], u[1], -f[1], 0, s[2], u[2], -f[2], 0, -dot(eye, s), -dot(eye, u), dot(eye, f), 1};
}
inline Mat4 look_at_rh(Vec3 eye, Vec3 center, Vec3 up) { return look_to_rh(eye, sub(center, eye), up); }
inline Mat4 perspective_rh(float fov_y, float aspect, float z_near, float z_far) {
    float s = std::sin(0.5f * fov_y), c = std::cos(0.5f * fov_y), h = c / s, w = h / aspect, r = z_far / (z_near - z_far);
    return {w, 0, 0, 0, 0, h, 0, 0, 0, 0, r, -1, 0, 0, r * z_near, 0};
}
inline Quat quat_mul(Quat a, Quat b) {
    return {a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
            a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]};
}
inline Quat quat_from_euler_zyx(float z, float y, float x) {  // Quat::from_euler(EulerRot::ZYX, z, y, x)
    Quat qz{0, 0, std::sin(0.5f * z), std::cos(0.5f * z)}, qy{0, std::sin(0.5f * y), 0, std::cos(0.5f * y)},
        qx{std::sin(0.5f * x), 0, 0, std::cos(0.5f * x)};
    return quat_mul(quat_mul(qz, qy), qx);
}

struct CameraTrait {  // gs::CameraTrait
    virtual ~CameraTrait() = default;
    virtual Mat4 view() const = 0;
    virtual Mat4 projection(float aspect_ratio) const = 0;
};
struct CameraOrbitControl : CameraTrait {  // app.rs:1208-1244
    Vec3 target{0, 0, 0}, pos{0, 0, -1};
    float z_near = 0.1f, z_far = 1e4f, vertical_fov = 1.0471975512f;
    Mat4 view() const override { return look_at_rh(pos, target, {0, 1, 0}); }
    Mat4 projection(float aspect) const override { return perspective_rh(vertical_fov, aspect, z_near, z_far); }
};

class MultiModelViewer;

class GaussiansBuffer {  // gs::GaussiansBuffer<G>
    gsx_viewer* v_;
    std::string key_;
public:
    GaussiansBuffer(gsx_viewer* v, std::string key) : v_(v), key_(std::move(key)) {}
    size_t len() const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        return (size_t)n;
    }
    void update_range(size_t start, const Gaussian* gaussians, size_t n) {  // scene.rs:2083-2084
        check(gsx_model_upload_range(v_, key_.c_str(), start, gaussians, n));
    }
    void update_range(size_t start, const std::vector<Gaussian>& g) { update_range(start, g.data(), g.size()); }
    // gsx_model_upload_ply_rows: n binary PLY vertex rows of header.vertex_bytes each, decoded on the device into the Gaussians from
    // `start` on (spec section 15): update_range of the rows' Gaussians without the records in between
    void update_range_ply(size_t start, const void* rows, size_t n, const gsx_ply_header& header, uint64_t staging_bytes = 0) {
        const gsx_import_desc d{0u, 0u, staging_bytes};
        check(gsx_model_upload_ply_rows(v_, key_.c_str(), start, rows, n, &header, &d));
    }
};
// A cloned buffer (`edit_buffer.clone()` / `mask_buffer.clone()`, app.rs:769-780): copyable, shares one device-side snapshot
// taken at clone time; download() may run on any thread while the viewer renders (gsx_buffer_*).
template <class T>
class BufferClone {
    gsx_buffer* h_ = nullptr;
public:
    BufferClone(gsx_viewer* v, const std::string& key, gsx_buffer_kind kind) { check(gsx_model_buffer_retain(v, key.c_str(), kind, &h_)); }
    BufferClone(const BufferClone& o) : h_(o.h_) { if (h_) check(gsx_buffer_retain(h_)); }
    BufferClone(BufferClone&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    BufferClone& operator=(BufferClone o) noexcept { std::swap(h_, o.h_); return *this; }
    ~BufferClone() { gsx_buffer_release(h_); }
    std::vector<T> download() const {
        uint64_t n = 0;
        check(gsx_buffer_len(h_, &n));
        std::vector<T> out(n);
        check(gsx_buffer_download(h_, out.data(), n));
        return out;
    }
};
class MaskBuffer {  // gs::MaskBuffer (scene.rs:1851, app.rs:806-807): bit = kept
    gsx_viewer* v_;
    std::string key_;
public:
    MaskBuffer(gsx_viewer* v, std::string key) : v_(v), key_(std::move(key)) {}
    void upload(const std::vector<uint32_t>& words) { check(gsx_model_upload_mask(v_, key_.c_str(), words.data(), words.size())); }
    std::vector<uint32_t> download(size_t n_gaussians) {
        std::vector<uint32_t> w((n_gaussians + 31) / 32);
        check(gsx_model_download_mask(v_, key_.c_str(), w.data(), w.size()));
        return w;
    }
    BufferClone<uint32_t> clone() const { return BufferClone<uint32_t>(v_, key_, GSX_BUFFER_MASK); }  // app.rs:775
};
class SelectionBuffer {  // gs::SelectionBuffer (scene.rs:1846-1850): bit = selected
    gsx_viewer* v_;
    std::string key_;
public:
    SelectionBuffer(gsx_viewer* v, std::string key) : v_(v), key_(std::move(key)) {}
    void upload(const std::vector<uint32_t>& words) { check(gsx_model_upload_selection(v_, key_.c_str(), words.data(), words.size())); }
    void clear() { check(gsx_model_upload_selection(v_, key_.c_str(), nullptr, 0)); }
    std::vector<uint32_t> download(size_t n_gaussians) {
        std::vector<uint32_t> w((n_gaussians + 31) / 32);
        check(gsx_model_download_selection(v_, key_.c_str(), w.data(), w.size()));
        return w;
    }
    BufferClone<uint32_t> clone() const { return BufferClone<uint32_t>(v_, key_, GSX_BUFFER_SELECTION); }
};
using GaussianEditPod = gsx_gaussian_edit;  // gs::GaussianEditPod (app.rs:1553-1562)
class GaussiansEditBuffer {  // gs::GaussiansEditBuffer (scene.rs:1816-1830, app.rs:789)
    gsx_viewer* v_;
    std::string key_;
public:
    GaussiansEditBuffer(gsx_viewer* v, std::string key) : v_(v), key_(std::move(key)) {}
    std::vector<GaussianEditPod> download(size_t n_gaussians) {
        std::vector<GaussianEditPod> e(n_gaussians);
        check(gsx_model_download_edits(v_, key_.c_str(), e.data(), e.size()));
        return e;
    }
    void upload(const std::vector<GaussianEditPod>& e) { check(gsx_model_upload_edits(v_, key_.c_str(), e.data(), e.size())); }
    BufferClone<GaussianEditPod> clone() const { return BufferClone<GaussianEditPod>(v_, key_, GSX_BUFFER_EDITS); }  // app.rs:772
};
struct MultiModelViewerGaussianBuffers {
    GaussiansBuffer gaussians_buffer;
    MaskBuffer mask_buffer;
    SelectionBuffer selection_buffer;
    GaussiansEditBuffer gaussians_edit_buffer;
};
using ModelBounds = gsx_model_bounds_t;  // box, centre (GaussianSplattingModel::center, app.rs:1019-1046), centroid, trimmed box
struct MultiModelViewerModel {
    MultiModelViewerGaussianBuffers gaussian_buffers;
    gsx_viewer* v_ = nullptr;
    std::string key_;
    // gsx_model_bounds: model space, Gaussian centres; filter = GSX_BOUNDS_* flags, trim_permille < 500.  After the last
    // update_range of a load: model.center = viewer.models.at(key).bounds().center
    ModelBounds bounds(uint32_t filter = 0, uint32_t trim_permille = 0) const {
        const gsx_bounds_desc d{filter, trim_permille};
        ModelBounds b;
        check(gsx_model_bounds(v_, key_.c_str(), &d, &b));
        return b;
    }
    // gsx_model_pod_kind: the kinds this model's planes are stored in (a viewer may hold models of several kinds after convert)
    std::pair<ShCompression, Cov3dCompression> pod_kind() const {
        gsx_sh_kind s = GSX_SH_SINGLE;
        gsx_cov3d_kind c = GSX_COV3D_SINGLE;
        check(gsx_model_pod_kind(v_, key_.c_str(), &s, &c));
        return {(ShCompression)s, (Cov3dCompression)c};
    }
    // gsx_model_set_pod_kind: the Compression Settings menu (app.rs:152-177) applied to this loaded model: same key, length, transform,
    // mask, selection and edits; the planes requantised on the device; the next frame unspeculated.  The same kind does nothing.
    void set_pod_kind(ShCompression sh, Cov3dCompression cov3d) {
        check(gsx_model_set_pod_kind(v_, key_.c_str(), (gsx_sh_kind)sh, (gsx_cov3d_kind)cov3d));
    }
    // gsx_model_apply_transform: the Gaussians that pass desc.filter (desc.flags GSX_EXTRACT_INVERT: those that do not) are moved,
    // rotated, scaled or mirrored about desc.pivot where they lie, on the device: positions, covariances, SH and shade records as
    // gsx_model_merge bakes a model transform; order, mask, selection and edits stay.  "Rotate the selection about its centre":
    // pivot = bounds(GSX_BOUNDS_SELECTED).center.  Returns the number of Gaussians moved.
    uint64_t apply_transform(const gsx_transform_desc& desc) {
        uint64_t count = 0;
        check(gsx_model_apply_transform(v_, key_.c_str(), &desc, &count));
        return count;
    }
    // gsx_model_decimate without a destination: how a grid of edge desc.cell would divide the model: the statistics, and in map (the
    // model's length) the cell every Gaussian would go into (0xFFFFFFFF: it does not participate).  Nothing is created.
    gsx_decimate_stats_t decimate_count(const gsx_decimate_desc& desc, std::vector<uint32_t>* map = nullptr) const {
        if (map) {
            uint64_t n = 0;
            check(gsx_model_len(v_, key_.c_str(), &n));
            map->assign((size_t)n, 0xFFFFFFFFu);
        }
        gsx_decimate_stats_t out{};
        check(gsx_model_decimate(v_, key_.c_str(), nullptr, &desc, map ? map->data() : nullptr, &out));
        return out;
    }
    // gsx_model_decimate_edge: the smallest probed cell edge that leaves at most target_cells cells, by count-only bisection on the
    // device.  Returns {edge, cells}.
    std::pair<float, uint64_t> decimate_edge(uint64_t target_cells, uint32_t filter = 0, uint32_t flags = 0) const {
        float cell = 0.0f;
        uint64_t cells = 0;
        check(gsx_model_decimate_edge(v_, key_.c_str(), filter, flags, target_cells, &cell, &cells));
        return {cell, cells};
    }
    // gsx_model_property_values: one float32 per Gaussian, computed on the device from the stored values (edits are not applied): the
    // stored position (flags = GSX_PROP_WORLD: the model transform applied as merge bakes it), the bytes of the colour word / 255, their
    // HSV, or the scales export solves from the covariance.
    std::vector<float> property_values(gsx_property property, uint32_t flags = 0) const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        std::vector<float> out((size_t)n);
        check(gsx_model_property_values(v_, key_.c_str(), (uint32_t)property, flags, out.data(), n));
        return out;
    }
    // gsx_model_histogram: desc.bins equal bins of the property over [lo, hi] (GSX_HIST_AUTO_RANGE: over [min, max], returned in the
    // result's lo / hi) among the Gaussians that pass desc.filter and have a finite value.  bins receives the counts.
    gsx_histogram_t histogram(const gsx_histogram_desc& desc, std::vector<uint64_t>& bins) const {
        bins.assign(desc.bins ? desc.bins : 1u, 0);
        gsx_histogram_t h{};
        check(gsx_model_histogram(v_, key_.c_str(), &desc, bins.data(), &h));
        return h;
    }
    // gsx_model_select_range: the Gaussians that pass desc.filter, have a finite value in [lo, hi] and (desc.bins > 0) a bin in [bin_lo,
    // bin_hi] are the hit set; desc.selection_op sets, adds or removes it, on the device.  Returns {hit, selected afterwards}.
    std::pair<uint64_t, uint64_t> select_range(const gsx_select_desc& desc) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_range(v_, key_.c_str(), &desc, &hit, &selected));
        return {hit, selected};
    }
    // gsx_model_neighbors: for every Gaussian, how many others lie within desc.radius of it in model space (d2 <= r2 in float32),
    // saturated at desc.max_count, among the Gaussians that pass desc.filter and have a finite position; computed on the device with a
    // hashed grid.  counts receives one count per Gaussian, hist[c] the number of participants with count c.
    gsx_neighbor_stats_t neighbors(const gsx_neighbor_desc& desc, std::vector<uint32_t>& counts, std::vector<uint64_t>& hist) const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        counts.assign((size_t)n, 0u);
        hist.assign((size_t)(desc.max_count < GSX_NEIGHBOR_MAX_COUNT ? desc.max_count : GSX_NEIGHBOR_MAX_COUNT) + 1u, 0);
        gsx_neighbor_stats_t out{};
        check(gsx_model_neighbors(v_, key_.c_str(), &desc, counts.data(), hist.data(), &out));
        return out;
    }
    // gsx_model_select_neighbors: the participants whose saturated count lies in [count_lo, count_hi] are the hit set;
    // desc.selection_op sets, adds or removes it, on the device.  Floaters with fewer than k neighbours: max_count = k, [0, k - 1].
    // Returns {hit, selected afterwards}.
    std::pair<uint64_t, uint64_t> select_neighbors(const gsx_neighbor_select_desc& desc) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_neighbors(v_, key_.c_str(), &desc, &hit, &selected));
        return {hit, selected};
    }
    // gsx_model_clusters: the connected pieces of the model under "within desc.radius of one another" (d2 <= r2 in float32, model
    // space), among the Gaussians that pass desc.filter and have a finite position; computed on the device by a union-find over a
    // hashed grid.  labels receives the smallest Gaussian index of each Gaussian's cluster (GSX_CLUSTER_NONE for one that does not
    // participate), sizes the size of its cluster.
    gsx_cluster_stats_t clusters(const gsx_cluster_desc& desc, std::vector<uint32_t>& labels, std::vector<uint32_t>& sizes) const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        labels.assign((size_t)n, GSX_CLUSTER_NONE);
        sizes.assign((size_t)n, 0u);
        gsx_cluster_stats_t out{};
        check(gsx_model_clusters(v_, key_.c_str(), &desc, labels.data(), sizes.data(), &out));
        return out;
    }
    // gsx_model_select_clusters: the hit set is, by desc.mode, the clusters with a size in [size_lo, size_hi], the largest cluster, or
    // the clusters that hold a selected Gaussian; desc.selection_op sets, adds or removes it, on the device.  Returns {hit, selected
    // afterwards}.
    std::pair<uint64_t, uint64_t> select_clusters(const gsx_cluster_select_desc& desc) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_clusters(v_, key_.c_str(), &desc, &hit, &selected));
        return {hit, selected};
    }
    // gsx_model_knn: every Gaussian's desc.k smallest squared distances to the others (float32, model space), a score from them
    // (GSX_KNN_SCORE_*) and the score's statistics, among the Gaussians that pass desc.filter and have a finite position; computed on
    // the device, bit for bit the brute-force answer.  score receives one float a Gaussian, d2 (nullable) n * k floats, row i at i *
    // k; both +inf for a Gaussian that does not participate.
    gsx_knn_stats_t knn(const gsx_knn_desc& desc, std::vector<float>& score, std::vector<float>* d2 = nullptr) const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        score.assign((size_t)n, std::numeric_limits<float>::infinity());
        if (d2) d2->assign((size_t)n * desc.k, std::numeric_limits<float>::infinity());
        gsx_knn_stats_t out{};
        check(gsx_model_knn(v_, key_.c_str(), &desc, d2 ? d2->data() : nullptr, score.data(), &out));
        return out;
    }
    // gsx_model_select_knn: the hit set is, by desc.mode, the participants with a score in [lo, hi] or the statistical outliers (score
    // above mean + std_ratio * std); desc.selection_op sets, adds or removes it, on the device.  Returns {hit, selected afterwards};
    // stats (nullable) receives the statistics and the threshold.
    std::pair<uint64_t, uint64_t> select_knn(const gsx_knn_select_desc& desc, gsx_knn_stats_t* stats = nullptr) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_knn(v_, key_.c_str(), &desc, &hit, &selected, stats));
        return {hit, selected};
    }
    // gsx_model_normals: a plane fitted in double to every Gaussian and its desc.k nearest (by squared distance, then index), among the
    // Gaussians that pass desc.filter and have a finite position, on the device.  normal receives n * 3 floats ((0, 0, 0) where none
    // is fitted), variation one float a Gaussian (+inf there), index (nullable) n * k words, row i at i * k, GSX_NORMALS_NONE where
    // there is no such neighbour.
    gsx_normals_stats_t normals(const gsx_normals_desc& desc, std::vector<float>& normal, std::vector<float>& variation,
                                std::vector<uint32_t>* index = nullptr) const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        normal.assign((size_t)n * 3, 0.0f);
        variation.assign((size_t)n, std::numeric_limits<float>::infinity());
        if (index) index->assign((size_t)n * desc.k, GSX_NORMALS_NONE);
        gsx_normals_stats_t out{};
        check(gsx_model_normals(v_, key_.c_str(), &desc, normal.data(), variation.data(), index ? index->data() : nullptr, &out));
        return out;
    }
    // gsx_model_select_normals: the hit set is, by desc.mode, the fitted Gaussians with a variation in [lo, hi] or with a cosine
    // between their normal and desc.dir in [lo, hi]; desc.selection_op sets, adds or removes it, on the device.  Returns {hit,
    // selected afterwards}; stats (nullable) receives the statistics.
    std::pair<uint64_t, uint64_t> select_normals(const gsx_normals_select_desc& desc, gsx_normals_stats_t* stats = nullptr) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_normals(v_, key_.c_str(), &desc, &hit, &selected, stats));
        return {hit, selected};
    }
    // gsx_model_nearest: for every Gaussian of this model, mapped by desc.xform (or by the two models' transforms), the nearest
    // Gaussian of the model dst_key: index (GSX_NEAREST_NONE where none) and squared distance (+inf there), both nullable, on the
    // device, bit for bit the brute-force answer with ties going to the smaller index.  The stats carry the one-sided chamfer (mean)
    // and Hausdorff (d_max) distances and the matrix used.
    gsx_nearest_stats_t nearest(const std::string& dst_key, const gsx_nearest_desc& desc, std::vector<uint32_t>* index = nullptr,
                                std::vector<float>* d2 = nullptr) const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        if (index) index->assign((size_t)n, GSX_NEAREST_NONE);
        if (d2) d2->assign((size_t)n, std::numeric_limits<float>::infinity());
        gsx_nearest_stats_t out{};
        check(gsx_model_nearest(v_, key_.c_str(), dst_key.c_str(), &desc, index ? index->data() : nullptr, d2 ? d2->data() : nullptr, &out));
        return out;
    }
    // gsx_model_select_nearest: writes THIS model's selection; the hit set is, by desc.mode, the Gaussians whose distance to the model
    // dst_key lies in [lo, hi] or those whose nearest target is selected there.  Returns {hit, selected afterwards}.
    std::pair<uint64_t, uint64_t> select_nearest(const std::string& dst_key, const gsx_nearest_select_desc& desc, gsx_nearest_stats_t* stats = nullptr) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_nearest(v_, key_.c_str(), dst_key.c_str(), &desc, &hit, &selected, stats));
        return {hit, selected};
    }
    // gsx_model_align_step: one least-squares step of point-to-point registration of this model onto the model dst_key.
    gsx_align_step_t align_step(const std::string& dst_key, const gsx_align_desc& desc) const {
        gsx_align_step_t out{};
        check(gsx_model_align_step(v_, key_.c_str(), dst_key.c_str(), &desc, &out));
        return out;
    }
    // Iterative closest point: align_step until rms_before changes by less than tol relatively or does not fall any more (at the
    // float32 rounding of the positions it only flickers: a rise is the end), a step is degenerate or max_iters steps ran; every step starts from the step before's xform_next.  Returns the last step: its nearest.xform is the final
    // matrix.  delta (nullable, 12 doubles, row-major 3x4) receives the composed similarity D with final = D o initial.
    gsx_align_step_t align(const std::string& dst_key, gsx_align_desc desc, uint32_t max_iters = 30, double tol = 1e-6, double* delta = nullptr) const {
        double D[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        gsx_align_step_t out{};
        double last = -1.0;
        for (uint32_t it = 0; it < max_iters; ++it) {
            out = align_step(dst_key, desc);
            const double now = out.rms_before;
            if (out.degenerate || (last >= 0.0 && (now >= last || last - now <= tol * last))) break;
            last = now;
            const double x = out.quat[0], y = out.quat[1], z = out.quat[2], w = out.quat[3], s = out.scale;
            const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                                 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
            double next[12];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c)
                    next[4 * r + c] = s * (R[3 * r] * D[c] + R[3 * r + 1] * D[4 + c] + R[3 * r + 2] * D[8 + c]) + (c == 3 ? out.pos[r] : 0.0);
            for (int k = 0; k < 12; ++k) D[k] = next[k];
            desc.nearest.flags &= ~GSX_NEAREST_MODEL_TRANSFORMS;  // (from the second step on the matrix is the step before's)
            for (int k = 0; k < 12; ++k) desc.nearest.xform[k] = out.xform_next[k];
        }
        if (delta)
            for (int k = 0; k < 12; ++k) delta[k] = D[k];
        return out;
    }
    // gsx_model_normals_keep: normals() whose normals and variations stay on the device with the model (16 bytes a Gaussian), for
    // align_plane_step; a second keep replaces the first.  An upload, an import, a transform and a pod kind change drop the plane.
    gsx_normals_stats_t keep_normals(const gsx_normals_desc& desc) {
        gsx_normals_stats_t out{};
        check(gsx_model_normals_keep(v_, key_.c_str(), &desc, &out));
        return out;
    }
    // gsx_model_normals_kept: whether a plane is resident and what it was made with; normal (n * 3) and variation (n), both nullable,
    // receive its contents and stay as they are without a plane.
    gsx_normals_kept_t kept_normals(std::vector<float>* normal = nullptr, std::vector<float>* variation = nullptr) const {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        gsx_normals_kept_t out{};
        check(gsx_model_normals_kept(v_, key_.c_str(), &out, nullptr, nullptr));
        if (out.present && (normal || variation)) {
            if (normal) normal->assign((size_t)n * 3, 0.0f);
            if (variation) variation->assign((size_t)n, std::numeric_limits<float>::infinity());
            check(gsx_model_normals_kept(v_, key_.c_str(), &out, normal ? normal->data() : nullptr, variation ? variation->data() : nullptr));
        }
        return out;
    }
    // gsx_model_normals_reset: frees the kept plane.
    void reset_normals() { check(gsx_model_normals_reset(v_, key_.c_str())); }
    // gsx_model_align_plane_step: one Gauss-Newton step of point-to-plane registration of this model onto the model dst_key, which
    // needs keep_normals first.  The step moves only along what the pairs determine (out.rank of the six motions).
    gsx_align_plane_step_t align_plane_step(const std::string& dst_key, const gsx_align_plane_desc& desc) const {
        gsx_align_plane_step_t out{};
        check(gsx_model_align_plane_step(v_, key_.c_str(), dst_key.c_str(), &desc, &out));
        return out;
    }
    // gsx_model_fit_plane: the model's dominant plane by consensus, on the device: desc.n_candidates planes (sampled from triples,
    // from kept normals, or the caller's `candidates`, which are used as given), every participant tested against every plane, the
    // winner refined by least squares.  out_candidates and out_counts (nullable) receive every candidate and its exact inlier count.
    // Level a capture: plane_level(fit.plane, up, quat, pos), then update_model_transform.  Remove the floor: select_plane with lo =
    // -inf, hi = tolerance, then extract with GSX_BOUNDS_SELECTED and GSX_EXTRACT_INVERT.  Peel the next plane: select_plane with
    // GSX_SELECTION_ADD, then fit again with filter GSX_BOUNDS_SELECTED and flags GSX_EXTRACT_INVERT.
    static gsx_plane_fit_desc plane_fit_desc() {
        gsx_plane_fit_desc d{};
        gsx_plane_fit_desc_default(&d);
        return d;
    }
    gsx_plane_fit_t fit_plane(const gsx_plane_fit_desc& desc, const std::vector<gsx_plane_t>* candidates = nullptr,
                              std::vector<gsx_plane_t>* out_candidates = nullptr, std::vector<uint32_t>* out_counts = nullptr) const {
        if (candidates && candidates->size() < desc.n_candidates) throw std::invalid_argument("fit_plane: fewer candidates than desc.n_candidates");
        const size_t rows = desc.n_candidates <= GSX_PLANE_MAX_CANDIDATES ? desc.n_candidates : 0;  // (the call refuses more)
        if (out_candidates) out_candidates->assign(rows, gsx_plane_t{});
        if (out_counts) out_counts->assign(rows, 0u);
        gsx_plane_fit_t out{};
        check(gsx_model_fit_plane(v_, key_.c_str(), &desc, candidates ? candidates->data() : nullptr, out_candidates && rows ? out_candidates->data() : nullptr,
                                  out_counts && rows ? out_counts->data() : nullptr, &out));
        return out;
    }
    // gsx_model_select_plane: the participants whose signed residual against desc.plane lies in [lo, hi] (a bound may be infinite)
    // and, with min_cos > 0, whose kept normal is within that cosine of the plane's; desc.selection_op sets, adds or removes the hit
    // set, on the device.  Returns {hit, selected afterwards}.
    static gsx_plane_select_desc plane_select_desc() {
        gsx_plane_select_desc d{};
        gsx_plane_select_desc_default(&d);
        return d;
    }
    std::pair<uint64_t, uint64_t> select_plane(const gsx_plane_select_desc& desc) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_plane(v_, key_.c_str(), &desc, &hit, &selected));
        return {hit, selected};
    }
    // gsx_plane_level (host only): the shortest-arc rotation (x, y, z, w; w >= 0) that takes the plane's unit normal to up / |up| and
    // the translation that puts the rotated plane through the origin's height: update_model_transform's or apply_transform's
    // arguments with scale 1.
    static void plane_level(const gsx_plane_t& plane, const float up[3], float quat_xyzw[4], float pos[3]) {
        check(gsx_plane_level(&plane, up, quat_xyzw, pos));
    }
    // gsx_model_visibility: draws this model ALONE with the viewer's current camera and keeps, per Gaussian and on the device, the
    // peak blending weight T * alpha, the summed weight (2^-24 fixed point, as double) and the pixel count; accumulate folds the
    // view into the planes an earlier call left.  Every output is nullable.  The model goes through preprocess + sort again before
    // the next render(); render_frame() needs nothing.
    gsx_visibility_stats_t visibility(bool accumulate = false, std::vector<float>* peak = nullptr, std::vector<double>* weight = nullptr,
                                      std::vector<uint32_t>* pixels = nullptr, std::vector<float>* transmittance = nullptr,
                                      uint32_t width = 0, uint32_t height = 0) {
        uint64_t n = 0;
        check(gsx_model_len(v_, key_.c_str(), &n));
        if (peak) peak->assign((size_t)n, 0.0f);
        if (weight) weight->assign((size_t)n, 0.0);
        if (pixels) pixels->assign((size_t)n, 0u);
        if (transmittance) transmittance->assign((size_t)width * height, 1.0f);  // (the viewport of the view: the caller knows it)
        gsx_visibility_desc desc{};
        gsx_visibility_desc_default(&desc);
        desc.flags = accumulate ? GSX_VIS_ACCUMULATE : 0u;
        gsx_visibility_stats_t out{};
        check(gsx_model_visibility(v_, key_.c_str(), &desc, peak ? peak->data() : nullptr, weight ? weight->data() : nullptr,
                                   pixels ? pixels->data() : nullptr, transmittance ? transmittance->data() : nullptr, &out));
        return out;
    }
    // gsx_model_select_visibility: selects the Gaussians that pass desc.filter and whose resident measure lies in [lo, hi];
    // "never seen" is GSX_VIS_PEAK in [0, 0].  Returns {hit, selected afterwards}.
    std::pair<uint64_t, uint64_t> select_visibility(const gsx_visibility_select_desc& desc) {
        uint64_t hit = 0, selected = 0;
        check(gsx_model_select_visibility(v_, key_.c_str(), &desc, &hit, &selected));
        return {hit, selected};
    }
    // gsx_model_visibility_reset: frees the resident planes
    void visibility_reset() { check(gsx_model_visibility_reset(v_, key_.c_str())); }
    // Resets the planes, then folds one view per camera (16 floats of view and of projection each, column-major): every Gaussian's
    // best and summed contribution over an orbit.  The viewer keeps the last camera.  Returns the last view's statistics.
    gsx_visibility_stats_t visibility_orbit(const std::vector<std::pair<const float*, const float*>>& cameras, uint32_t width, uint32_t height) {
        visibility_reset();
        gsx_visibility_stats_t out{};
        for (const auto& c : cameras) {
            check(gsx_update_camera(v_, c.first, c.second, width, height));
            out = visibility(true);
        }
        return out;
    }
};

class MultiModelViewer {
    gsx_viewer* v_ = nullptr;
    struct Pre { gsx_viewer*& v; void preprocess(const std::string& key) { check(gsx_preprocess(v, key.c_str())); } };
    struct Sort { gsx_viewer*& v; void sort(const std::string& key) { check(gsx_sort(v, key.c_str())); } };
    struct Post { gsx_viewer*& v; void postprocess(const std::string& key) { check(gsx_postprocess(v, key.c_str())); } };  // scene.rs:601-611
    struct Ren {
        gsx_viewer*& v;
        void render(const std::vector<std::string>& model_render_keys) {  // far -> near, scene.rs:533-558
            std::vector<const char*> k;
            for (auto& s : model_render_keys) k.push_back(s.c_str());
            check(gsx_render(v, k.data(), (uint32_t)k.size()));
        }
    };
public:
    std::map<std::string, MultiModelViewerModel> models;
    Pre preprocessor{v_};
    Sort radix_sorter{v_};
    Ren renderer{v_};
    Post postprocessor{v_};
    ShCompression sh;
    Cov3dCompression cov3d;
    UVec2 size{1, 1};

    // MultiModelViewer::new_with(&device, format, depth_stencil, size): the target format has no meaning for a float (rgb,T)
    // framebuffer and is dropped; depth_stencil = Some(DepthStencilState { Depth32Float, depth_write_enabled: false, Less }) is
    // depth_test = GSX_DEPTH_LESS (scene.rs:1969-1980) — hand the frame's depth attachment over with update_depth_buffer.
    static MultiModelViewer new_with(int device, UVec2 size, ShCompression sh = ShCompression::Single,
                                     Cov3dCompression cov3d = Cov3dCompression::Single,
                                     gsx_depth_compare depth_test = GSX_DEPTH_ALWAYS) {
        MultiModelViewer v(device, size, sh, cov3d);
        v.set_depth_test(depth_test);
        return v;
    }
    void set_depth_test(gsx_depth_compare c) { check(gsx_viewer_set_depth_test(v_, c)); }
    // float32 [size.y][size.x] NDC depth, row 0 at the top: copied (host memory) or read in place (device memory, row pitch in bytes).
    // With frames_in_flight > 1 a depth-tested frame is dealt to a lane like any other and the lane takes its own snapshot: the
    // buffer is read as if on the viewer's stream at the render_frame that uses it — what is set or enqueued there afterwards
    // waits for that read (no host wait), not for the frame (gsx.h, the depth block)
    void update_depth_buffer(const float* host, UVec2 sz) { check(gsx_viewer_upload_depth_buffer(v_, host, sz.x, sz.y)); }
    void set_depth_buffer_device(const float* d_ptr, UVec2 sz, uint64_t row_pitch_bytes) {
        check(gsx_viewer_set_depth_buffer_device(v_, d_ptr, sz.x, sz.y, row_pitch_bytes));
    }
    // gsx_render_depth_map: walks the models in the order render_frame composites them (the LAST key first) with the viewer's current
    // camera and keeps per pixel ([size.y][size.x], row 0 at the top) the surface depth — the view depth of the first record after
    // whose blend T < threshold, +inf without one — that record's Gaussian index and layer (0xFFFFFFFF without), S = sum w * d,
    // A = sum w and the final T (the rendered frame's, bit for bit).  Every vector is optional.  The planes stay on the device
    // (depth_map_device_ptrs); with ndc = true an NDC depth plane is written as well, which set_depth_buffer_device takes as it is
    // (the writes are complete when the call returns).  The framebuffer keeps the last frame; every model named needs
    // preprocess() + sort() before the next render(); render_frame() needs nothing.
    struct DepthMapPlanes { void *surface, *sum, *alpha, *transmittance, *index, *layer, *ndc; UVec2 size; };
    gsx_depth_map_stats_t render_depth_map(const std::vector<std::string>& model_render_keys, float threshold = 0.5f, bool ndc = false,
                                           std::vector<float>* surface = nullptr, std::vector<float>* sum = nullptr, std::vector<float>* alpha = nullptr,
                                           std::vector<float>* transmittance = nullptr, std::vector<uint32_t>* index = nullptr,
                                           std::vector<uint32_t>* layer = nullptr) {
        std::vector<const char*> k;
        for (const auto& s : model_render_keys) k.push_back(s.c_str());
        const size_t npx = (size_t)size.x * size.y;
        for (auto* f : {surface, sum, alpha, transmittance})
            if (f) f->assign(npx, 0.0f);
        for (auto* u : {index, layer})
            if (u) u->assign(npx, 0xFFFFFFFFu);
        gsx_depth_map_desc desc{};
        gsx_depth_map_desc_default(&desc);
        desc.flags = ndc ? GSX_DEPTH_MAP_NDC : 0u;
        desc.threshold = threshold;
        gsx_depth_map_stats_t out{};
        check(gsx_render_depth_map(v_, k.data(), (uint32_t)k.size(), &desc, surface ? surface->data() : nullptr, sum ? sum->data() : nullptr,
                                   alpha ? alpha->data() : nullptr, transmittance ? transmittance->data() : nullptr, index ? index->data() : nullptr,
                                   layer ? layer->data() : nullptr, &out));
        return out;
    }
    // gsx_depth_map_device_ptrs: the last depth map's planes on the device (ndc: nullptr unless it was asked for), valid until the
    // next render_depth_map, a viewport change or the viewer's end
    DepthMapPlanes depth_map_device_ptrs() {
        DepthMapPlanes p{};
        check(gsx_depth_map_device_ptrs(v_, &p.surface, &p.sum, &p.alpha, &p.transmittance, &p.index, &p.layer, &p.ndc, &p.size.x, &p.size.y));
        return p;
    }
    // gsx_depth_map_unproject (host only): the world-space point seen at pixel position (px, py) at view depth view_depth
    static std::array<float, 3> depth_map_unproject(const float view[16], const float proj[16], UVec2 sz, float px, float py, float view_depth) {
        std::array<float, 3> w{};
        check(gsx_depth_map_unproject(view, proj, sz.x, sz.y, px, py, view_depth, w.data()));
        return w;
    }
    // MeasurementRenderer::update_hit_pairs (src/renderer/measurement.rs:133-167): the measurement lines, drawn by the library with depth
    // write before the splats of every frame from then on (gsx.h, the overlay block); an empty vector clears them
    void update_hit_pairs(const std::vector<gsx_overlay_line>& lines) {
        check(gsx_viewer_set_overlay_lines(v_, lines.empty() ? nullptr : lines.data(), (uint32_t)lines.size()));
    }
    // gs::MaskGizmo (src/tab/scene.rs:2211-2247, 2283-2293): the mask shapes' wireframes, drawn by the library before the measurement
    // lines with their depth state (gsx.h, the gizmo block): per render key the model's visible boxes, then its visible ellipsoids, in
    // world space; an empty vector clears them
    void set_mask_gizmos(const std::vector<gsx_mask_gizmo>& gizmos) {
        check(gsx_viewer_set_mask_gizmos(v_, gizmos.empty() ? nullptr : gizmos.data(), (uint32_t)gizmos.size()));
    }
    // last frame's overlay: premultiplied rgba [size.y][size.x][4] and the effective depth [size.y][size.x]; either may be null
    void download_overlay(float* rgba, float* depth) { check(gsx_download_overlay(v_, rgba, depth)); }
    MultiModelViewer(int device, UVec2 sz, ShCompression sh_, Cov3dCompression cov_) : sh(sh_), cov3d(cov_), size(sz) {
        gsx_viewer_desc d{GSX_ABI_VERSION, device, nullptr, sz.x, sz.y};
        check(gsx_viewer_create(&d, &v_));
    }
    MultiModelViewer(const MultiModelViewer&) = delete;
    MultiModelViewer(MultiModelViewer&& o) noexcept : v_(o.v_), models(std::move(o.models)), sh(o.sh), cov3d(o.cov3d), size(o.size) { o.v_ = nullptr; }
    ~MultiModelViewer() { if (v_) gsx_viewer_destroy(v_); }
    gsx_viewer* raw() { return v_; }

    MultiModelViewerModel& add_model(const std::string& key, size_t count) {  // new_empty + BindGroups::new + insert
        check(gsx_model_create(v_, key.c_str(), count, (gsx_sh_kind)sh, (gsx_cov3d_kind)cov3d));
        return models.emplace(key, MultiModelViewerModel{{GaussiansBuffer(v_, key), MaskBuffer(v_, key), SelectionBuffer(v_, key),
                                                            GaussiansEditBuffer(v_, key)}, v_, key}).first->second;
    }
    // gsx_model_extract: the Gaussians of `src_key` that pass `filter` (GSX_BOUNDS_* flags; flags: GSX_EXTRACT_INVERT, _DROP_EDITS) become
    // the new model `dst_key`, in their order, on the device, as stored bits.  Returns the number kept; 0 creates no model.
    // "Separate selection into a model": extract(k, a, GSX_BOUNDS_SELECTED), extract(k, b, GSX_BOUNDS_SELECTED, GSX_EXTRACT_INVERT).
    uint64_t extract(const std::string& src_key, const std::string& dst_key, uint32_t filter = 0, uint32_t flags = 0) {
        const gsx_extract_desc d{filter, flags};
        uint64_t count = 0;
        check(gsx_model_extract(v_, src_key.c_str(), dst_key.c_str(), &d, &count));
        if (count)
            models.emplace(dst_key, MultiModelViewerModel{{GaussiansBuffer(v_, dst_key), MaskBuffer(v_, dst_key), SelectionBuffer(v_, dst_key),
                                                           GaussiansEditBuffer(v_, dst_key)}, v_, dst_key});
        return count;
    }
    // gsx_model_decimate: the Gaussians of src_key that share a cell of a grid of edge desc.cell become one moment-matched Gaussian
    // of the new model dst_key, on the device (one-member cells are copied as stored bits).  map (nullable) receives the dst index
    // of every source Gaussian.  Returns the statistics; cells == 0 creates no model.
    gsx_decimate_stats_t decimate(const std::string& src_key, const std::string& dst_key, const gsx_decimate_desc& desc, std::vector<uint32_t>* map = nullptr) {
        if (map) {
            uint64_t n = 0;
            check(gsx_model_len(v_, src_key.c_str(), &n));
            map->assign((size_t)n, 0xFFFFFFFFu);
        }
        gsx_decimate_stats_t out{};
        check(gsx_model_decimate(v_, src_key.c_str(), dst_key.c_str(), &desc, map ? map->data() : nullptr, &out));
        if (out.cells)
            models.emplace(dst_key, MultiModelViewerModel{{GaussiansBuffer(v_, dst_key), MaskBuffer(v_, dst_key), SelectionBuffer(v_, dst_key),
                                                           GaussiansEditBuffer(v_, dst_key)}, v_, dst_key});
        return out;
    }
    // gsx_model_convert: extract into a model of the pod kind (sh, cov3d): position and colour word carried, covariance and SH
    // dequantised exactly and quantised once into the new kind, on the device.  The same kind is extract.  Returns the number kept; 0
    // creates no model.  Models of different kinds are merged by converting first.
    uint64_t convert(const std::string& src_key, const std::string& dst_key, ShCompression sh, Cov3dCompression cov3d, uint32_t filter = 0,
                     uint32_t flags = 0) {
        const gsx_convert_desc d{filter, flags, (uint32_t)sh, (uint32_t)cov3d};
        uint64_t count = 0;
        check(gsx_model_convert(v_, src_key.c_str(), dst_key.c_str(), &d, &count));
        if (count)
            models.emplace(dst_key, MultiModelViewerModel{{GaussiansBuffer(v_, dst_key), MaskBuffer(v_, dst_key), SelectionBuffer(v_, dst_key),
                                                           GaussiansEditBuffer(v_, dst_key)}, v_, dst_key});
        return count;
    }
    // gsx_model_merge: the Gaussians of the models `src_keys` that pass `filter` become the one new model `dst_key`, source after source,
    // each source's model transform baked into its Gaussians (an identity source travels as stored bits); dst has the identity transform.
    // Returns the total kept (0 creates no model); counts (optional) receives one kept count per source.
    uint64_t merge(const std::vector<std::string>& src_keys, const std::string& dst_key, uint32_t filter = 0, uint32_t flags = 0,
                   std::vector<uint64_t>* counts = nullptr) {
        const gsx_extract_desc d{filter, flags};
        std::vector<const char*> keys;
        for (const std::string& k : src_keys) keys.push_back(k.c_str());
        std::vector<uint64_t> per(src_keys.size() ? src_keys.size() : 1);
        uint64_t total = 0;
        check(gsx_model_merge(v_, keys.data(), (uint32_t)keys.size(), dst_key.c_str(), &d, per.data(), &total));
        if (total)
            models.emplace(dst_key, MultiModelViewerModel{{GaussiansBuffer(v_, dst_key), MaskBuffer(v_, dst_key), SelectionBuffer(v_, dst_key),
                                                           GaussiansEditBuffer(v_, dst_key)}, v_, dst_key});
        if (counts) counts->assign(per.begin(), per.begin() + src_keys.size());
        return total;
    }
    // gsx_model_export: the Gaussians of `key` that pass `filter` (flags: GSX_EXTRACT_INVERT, GSX_EXPORT_BAKE_EDITS) as gsx_gaussian
    // records in model space: rotation and scale solved from the stored covariance on the device, positions, colours and SH as stored.
    // The way out for a model that only the device holds (extract, merge); upload the records into a model of any pod kind.
    std::vector<gsx_gaussian> export_gaussians(const std::string& key, uint32_t filter = 0, uint32_t flags = 0, uint64_t staging_bytes = 0) {
        const gsx_export_desc d{filter, flags, GSX_EXPORT_GAUSSIANS, 0u, staging_bytes};
        uint64_t count = 0;
        check(gsx_model_export(v_, key.c_str(), &d, nullptr, 0, &count));
        std::vector<gsx_gaussian> out(count);
        if (count) check(gsx_model_export(v_, key.c_str(), &d, out.data(), count * sizeof(gsx_gaussian), &count));
        return out;
    }
    // gsx_model_export_ply: the same Gaussians as a binary INRIA PLY file (gsx_ply_write's header and rows).  The reference's
    // write_ply(edits, mask) is export_ply(key, GSX_BOUNDS_MASKED | GSX_BOUNDS_SKIP_HIDDEN, GSX_EXPORT_BAKE_EDITS).
    std::vector<uint8_t> export_ply(const std::string& key, uint32_t filter = 0, uint32_t flags = 0, uint64_t staging_bytes = 0) {
        const gsx_export_desc d{filter, flags, GSX_EXPORT_PLY_VERTICES, 0u, staging_bytes};
        uint64_t size = 0;
        check(gsx_model_export_ply(v_, key.c_str(), &d, nullptr, 0, &size));
        std::vector<uint8_t> out(size);
        check(gsx_model_export_ply(v_, key.c_str(), &d, out.data(), out.size(), &size));
        return out;
    }
    // gsx_model_import_ply: the app's load path read_ply_header -> read_ply_gaussians -> Gaussian::from -> update_range (app.rs:1053-1096)
    // in one call, the rows decoded on the device: a binary INRIA PLY file becomes the new model `key` of this viewer's pod kinds.
    // Returns the count; a file of 0 vertices creates no model.
    uint64_t import_ply(const std::string& key, const void* data, uint64_t size, uint64_t staging_bytes = 0) {
        const gsx_import_desc d{0u, 0u, staging_bytes};
        uint64_t count = 0;
        check(gsx_model_import_ply(v_, key.c_str(), data, size, (gsx_sh_kind)sh, (gsx_cov3d_kind)cov3d, &d, &count));
        if (count)
            models.emplace(key, MultiModelViewerModel{{GaussiansBuffer(v_, key), MaskBuffer(v_, key), SelectionBuffer(v_, key),
                                                       GaussiansEditBuffer(v_, key)}, v_, key});
        return count;
    }
    void remove_model(const std::string& key) {  // scene.rs:2176
        check(gsx_model_remove(v_, key.c_str()));
        models.erase(key);
    }
    void update_camera(const CameraTrait& camera, UVec2 sz) {  // scene.rs:795
        Mat4 v = camera.view(), p = camera.projection((float)sz.x / (float)sz.y);
        check(gsx_update_camera(v_, v.data(), p.data(), sz.x, sz.y));
        size = sz;
    }
    void update_model_transform(const std::string& key, Vec3 pos, Quat quat, Vec3 scale) {  // scene.rs:796-802
        check(gsx_update_model_transform(v_, key.c_str(), pos.data(), quat.data(), scale.data()));
    }
    void update_gaussian_transform(float sz, GaussianDisplayMode mode, GaussianShDegree sh_deg, bool no_sh0) {  // scene.rs:803-809
        check(gsx_update_gaussian_transform(v_, sz, (gsx_display_mode)mode, sh_deg.degree(), no_sh0 ? 1u : 0u));
    }
    void update_query(const gsx_query& pod) { check(gsx_update_query(v_, &pod)); }  // scene.rs:785
    void update_query_texture(const std::vector<uint8_t>& texels, UVec2 sz) {  // scene.rs:740, 791
        check(gsx_update_query_texture(v_, texels.data(), sz.x, sz.y));
    }
    void update_selection_highlight(std::array<float, 4> rgba) { check(gsx_update_selection_highlight(v_, rgba.data())); }  // scene.rs:816-829
    void update_selection_edit_with_pod(const GaussianEditPod& pod) { check(gsx_update_selection_edit(v_, &pod)); }   // scene.rs:815
    void show_unedited(const std::string& key, bool on) { check(gsx_model_show_unedited(v_, key.c_str(), on ? 1u : 0u)); }  // scene.rs:856-863
    std::vector<gsx_query_hit> download_query_hits(const std::string& key) {  // gs::query::download, scene.rs:651-657
        std::vector<gsx_query_hit> h(GSX_QUERY_MAX_HITS);
        uint64_t n = 0;
        check(gsx_query_download_hits(v_, key.c_str(), h.data(), h.size(), &n));
        h.resize((size_t)n);
        return h;
    }
    // QueryTextureOverlay / QueryCursor (scene.rs:2003-2014, 2317-2325): the colours the RGBA8 resolve draws the stroke and the cursor
    // with (straight alpha; alpha 0, the default, draws nothing); the query texture as the device holds it
    void set_toolset_overlay(std::array<float, 4> texture_rgba, std::array<float, 4> cursor_rgba, float cursor_thickness) {
        check(gsx_toolset_set_overlay(v_, texture_rgba.data(), cursor_rgba.data(), cursor_thickness));
    }
    std::vector<uint8_t> download_query_texture() {
        std::vector<uint8_t> t((size_t)size.x * size.y);
        check(gsx_download_query_texture(v_, t.data(), size.x, size.y));
        return t;
    }
    void poll() { check(gsx_sync(v_)); }  // device.poll(Maintain::Wait)
    std::vector<float> download_framebuffer() {
        std::vector<float> fb((size_t)size.x * size.y * 4);
        check(gsx_download_framebuffer(v_, fb.data(), fb.size()));
        return fb;
    }
    gsx_frame_stats frame_stats(const std::string& key) {
        gsx_frame_stats st{};
        check(gsx_model_frame_stats(v_, key.c_str(), &st));
        return st;
    }
};

enum class QueryToolsetTool : uint32_t { Rect = GSX_TOOL_RECT, Brush = GSX_TOOL_BRUSH };  // gs::QueryToolsetTool, scene.rs:1258-1264

// gs::QueryToolset (scene.rs:766-791) of a viewer, inside the library: start / update_pos queue what they paint, render() enqueues it on
// the viewer's stream as one launch — the query texture never crosses the host (gsx.h, the toolset block).  The viewer must outlive it.
class QueryToolset {
    gsx_viewer* v_;
public:
    struct State { QueryToolsetTool tool; gsx_selection_op op; std::array<float, 2> start, pos; };
    explicit QueryToolset(MultiModelViewer& viewer) : v_(viewer.raw()) {}
    void set_use_texture(bool on) { check(gsx_toolset_set_use_texture(v_, on ? 1u : 0u)); }
    void update_brush_radius(float r) { check(gsx_toolset_update_brush_radius(v_, r)); }
    void start(QueryToolsetTool tool, gsx_selection_op op, std::array<float, 2> pos) { check(gsx_toolset_start(v_, (uint32_t)tool, (uint32_t)op, pos.data())); }
    void update_pos(std::array<float, 2> pos) { check(gsx_toolset_update_pos(v_, pos.data())); }
    void end() { check(gsx_toolset_end(v_)); }
    gsx_query query() {  // query_toolset.query(): hand it to MultiModelViewer::update_query
        gsx_query q{};
        check(gsx_toolset_query(v_, &q));
        return q;
    }
    bool state(State* out) {  // query_toolset.state(): false = no tool in use
        uint32_t active = 0, tool = 0, op = 0;
        State s{};
        check(gsx_toolset_state(v_, &active, &tool, &op, s.start.data(), s.pos.data()));
        if (!active) return false;
        s.tool = (QueryToolsetTool)tool;
        s.op = (gsx_selection_op)op;
        if (out) *out = s;
        return true;
    }
    void render() { check(gsx_toolset_render(v_)); }  // query_toolset.render(queue, &mut encoder, &query_texture), scene.rs:791
};

}  // namespace gs
