//! gsx — the `gs::` facade over libgsx: the names and call shapes `LioQing/wgpu-3dgs-viewer-app` already uses for its
//! render path (`use wgpu_3dgs_viewer as gs;`), so that `src/tab/scene.rs` / `src/app.rs` change in imports only.
//!
//! NOT COMPILED IN THIS REPOSITORY (no Rust toolchain in the build image).  It mirrors, name for name, what is compiled and
//! tested here in two other host languages: `include/gsx.hpp` (C++ `gs::`, exercised by `tools/frame_driver.cpp`) and
//! `wgpu_3dgs_viewer_app_amd/viewer.py` (what the parity tests drive).  Every method cites the app call site it serves.
//!
//! What does NOT carry over: wgpu `Device` / `Queue` / `CommandEncoder` / bind groups.  libgsx enqueues on its own HIP stream;
//! the arguments stay in the signatures (ignored) so that call sites compile unchanged, and `device.poll(Maintain::Wait)`
//! becomes `viewer.poll()`.
use gsx_sys as sys;
use std::collections::HashMap;
use std::ffi::{CStr, CString};
use std::marker::PhantomData;

pub use sys::gsx_gaussian as Gaussian; // rot: Quat(xyzw), pos, color: U8Vec4, sh: [Vec3; 15], scale — field for field
pub use sys::gsx_gaussian_edit as GaussianEditPod;
pub use sys::gsx_query_hit as QueryHitResultPod;

/// `gs::Error` (app.rs:548, scene.rs:234): every non-zero status, with the library's thread-local message.
#[derive(Debug)]
pub enum Error {
    Io(String),
    Gsx { status: i32, message: String },
}
impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        match self {
            Error::Io(m) => write!(f, "io: {m}"),
            Error::Gsx { status, message } => write!(f, "gsx status {status}: {message}"),
        }
    }
}
fn check(status: sys::gsx_status) -> Result<(), Error> {
    if status == sys::GSX_OK {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(sys::gsx_last_error_string()) }.to_string_lossy().into_owned();
    Err(if status == sys::GSX_ERR_IO { Error::Io(message) } else { Error::Gsx { status, message } })
}

/// The pod generic `G: gs::GaussianPod` of the app's 8-way dispatch (scene.rs:23-81, app.rs:352-418) becomes two enums.
pub trait GaussianPod {
    const SH: sys::gsx_sh_kind;
    const COV3D: sys::gsx_cov3d_kind;
}
macro_rules! pod {
    ($name:ident, $sh:ident, $cov:ident) => {
        pub struct $name;
        impl GaussianPod for $name {
            const SH: sys::gsx_sh_kind = sys::gsx_sh_kind::$sh;
            const COV3D: sys::gsx_cov3d_kind = sys::gsx_cov3d_kind::$cov;
        }
    };
}
pod!(GaussianPodWithShSingleCov3dSingleConfigs, Single, Single);
pod!(GaussianPodWithShSingleCov3dHalfConfigs, Single, Half);
pod!(GaussianPodWithShHalfCov3dSingleConfigs, Half, Single);
pod!(GaussianPodWithShHalfCov3dHalfConfigs, Half, Half);
pod!(GaussianPodWithShNorm8Cov3dSingleConfigs, Norm8, Single);
pod!(GaussianPodWithShNorm8Cov3dHalfConfigs, Norm8, Half); // the app's default (app.rs:398-417)
pod!(GaussianPodWithShNoneCov3dSingleConfigs, None, Single);
pod!(GaussianPodWithShNoneCov3dHalfConfigs, None, Half);

#[derive(Clone, Copy, PartialEq, Eq)]
pub enum GaussianDisplayMode { Splat = 0, Ellipse = 1, Point = 2 }
/// `GaussianShDegree::new` returns `None` above 3 (transform.rs:139).
#[derive(Clone, Copy)]
pub struct GaussianShDegree(u32);
impl GaussianShDegree {
    pub fn new(deg: u32) -> Option<Self> { (deg <= 3).then_some(Self(deg)) }
    pub fn degree(&self) -> u32 { self.0 }
}

/// What crosses the ABI of a camera: its two matrices (`CameraTrait`, app.rs:1236-1244, 1329-1343; glam column-major).
pub trait CameraTrait {
    fn view(&self) -> [f32; 16];
    fn projection(&self, aspect_ratio: f32) -> [f32; 16];
}

struct Handle(*mut sys::gsx_viewer);
impl Drop for Handle {
    fn drop(&mut self) { unsafe { sys::gsx_viewer_destroy(self.0) } }
}

/// `gs::GaussiansBuffer<G>`: `update_range(&queue, start, &[Gaussian])` (scene.rs:2083-2084), `len()` (scene.rs:608, 862).
pub struct GaussiansBuffer { v: *mut sys::gsx_viewer, key: CString }
impl GaussiansBuffer {
    pub fn update_range<Q>(&self, _queue: &Q, start: usize, gaussians: &[Gaussian]) {
        check(unsafe { sys::gsx_model_upload_range(self.v, self.key.as_ptr(), start as u64, gaussians.as_ptr(), gaussians.len() as u64) })
            .expect("update_range"); // infallible in the crate's signature: panics like the reference (scene.rs:2078-2081)
    }
    /// `gsx_model_upload_ply_rows`: binary PLY vertex rows (`header.vertex_bytes` each) decoded on the device into the Gaussians from
    /// `start` on: `update_range` of the rows' Gaussians without the records in between (spec section 15).
    pub fn update_range_ply<Q>(&self, _queue: &Q, start: usize, rows: &[u8], header: &sys::gsx_ply_header) -> Result<(), Error> {
        let desc = sys::gsx_import_desc { flags: 0, reserved: 0, staging_bytes: 0 };
        let n = if header.vertex_bytes > 0 { rows.len() as u64 / header.vertex_bytes as u64 } else { 0 };
        check(unsafe { sys::gsx_model_upload_ply_rows(self.v, self.key.as_ptr(), start as u64, rows.as_ptr() as *const std::os::raw::c_void, n, header, &desc) })
    }
    pub fn len(&self) -> usize {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) }).expect("len");
        n as usize
    }
}
/// What `buffer.clone()` gives in the app (app.rs:769-780: the clones are moved into spawned download threads): a handle on a
/// device-side snapshot of the buffer taken at clone time.  `Clone` adds a reference, `Drop` releases it, `download` may run on
/// any thread while the viewer renders (`gsx_buffer_*` in include/gsx.h).
pub struct BufferClone<T> { h: *mut sys::gsx_buffer, _t: std::marker::PhantomData<T> }
unsafe impl<T: Send> Send for BufferClone<T> {}
impl<T> Clone for BufferClone<T> {
    fn clone(&self) -> Self { unsafe { sys::gsx_buffer_retain(self.h) }; Self { h: self.h, _t: std::marker::PhantomData } }
}
impl<T> Drop for BufferClone<T> { fn drop(&mut self) { unsafe { sys::gsx_buffer_release(self.h) } } }
impl<T: Copy> BufferClone<T> {
    fn retain(v: *mut sys::gsx_viewer, key: &CString, kind: sys::gsx_buffer_kind) -> Result<Self, Error> {
        let mut h = std::ptr::null_mut();
        check(unsafe { sys::gsx_model_buffer_retain(v, key.as_ptr(), kind, &mut h) })?;
        Ok(Self { h, _t: std::marker::PhantomData })
    }
    pub async fn download<D, Q>(&self, _device: &D, _queue: &Q) -> Result<Vec<T>, Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_buffer_len(self.h, &mut n) })?;
        let mut out: Vec<T> = Vec::with_capacity(n as usize);
        check(unsafe { sys::gsx_buffer_download(self.h, out.as_mut_ptr() as *mut std::os::raw::c_void, n) })?;
        unsafe { out.set_len(n as usize) };
        Ok(out)
    }
}
/// `gs::MaskBuffer` / `gs::SelectionBuffer` / `gs::GaussiansEditBuffer`: `download::<T>(&device, &queue).await` (app.rs:789, 806).
pub struct MaskBuffer { v: *mut sys::gsx_viewer, key: CString, words: usize }
impl MaskBuffer {
    pub async fn download<D, Q>(&self, _device: &D, _queue: &Q) -> Result<Vec<u32>, Error> {
        let mut w = vec![0u32; self.words];
        check(unsafe { sys::gsx_model_download_mask(self.v, self.key.as_ptr(), w.as_mut_ptr(), w.len() as u64) })?;
        Ok(w)
    }
    /// `mask_buffer.clone()` (app.rs:775)
    pub fn clone_handle(&self) -> Result<BufferClone<u32>, Error> { BufferClone::retain(self.v, &self.key, sys::gsx_buffer_kind::Mask) }
}
pub struct GaussiansEditBuffer { v: *mut sys::gsx_viewer, key: CString, n: usize }
impl GaussiansEditBuffer {
    pub async fn download<D, Q>(&self, _device: &D, _queue: &Q) -> Result<Vec<GaussianEditPod>, Error> {
        let mut e = Vec::with_capacity(self.n);
        check(unsafe { sys::gsx_model_download_edits(self.v, self.key.as_ptr(), e.as_mut_ptr(), self.n as u64) })?;
        unsafe { e.set_len(self.n) };
        Ok(e)
    }
    /// `gaussians_edit_buffer.clone()` (app.rs:772)
    pub fn clone_handle(&self) -> Result<BufferClone<GaussianEditPod>, Error> { BufferClone::retain(self.v, &self.key, sys::gsx_buffer_kind::Edits) }
}
/// `gs::MultiModelViewerGaussianBuffers<G>::new_empty(&device, count)` (scene.rs:2111-2112)
pub struct MultiModelViewerGaussianBuffers {
    pub gaussians_buffer: GaussiansBuffer,
    pub mask_buffer: MaskBuffer,
    pub gaussians_edit_buffer: GaussiansEditBuffer,
}
/// `gs::MultiModelViewerModel { gaussian_buffers, bind_groups }` (scene.rs:2133-2139); bind groups have no counterpart.
pub struct MultiModelViewerModel { pub gaussian_buffers: MultiModelViewerGaussianBuffers, v: *mut sys::gsx_viewer, key: CString }
/// The result of `MultiModelViewerModel::bounds`: `center` is `GaussianSplattingModel::center` (app.rs:1019-1046).
pub type ModelBounds = sys::gsx_model_bounds_t;
impl MultiModelViewerModel {
    /// `gsx_model_bounds`: box, centre, centroid and trimmed box of the model's Gaussian centres, in model space, computed on the
    /// device.  `filter`: `sys::GSX_BOUNDS_*` flags; `trim_permille` < 500.  After the last `update_range` of a load:
    /// `model.center = viewer.models[key].bounds(0, 0)?.center.into()` (the reference leaves it `Vec3::ZERO`).
    pub fn bounds(&self, filter: u32, trim_permille: u32) -> Result<ModelBounds, Error> {
        let desc = sys::gsx_bounds_desc { filter, trim_permille };
        let mut out = ModelBounds::default();
        check(unsafe { sys::gsx_model_bounds(self.v, self.key.as_ptr(), &desc, &mut out) })?;
        Ok(out)
    }
    /// `gsx_model_pod_kind`: the kinds this model's planes are stored in (after `convert` a viewer holds models of several kinds).
    pub fn pod_kind(&self) -> Result<(sys::gsx_sh_kind, sys::gsx_cov3d_kind), Error> {
        let (mut sh, mut cov3d) = (sys::gsx_sh_kind::Single, sys::gsx_cov3d_kind::Single);
        check(unsafe { sys::gsx_model_pod_kind(self.v, self.key.as_ptr(), &mut sh, &mut cov3d) })?;
        Ok((sh, cov3d))
    }
    /// `gsx_model_set_pod_kind`: the Compression Settings menu (app.rs:152-177) applied to this loaded model: same key, length,
    /// transform, mask, selection and edits; the planes requantised on the device; the next frame unspeculated.  The same kind does
    /// nothing.
    pub fn set_pod_kind(&mut self, sh: sys::gsx_sh_kind, cov3d: sys::gsx_cov3d_kind) -> Result<(), Error> {
        check(unsafe { sys::gsx_model_set_pod_kind(self.v, self.key.as_ptr(), sh, cov3d) })
    }
    /// `gsx_model_apply_transform`: the Gaussians that pass `desc.filter` (`desc.flags` `GSX_EXTRACT_INVERT`: those that do not) are
    /// moved, rotated, scaled or mirrored about `desc.pivot` where they lie, on the device: positions, covariances, SH and shade
    /// records as `merge` bakes a model transform; order, mask, selection and edits stay.  "Rotate the selection about its centre":
    /// `pivot = bounds(GSX_BOUNDS_SELECTED, 0)?.center`.  Returns the number of Gaussians moved.
    pub fn apply_transform(&mut self, desc: &sys::gsx_transform_desc) -> Result<u64, Error> {
        let mut count = 0u64;
        check(unsafe { sys::gsx_model_apply_transform(self.v, self.key.as_ptr(), desc, &mut count) })?;
        Ok(count)
    }
    /// `gsx_model_visibility`: draws this model ALONE with the viewer's current camera and keeps, per Gaussian and on the device, the
    /// peak blending weight `T * alpha`, the summed weight (2^-24 fixed point, as `f64`) and the pixel count; `accumulate` folds the
    /// view into the planes an earlier call left.  Returns `(peak, weight, pixels, stats)` (the three empty without `rows`).  The
    /// model goes through `preprocess` + `sort` again before the next `render`; `render_frame` needs nothing.
    pub fn visibility(&mut self, accumulate: bool, rows: bool) -> Result<(Vec<f32>, Vec<f64>, Vec<u32>, sys::gsx_visibility_stats_t), Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let len = if rows { n as usize } else { 0 };
        let (mut peak, mut weight, mut pixels) = (vec![0f32; len], vec![0f64; len], vec![0u32; len]);
        let desc = sys::gsx_visibility_desc { flags: if accumulate { sys::GSX_VIS_ACCUMULATE } else { 0 }, reserved: [0; 3] };
        let mut out = sys::gsx_visibility_stats_t::default();
        let (p, w, c) = if rows { (peak.as_mut_ptr(), weight.as_mut_ptr(), pixels.as_mut_ptr()) } else { (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()) };
        check(unsafe { sys::gsx_model_visibility(self.v, self.key.as_ptr(), &desc, p, w, c, std::ptr::null_mut(), &mut out) })?;
        Ok((peak, weight, pixels, out))
    }
    /// `gsx_model_select_visibility`: selects the Gaussians that pass `desc.filter` and whose resident measure lies in `[lo, hi]`;
    /// "never seen" is `GSX_VIS_PEAK` in `[0, 0]`.  Returns `(hit, selected)`.
    pub fn select_visibility(&mut self, desc: &sys::gsx_visibility_select_desc) -> Result<(u64, u64), Error> {
        let (mut hit, mut selected) = (0u64, 0u64);
        check(unsafe { sys::gsx_model_select_visibility(self.v, self.key.as_ptr(), desc, &mut hit, &mut selected) })?;
        Ok((hit, selected))
    }
    /// `gsx_model_visibility_reset`: frees the resident planes.
    pub fn visibility_reset(&mut self) -> Result<(), Error> {
        check(unsafe { sys::gsx_model_visibility_reset(self.v, self.key.as_ptr()) })
    }
    /// Resets the planes, then folds one view per camera (`(view, proj)`, 16 column-major floats each): every Gaussian's best and
    /// summed contribution over an orbit.  The viewer keeps the last camera.  Returns the last view's result.
    pub fn visibility_orbit(&mut self, cameras: &[([f32; 16], [f32; 16])], size: (u32, u32), rows: bool) -> Result<(Vec<f32>, Vec<f64>, Vec<u32>, sys::gsx_visibility_stats_t), Error> {
        self.visibility_reset()?;
        let mut out = (Vec::new(), Vec::new(), Vec::new(), sys::gsx_visibility_stats_t::default());
        for (k, (view, proj)) in cameras.iter().enumerate() {
            check(unsafe { sys::gsx_update_camera(self.v, view.as_ptr(), proj.as_ptr(), size.0, size.1) })?;
            out = self.visibility(true, rows && k + 1 == cameras.len())?;
        }
        Ok(out)
    }
    /// `gsx_model_decimate` without a destination: how a grid of edge `desc.cell` would divide the model.  Returns the statistics
    /// and the cell every Gaussian would go into (`0xFFFF_FFFF`: it does not participate).  Nothing is created.
    pub fn decimate_count(&self, desc: &sys::gsx_decimate_desc) -> Result<(sys::gsx_decimate_stats_t, Vec<u32>), Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let mut map = vec![u32::MAX; n as usize];
        let mut out = sys::gsx_decimate_stats_t::default();
        check(unsafe { sys::gsx_model_decimate(self.v, self.key.as_ptr(), std::ptr::null(), desc, map.as_mut_ptr(), &mut out) })?;
        Ok((out, map))
    }
    /// `gsx_model_decimate_edge`: the smallest probed cell edge that leaves at most `target_cells` cells, by count-only bisection on
    /// the device.  Returns `(edge, cells)`.
    pub fn decimate_edge(&self, target_cells: u64, filter: u32, flags: u32) -> Result<(f32, u64), Error> {
        let (mut cell, mut cells) = (0f32, 0u64);
        check(unsafe { sys::gsx_model_decimate_edge(self.v, self.key.as_ptr(), filter, flags, target_cells, &mut cell, &mut cells) })?;
        Ok((cell, cells))
    }
    /// `gsx_model_property_values`: one `f32` per Gaussian, computed on the device from the stored values (edits are not applied):
    /// the stored position (`flags = GSX_PROP_WORLD`: the model transform applied as `merge` bakes it), the bytes of the colour word
    /// / 255, their HSV, or the scales `export` solves from the covariance.
    pub fn property_values(&self, property: sys::gsx_property, flags: u32) -> Result<Vec<f32>, Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let mut out = vec![0f32; n as usize];
        check(unsafe { sys::gsx_model_property_values(self.v, self.key.as_ptr(), property as u32, flags, out.as_mut_ptr(), n) })?;
        Ok(out)
    }
    /// `gsx_model_histogram`: `desc.bins` equal bins of the property over `[lo, hi]` (`GSX_HIST_AUTO_RANGE`: over `[min, max]`,
    /// returned in the result's `lo` / `hi`) among the Gaussians that pass `desc.filter` and have a finite value.
    pub fn histogram(&self, desc: &sys::gsx_histogram_desc) -> Result<(sys::gsx_histogram_t, Vec<u64>), Error> {
        let mut bins = vec![0u64; desc.bins.max(1) as usize];
        let mut out = sys::gsx_histogram_t::default();
        check(unsafe { sys::gsx_model_histogram(self.v, self.key.as_ptr(), desc, bins.as_mut_ptr(), &mut out) })?;
        Ok((out, bins))
    }
    /// `gsx_model_select_range`: the Gaussians that pass `desc.filter`, have a finite value in `[lo, hi]` and (`desc.bins > 0`) a bin
    /// in `[bin_lo, bin_hi]` are the hit set; `desc.selection_op` sets, adds or removes it, on the device.  Returns `(hit, selected)`.
    pub fn select_range(&mut self, desc: &sys::gsx_select_desc) -> Result<(u64, u64), Error> {
        let (mut hit, mut selected) = (0u64, 0u64);
        check(unsafe { sys::gsx_model_select_range(self.v, self.key.as_ptr(), desc, &mut hit, &mut selected) })?;
        Ok((hit, selected))
    }
    /// `gsx_model_neighbors`: for every Gaussian, how many others lie within `desc.radius` of it in model space (`d2 <= r2` in `f32`),
    /// saturated at `desc.max_count`, among the Gaussians that pass `desc.filter` and have a finite position; computed on the device
    /// with a hashed grid.  Returns `(counts, hist, stats)`: `hist[c]` is the number of participants with count `c`.
    pub fn neighbors(&self, desc: &sys::gsx_neighbor_desc) -> Result<(Vec<u32>, Vec<u64>, sys::gsx_neighbor_stats_t), Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let mut counts = vec![0u32; n as usize];
        let mut hist = vec![0u64; desc.max_count.min(sys::GSX_NEIGHBOR_MAX_COUNT) as usize + 1];
        let mut out = sys::gsx_neighbor_stats_t::default();
        check(unsafe { sys::gsx_model_neighbors(self.v, self.key.as_ptr(), desc, counts.as_mut_ptr(), hist.as_mut_ptr(), &mut out) })?;
        Ok((counts, hist, out))
    }
    /// `gsx_model_select_neighbors`: the participants whose saturated count lies in `[count_lo, count_hi]` are the hit set;
    /// `desc.selection_op` sets, adds or removes it, on the device.  Floaters with fewer than `k` neighbours: `max_count = k`,
    /// `[0, k - 1]`.  Returns `(hit, selected)`.
    pub fn select_neighbors(&mut self, desc: &sys::gsx_neighbor_select_desc) -> Result<(u64, u64), Error> {
        let (mut hit, mut selected) = (0u64, 0u64);
        check(unsafe { sys::gsx_model_select_neighbors(self.v, self.key.as_ptr(), desc, &mut hit, &mut selected) })?;
        Ok((hit, selected))
    }
    /// `gsx_model_clusters`: the connected pieces of the model under "within `desc.radius` of one another" (`d2 <= r2` in `f32`, model
    /// space), among the Gaussians that pass `desc.filter` and have a finite position; computed on the device by a union-find over a
    /// hashed grid.  Returns `(labels, sizes, stats)`: `labels[i]` is the smallest Gaussian index of `i`'s cluster
    /// (`GSX_CLUSTER_NONE` for one that does not participate), `sizes[i]` the size of its cluster.
    pub fn clusters(&self, desc: &sys::gsx_cluster_desc) -> Result<(Vec<u32>, Vec<u32>, sys::gsx_cluster_stats_t), Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let mut labels = vec![sys::GSX_CLUSTER_NONE; n as usize];
        let mut sizes = vec![0u32; n as usize];
        let mut out = sys::gsx_cluster_stats_t::default();
        check(unsafe { sys::gsx_model_clusters(self.v, self.key.as_ptr(), desc, labels.as_mut_ptr(), sizes.as_mut_ptr(), &mut out) })?;
        Ok((labels, sizes, out))
    }
    /// `gsx_model_select_clusters`: the hit set is, by `desc.mode`, the clusters with a size in `[size_lo, size_hi]`, the largest
    /// cluster, or the clusters that hold a selected Gaussian; `desc.selection_op` sets, adds or removes it, on the device.  Returns
    /// `(hit, selected)`.
    pub fn select_clusters(&mut self, desc: &sys::gsx_cluster_select_desc) -> Result<(u64, u64), Error> {
        let (mut hit, mut selected) = (0u64, 0u64);
        check(unsafe { sys::gsx_model_select_clusters(self.v, self.key.as_ptr(), desc, &mut hit, &mut selected) })?;
        Ok((hit, selected))
    }
    /// `gsx_model_knn`: every Gaussian's `desc.k` smallest squared distances to the others (`f32`, model space), a score from them
    /// (`GSX_KNN_SCORE_*`) and the score's statistics, among the Gaussians that pass `desc.filter` and have a finite position; computed
    /// on the device, bit for bit the brute-force answer.  Returns `(d2, score, stats)`: `d2` holds `n * k` values, row `i` at `i * k`
    /// (empty without `rows`), `score` one value a Gaussian; both `+inf` for a Gaussian that does not participate.
    pub fn knn(&self, desc: &sys::gsx_knn_desc, rows: bool) -> Result<(Vec<f32>, Vec<f32>, sys::gsx_knn_stats_t), Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let mut d2 = vec![f32::INFINITY; if rows { n as usize * desc.k as usize } else { 0 }];
        let mut score = vec![f32::INFINITY; n as usize];
        let mut out = sys::gsx_knn_stats_t::default();
        let d2_ptr = if rows { d2.as_mut_ptr() } else { std::ptr::null_mut() };
        check(unsafe { sys::gsx_model_knn(self.v, self.key.as_ptr(), desc, d2_ptr, score.as_mut_ptr(), &mut out) })?;
        Ok((d2, score, out))
    }
    /// `gsx_model_select_knn`: the hit set is, by `desc.mode`, the participants with a score in `[lo, hi]` or the statistical outliers
    /// (score above mean + `std_ratio` * std); `desc.selection_op` sets, adds or removes it, on the device.  Returns
    /// `(hit, selected, stats)`.
    pub fn select_knn(&mut self, desc: &sys::gsx_knn_select_desc) -> Result<(u64, u64, sys::gsx_knn_stats_t), Error> {
        let (mut hit, mut selected) = (0u64, 0u64);
        let mut out = sys::gsx_knn_stats_t::default();
        check(unsafe { sys::gsx_model_select_knn(self.v, self.key.as_ptr(), desc, &mut hit, &mut selected, &mut out) })?;
        Ok((hit, selected, out))
    }
    /// `gsx_model_normals`: a plane fitted in double to every Gaussian and its `desc.k` nearest (by squared distance, then index), among
    /// the Gaussians that pass `desc.filter` and have a finite position, on the device.  Returns `(normal, variation, index, stats)`:
    /// `normal` holds `n * 3` values (`0, 0, 0` where none is fitted), `variation` one a Gaussian (`+inf` there), `index` `n * k` words,
    /// row `i` at `i * k` (empty without `indices`), `GSX_NORMALS_NONE` where there is no such neighbour.
    #[allow(clippy::type_complexity)]
    pub fn normals(&self, desc: &sys::gsx_normals_desc, indices: bool) -> Result<(Vec<f32>, Vec<f32>, Vec<u32>, sys::gsx_normals_stats_t), Error> {
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let mut normal = vec![0f32; n as usize * 3];
        let mut variation = vec![f32::INFINITY; n as usize];
        let mut index = vec![sys::GSX_NORMALS_NONE; if indices { n as usize * desc.k as usize } else { 0 }];
        let mut out = sys::gsx_normals_stats_t::default();
        let index_ptr = if indices { index.as_mut_ptr() } else { std::ptr::null_mut() };
        check(unsafe { sys::gsx_model_normals(self.v, self.key.as_ptr(), desc, normal.as_mut_ptr(), variation.as_mut_ptr(), index_ptr, &mut out) })?;
        Ok((normal, variation, index, out))
    }
    /// `gsx_model_select_normals`: the hit set is, by `desc.mode`, the fitted Gaussians with a variation in `[lo, hi]` or with a cosine
    /// between their normal and `desc.dir` in `[lo, hi]`; `desc.selection_op` sets, adds or removes it, on the device.  Returns
    /// `(hit, selected, stats)`.
    pub fn select_normals(&mut self, desc: &sys::gsx_normals_select_desc) -> Result<(u64, u64, sys::gsx_normals_stats_t), Error> {
        let (mut hit, mut selected) = (0u64, 0u64);
        let mut out = sys::gsx_normals_stats_t::default();
        check(unsafe { sys::gsx_model_select_normals(self.v, self.key.as_ptr(), desc, &mut hit, &mut selected, &mut out) })?;
        Ok((hit, selected, out))
    }
    /// `gsx_model_nearest`: for every Gaussian of this model, mapped by `desc.xform` (or by the two models' transforms), the nearest
    /// Gaussian of the model `dst_key`, on the device, bit for bit the brute-force answer with ties going to the smaller index.
    /// Returns `(index, d2, stats)`: `GSX_NEAREST_NONE` and `+inf` where there is none (both empty without `rows`); the stats carry
    /// the one-sided chamfer (`mean`) and Hausdorff (`d_max`) distances and the matrix used.
    pub fn nearest(&self, dst_key: &str, desc: &sys::gsx_nearest_desc, rows: bool) -> Result<(Vec<u32>, Vec<f32>, sys::gsx_nearest_stats_t), Error> {
        let dst = CString::new(dst_key).unwrap();
        let mut n = 0u64;
        check(unsafe { sys::gsx_model_len(self.v, self.key.as_ptr(), &mut n) })?;
        let mut index = vec![sys::GSX_NEAREST_NONE; if rows { n as usize } else { 0 }];
        let mut d2 = vec![f32::INFINITY; if rows { n as usize } else { 0 }];
        let mut out = sys::gsx_nearest_stats_t::default();
        let (index_ptr, d2_ptr) = if rows { (index.as_mut_ptr(), d2.as_mut_ptr()) } else { (std::ptr::null_mut(), std::ptr::null_mut()) };
        check(unsafe { sys::gsx_model_nearest(self.v, self.key.as_ptr(), dst.as_ptr(), desc, index_ptr, d2_ptr, &mut out) })?;
        Ok((index, d2, out))
    }
    /// `gsx_model_select_nearest`: writes THIS model's selection; the hit set is, by `desc.mode`, the Gaussians whose distance to the
    /// model `dst_key` lies in `[lo, hi]` or those whose nearest target is selected there.  Returns `(hit, selected, stats)`.
    pub fn select_nearest(&mut self, dst_key: &str, desc: &sys::gsx_nearest_select_desc) -> Result<(u64, u64, sys::gsx_nearest_stats_t), Error> {
        let dst = CString::new(dst_key).unwrap();
        let (mut hit, mut selected) = (0u64, 0u64);
        let mut out = sys::gsx_nearest_stats_t::default();
        check(unsafe { sys::gsx_model_select_nearest(self.v, self.key.as_ptr(), dst.as_ptr(), desc, &mut hit, &mut selected, &mut out) })?;
        Ok((hit, selected, out))
    }
    /// `gsx_model_align_step`: one least-squares step of point-to-point registration of this model onto the model `dst_key`.
    pub fn align_step(&self, dst_key: &str, desc: &sys::gsx_align_desc) -> Result<sys::gsx_align_step_t, Error> {
        let dst = CString::new(dst_key).unwrap();
        let mut out = sys::gsx_align_step_t::default();
        check(unsafe { sys::gsx_model_align_step(self.v, self.key.as_ptr(), dst.as_ptr(), desc, &mut out) })?;
        Ok(out)
    }
    /// Iterative closest point: `align_step` until `rms_before` changes by less than `tol` relatively or does not fall any more (at
    /// the float32 rounding of the positions it only flickers: a rise is the end), a step is degenerate or `max_iters` steps ran; every step starts from the step before's `xform_next`.  Returns the last step (its `nearest.xform` is
    /// the final matrix) and the composed similarity `D` (row-major 3x4, `f64`) with `final = D o initial`.
    pub fn align(&self, dst_key: &str, desc: &sys::gsx_align_desc, max_iters: u32, tol: f64) -> Result<(sys::gsx_align_step_t, [f64; 12]), Error> {
        let mut desc = *desc;
        let mut d = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0f64];
        let mut out = sys::gsx_align_step_t::default();
        let mut last = -1.0f64;
        for _ in 0..max_iters {
            out = self.align_step(dst_key, &desc)?;
            let now = out.rms_before;
            if out.degenerate != 0 || (last >= 0.0 && (now >= last || last - now <= tol * last)) { break; }
            last = now;
            let (x, y, z, w, s) = (out.quat[0], out.quat[1], out.quat[2], out.quat[3], out.scale);
            let r = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y), 2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z),
                     2.0 * (y * z - w * x), 2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)];
            let mut next = [0.0f64; 12];
            for row in 0..3 {
                for c in 0..4 {
                    next[4 * row + c] = s * (r[3 * row] * d[c] + r[3 * row + 1] * d[4 + c] + r[3 * row + 2] * d[8 + c]) + if c == 3 { out.pos[row] } else { 0.0 };
                }
            }
            d = next;
            desc.nearest.flags &= !sys::GSX_NEAREST_MODEL_TRANSFORMS; // from the second step on the matrix is the step before's
            desc.nearest.xform = out.xform_next;
        }
        Ok((out, d))
    }
    /// `gsx_model_normals_keep`: `normals` whose normals and variations stay on the device with the model (16 bytes a Gaussian), for
    /// `align_plane_step`; a second keep replaces the first.  An upload, an import, a transform and a pod kind change drop the plane.
    pub fn keep_normals(&mut self, desc: &sys::gsx_normals_desc) -> Result<sys::gsx_normals_stats_t, Error> {
        let mut out = sys::gsx_normals_stats_t::default();
        check(unsafe { sys::gsx_model_normals_keep(self.v, self.key.as_ptr(), desc, &mut out) })?;
        Ok(out)
    }
    /// `gsx_model_normals_kept`: whether a plane is resident and what it was made with and, with `rows`, its contents: `n * 3` normals
    /// and `n` variations (both empty without a plane).
    pub fn kept_normals(&self, rows: bool) -> Result<(sys::gsx_normals_kept_t, Vec<f32>, Vec<f32>), Error> {
        let mut out = sys::gsx_normals_kept_t::default();
        check(unsafe { sys::gsx_model_normals_kept(self.v, self.key.as_ptr(), &mut out, std::ptr::null_mut(), std::ptr::null_mut()) })?;
        if out.present == 0 || !rows { return Ok((out, Vec::new(), Vec::new())); }
        let n = out.count as usize;
        let (mut normal, mut variation) = (vec![0.0f32; n * 3], vec![f32::INFINITY; n]);
        check(unsafe { sys::gsx_model_normals_kept(self.v, self.key.as_ptr(), &mut out, normal.as_mut_ptr(), variation.as_mut_ptr()) })?;
        Ok((out, normal, variation))
    }
    /// `gsx_model_normals_reset`: frees the kept plane.
    pub fn reset_normals(&mut self) -> Result<(), Error> { check(unsafe { sys::gsx_model_normals_reset(self.v, self.key.as_ptr()) }) }
    /// `gsx_model_align_plane_step`: one Gauss-Newton step of point-to-plane registration of this model onto the model `dst_key`, which
    /// needs `keep_normals` first.  The step moves only along what the pairs determine (`rank` of the six motions).
    pub fn align_plane_step(&self, dst_key: &str, desc: &sys::gsx_align_plane_desc) -> Result<sys::gsx_align_plane_step_t, Error> {
        let dst = CString::new(dst_key).unwrap();
        let mut out = sys::gsx_align_plane_step_t::default();
        check(unsafe { sys::gsx_model_align_plane_step(self.v, self.key.as_ptr(), dst.as_ptr(), desc, &mut out) })?;
        Ok(out)
    }
    /// `gsx_plane_fit_desc_default`: triples, 256 candidates, seed 0, tolerance 0, two refine rounds.
    pub fn plane_fit_desc() -> sys::gsx_plane_fit_desc {
        let mut d = sys::gsx_plane_fit_desc::default();
        unsafe { sys::gsx_plane_fit_desc_default(&mut d) };
        d
    }
    /// `gsx_plane_select_desc_default`: the plane z = 0, lo = hi = 0, `GSX_SELECTION_SET`.
    pub fn plane_select_desc() -> sys::gsx_plane_select_desc {
        let mut d = sys::gsx_plane_select_desc::default();
        unsafe { sys::gsx_plane_select_desc_default(&mut d) };
        d
    }
    /// `gsx_model_fit_plane`: the model's dominant plane by consensus, on the device: `desc.n_candidates` planes (sampled from triples,
    /// from kept normals, or the caller's `candidates`, used as given), every participant tested against every plane, the winner
    /// refined by least squares.  With `rows`, every candidate and its exact inlier count come back too.  Level a capture:
    /// `plane_level(&fit.plane, up)`, then `update_model_transform`.  Remove the floor: `select_plane` with `lo = -inf`, `hi =
    /// tolerance`, then `extract` with `GSX_BOUNDS_SELECTED` and `GSX_EXTRACT_INVERT`.  Peel the next plane: `select_plane` with
    /// `GSX_SELECTION_ADD`, then fit again with filter `GSX_BOUNDS_SELECTED` and flags `GSX_EXTRACT_INVERT`.
    pub fn fit_plane(&self, desc: &sys::gsx_plane_fit_desc, candidates: Option<&[sys::gsx_plane_t]>, rows: bool)
                     -> Result<(sys::gsx_plane_fit_t, Vec<sys::gsx_plane_t>, Vec<u32>), Error> {
        if let Some(c) = candidates { assert!(c.len() >= desc.n_candidates as usize, "fit_plane: fewer candidates than desc.n_candidates"); }
        let n = if rows && desc.n_candidates <= sys::GSX_PLANE_MAX_CANDIDATES { desc.n_candidates as usize } else { 0 };
        let (mut planes, mut counts) = (vec![sys::gsx_plane_t::default(); n], vec![0u32; n]);
        let mut out = sys::gsx_plane_fit_t::default();
        check(unsafe {
            sys::gsx_model_fit_plane(self.v, self.key.as_ptr(), desc, candidates.map_or(std::ptr::null(), |c| c.as_ptr()),
                                     if n > 0 { planes.as_mut_ptr() } else { std::ptr::null_mut() }, if n > 0 { counts.as_mut_ptr() } else { std::ptr::null_mut() }, &mut out)
        })?;
        Ok((out, planes, counts))
    }
    /// `gsx_model_select_plane`: the participants whose signed residual against `desc.plane` lies in `[lo, hi]` (a bound may be
    /// infinite) and, with `min_cos > 0`, whose kept normal is within that cosine of the plane's; `desc.selection_op` sets, adds or
    /// removes the hit set, on the device.  Returns `(hit, selected afterwards)`.
    pub fn select_plane(&mut self, desc: &sys::gsx_plane_select_desc) -> Result<(u64, u64), Error> {
        let (mut hit, mut selected) = (0u64, 0u64);
        check(unsafe { sys::gsx_model_select_plane(self.v, self.key.as_ptr(), desc, &mut hit, &mut selected) })?;
        Ok((hit, selected))
    }
    /// `gsx_plane_level` (host only): `(quat, pos)` — the shortest-arc rotation (x, y, z, w; w >= 0) that takes the plane's unit normal
    /// to `up / |up|` and the translation that puts the rotated plane through the origin's height: `update_model_transform`'s or
    /// `apply_transform`'s arguments with scale 1.
    pub fn plane_level(plane: &sys::gsx_plane_t, up: [f32; 3]) -> Result<([f32; 4], [f32; 3]), Error> {
        let (mut quat, mut pos) = ([0f32; 4], [0f32; 3]);
        check(unsafe { sys::gsx_plane_level(plane, up.as_ptr(), quat.as_mut_ptr(), pos.as_mut_ptr()) })?;
        Ok((quat, pos))
    }
}

pub struct Preprocessor(*mut sys::gsx_viewer);
impl Preprocessor {
    /// `preprocessor.preprocess(&mut encoder, &bind_group, len)` (scene.rs:856-863): the model is named by its key.
    pub fn preprocess(&self, key: &str) { let k = CString::new(key).unwrap(); check(unsafe { sys::gsx_preprocess(self.0, k.as_ptr()) }).expect("preprocess") }
}
pub struct RadixSorter(*mut sys::gsx_viewer);
impl RadixSorter {
    /// `radix_sorter.sort(&mut encoder, &bind_group, &indirect_args)` (scene.rs:865-869)
    pub fn sort(&self, key: &str) { let k = CString::new(key).unwrap(); check(unsafe { sys::gsx_sort(self.0, k.as_ptr()) }).expect("sort") }
}
pub struct Renderer(*mut sys::gsx_viewer);
impl Renderer {
    /// the `render_with_pass` loop over `model_render_keys`, far -> near (scene.rs:2302-2314), as one call
    pub fn render(&self, model_render_keys: &[String]) {
        let keys: Vec<CString> = model_render_keys.iter().map(|k| CString::new(k.as_str()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = keys.iter().map(|k| k.as_ptr()).collect();
        check(unsafe { sys::gsx_render(self.0, ptrs.as_ptr(), ptrs.len() as u32) }).expect("render")
    }
}
pub struct Postprocessor(*mut sys::gsx_viewer);
impl Postprocessor {
    /// `postprocessor.postprocess(&mut encoder, bg0, bg1, len, &indirect_args)` (scene.rs:601-611)
    pub fn postprocess(&self, key: &str) { let k = CString::new(key).unwrap(); check(unsafe { sys::gsx_postprocess(self.0, k.as_ptr()) }).expect("postprocess") }
}

/// `gs::MultiModelViewer<G>` (scene.rs:1930): public fields as the app reads them (scene.rs:2115-2120, 2133-2139).
pub struct MultiModelViewer<G: GaussianPod> {
    handle: Handle,
    pub models: HashMap<String, MultiModelViewerModel>,
    pub preprocessor: Preprocessor,
    pub radix_sorter: RadixSorter,
    pub renderer: Renderer,
    pub postprocessor: Postprocessor,
    _pod: PhantomData<G>,
}
impl<G: GaussianPod> MultiModelViewer<G> {
    /// `MultiModelViewer::new_with(&device, target_format, depth_stencil, uvec2(1, 1))` (scene.rs:1969-1980).  The format does not
    /// apply (the result is an (rgb, T) float image); `depth_stencil = Some(..)` — the app's
    /// `DepthStencilState { Depth32Float, depth_write_enabled: false, Less }` — turns on the depth test against the buffer given to
    /// `update_depth_buffer` each frame (`None`: no test).  The state itself is not inspected: libgsx has `Less` without depth write
    /// only (the app's state), so ANY `Some(..)` — another compare, depth write on — is taken as that; map other states yourself.
    /// With `frames_in_flight > 1` a depth-tested frame is dealt to a lane like any other and the lane takes its own snapshot: the
    /// buffer is read as if on the viewer's stream at the `render_frame` that uses it — what is set or enqueued there afterwards
    /// waits for that read (no host wait), not for the frame (`gsx.h`, the depth block).
    pub fn new_with<D, F, S>(_device: &D, _format: F, depth_stencil: Option<S>, size: (u32, u32)) -> Result<Self, Error> {
        let desc = sys::gsx_viewer_desc { abi_version: sys::GSX_ABI_VERSION, device: 0, stream: std::ptr::null_mut(), width: size.0, height: size.1 };
        let mut v = std::ptr::null_mut();
        check(unsafe { sys::gsx_viewer_create(&desc, &mut v) })?;
        let viewer = Self { handle: Handle(v), models: HashMap::new(), preprocessor: Preprocessor(v), radix_sorter: RadixSorter(v), renderer: Renderer(v),
                            postprocessor: Postprocessor(v), _pod: PhantomData };
        if depth_stencil.is_some() {
            check(unsafe { sys::gsx_viewer_set_depth_test(v, sys::gsx_depth_compare::Less) })?;
        }
        Ok(viewer)
    }
    /// The frame's depth attachment after the gizmo and measurement passes (`Depth32Float`, `[height][width]`, row 0 at the top),
    /// copied; read by the frame's first preprocess.
    pub fn update_depth_buffer(&mut self, depth: &[f32], size: (u32, u32)) -> Result<(), Error> {
        if depth.len() != size.0 as usize * size.1 as usize {
            return Err(Error::Gsx { status: sys::GSX_ERR_INVALID_ARG, message: "update_depth_buffer: depth.len() != width * height".into() });
        }
        check(unsafe { sys::gsx_viewer_upload_depth_buffer(self.handle.0, depth.as_ptr(), size.0, size.1) })
    }
    /// `gsx_render_depth_map`: walks the models in the order a frame composites them (the LAST key first) with the viewer's current
    /// camera and keeps per pixel (`[height][width]`, row 0 at the top) the surface depth — the view depth of the first record after
    /// whose blend `T < threshold`, `+inf` without one — that record's Gaussian index and layer (`GSX_DEPTH_MAP_NONE` without),
    /// `S = sum w * d`, `A = sum w` and the final `T`.  `rows`: download the planes (surface, sum, alpha, transmittance, index,
    /// layer), otherwise they stay on the device alone (`depth_map_device_ptrs`).  With `ndc` an NDC depth plane is written as well,
    /// which `gsx_viewer_set_depth_buffer_device` takes as it is.
    #[allow(clippy::type_complexity)]
    pub fn render_depth_map(&mut self, model_render_keys: &[String], threshold: f32, ndc: bool, rows: bool, size: (u32, u32))
        -> Result<([Vec<f32>; 4], [Vec<u32>; 2], sys::gsx_depth_map_stats_t), Error> {
        let keys: Vec<CString> = model_render_keys.iter().map(|k| CString::new(k.as_str()).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = keys.iter().map(|k| k.as_ptr()).collect();
        let n = if rows { size.0 as usize * size.1 as usize } else { 0 };
        let mut f: [Vec<f32>; 4] = [vec![0f32; n], vec![0f32; n], vec![0f32; n], vec![0f32; n]];
        let mut u: [Vec<u32>; 2] = [vec![sys::GSX_DEPTH_MAP_NONE; n], vec![sys::GSX_DEPTH_MAP_NONE; n]];
        let desc = sys::gsx_depth_map_desc { flags: if ndc { sys::GSX_DEPTH_MAP_NDC } else { 0 }, threshold, reserved: [0; 2] };
        let mut out = sys::gsx_depth_map_stats_t::default();
        let fp = |v: &mut Vec<f32>| if rows { v.as_mut_ptr() } else { std::ptr::null_mut() };
        let (p0, p1, p2, p3) = (fp(&mut f[0]), fp(&mut f[1]), fp(&mut f[2]), fp(&mut f[3]));
        let up = |v: &mut Vec<u32>| if rows { v.as_mut_ptr() } else { std::ptr::null_mut() };
        let (q0, q1) = (up(&mut u[0]), up(&mut u[1]));
        check(unsafe { sys::gsx_render_depth_map(self.handle.0, ptrs.as_ptr(), ptrs.len() as u32, &desc, p0, p1, p2, p3, q0, q1, &mut out) })?;
        Ok((f, u, out))
    }
    /// `gsx_depth_map_device_ptrs`: the last depth map's planes on the device — surface, sum, alpha, transmittance, index, layer, ndc
    /// (null unless it was asked for) — and its size; valid until the next `render_depth_map`, a viewport change or the viewer's end.
    pub fn depth_map_device_ptrs(&self) -> Result<([*mut std::os::raw::c_void; 7], (u32, u32)), Error> {
        let mut p = [std::ptr::null_mut(); 7];
        let (mut w, mut h) = (0u32, 0u32);
        let q = p.as_mut_ptr();
        check(unsafe { sys::gsx_depth_map_device_ptrs(self.handle.0, q, q.add(1), q.add(2), q.add(3), q.add(4), q.add(5), q.add(6), &mut w, &mut h) })?;
        Ok((p, (w, h)))
    }
    /// `gsx_depth_map_unproject` (host only): the world-space point seen at pixel position `(px, py)` at view depth `view_depth`.
    pub fn depth_map_unproject(view: &[f32; 16], proj: &[f32; 16], size: (u32, u32), px: f32, py: f32, view_depth: f32) -> Result<[f32; 3], Error> {
        let mut w = [0f32; 3];
        check(unsafe { sys::gsx_depth_map_unproject(view.as_ptr(), proj.as_ptr(), size.0, size.1, px, py, view_depth, w.as_mut_ptr()) })?;
        Ok(w)
    }
    /// `MeasurementRenderer::update_hit_pairs(&device, &hit_pairs, &camera)` (src/renderer/measurement.rs:133-167): the measurement
    /// lines, drawn by the library with depth write before the splats of every frame from then on (`gsx.h`, the overlay block) — no
    /// depth attachment has to be handed over for them.  An empty slice clears them.
    pub fn update_hit_pairs(&mut self, hit_pairs: &[sys::gsx_overlay_line]) -> Result<(), Error> {
        let p = if hit_pairs.is_empty() { std::ptr::null() } else { hit_pairs.as_ptr() };
        check(unsafe { sys::gsx_viewer_set_overlay_lines(self.handle.0, p, hit_pairs.len() as u32) })
    }
    /// `gs::MaskGizmo::update` + `render_box_with_pass` / `render_ellipsoid_with_pass` (src/tab/scene.rs:2211-2247, 2283-2293): the mask
    /// shapes' wireframes, drawn by the library before the measurement lines, with their depth state (`gsx.h`, the gizmo block).  Pass, for
    /// each render key, that model's visible boxes and then its visible ellipsoids, in world space.  An empty slice clears them.
    pub fn set_mask_gizmos(&mut self, gizmos: &[sys::gsx_mask_gizmo]) -> Result<(), Error> {
        let p = if gizmos.is_empty() { std::ptr::null() } else { gizmos.as_ptr() };
        check(unsafe { sys::gsx_viewer_set_mask_gizmos(self.handle.0, p, gizmos.len() as u32) })
    }
    /// Last frame's overlay: premultiplied rgba `[height][width][4]` and the effective depth `[height][width]` the splats were tested against.
    pub fn download_overlay(&mut self, size: (u32, u32)) -> Result<(Vec<f32>, Vec<f32>), Error> {
        let n = size.0 as usize * size.1 as usize;
        let (mut rgba, mut depth) = (vec![0f32; 4 * n], vec![0f32; n]);
        check(unsafe { sys::gsx_download_overlay(self.handle.0, rgba.as_mut_ptr(), depth.as_mut_ptr()) })?;
        Ok((rgba, depth))
    }
    /// `GaussianBuffers::new_empty(&device, count)` + `BindGroups::new(..)` + `models.insert(key, ..)` (scene.rs:2111-2139)
    pub fn insert_model(&mut self, key: &str, count: usize) -> Result<(), Error> {
        let k = CString::new(key).unwrap();
        check(unsafe { sys::gsx_model_create(self.handle.0, k.as_ptr(), count as u64, G::SH, G::COV3D) })?;
        let v = self.handle.0;
        self.models.insert(key.to_owned(), MultiModelViewerModel { gaussian_buffers: MultiModelViewerGaussianBuffers {
            gaussians_buffer: GaussiansBuffer { v, key: k.clone() },
            mask_buffer: MaskBuffer { v, key: k.clone(), words: (count + 31) / 32 },
            gaussians_edit_buffer: GaussiansEditBuffer { v, key: k.clone(), n: count },
        }, v, key: k });
        Ok(())
    }
    /// `gsx_model_extract`: the Gaussians of `src_key` that pass `filter` (`sys::GSX_BOUNDS_*`; `flags`: `sys::GSX_EXTRACT_INVERT`,
    /// `sys::GSX_EXTRACT_DROP_EDITS`) become the new model `dst_key`, in their order, on the device, as stored bits.  Returns the
    /// number kept; 0 creates no model.  "Apply the mask": `extract(k, a, GSX_BOUNDS_MASKED | GSX_BOUNDS_SKIP_HIDDEN, 0)`, `remove_model(k)`.
    pub fn extract(&mut self, src_key: &str, dst_key: &str, filter: u32, flags: u32) -> Result<u64, Error> {
        let (s, k) = (CString::new(src_key).unwrap(), CString::new(dst_key).unwrap());
        let desc = sys::gsx_extract_desc { filter, flags };
        let mut count = 0u64;
        check(unsafe { sys::gsx_model_extract(self.handle.0, s.as_ptr(), k.as_ptr(), &desc, &mut count) })?;
        if count > 0 {
            let (v, n) = (self.handle.0, count as usize);
            self.models.insert(dst_key.to_owned(), MultiModelViewerModel { gaussian_buffers: MultiModelViewerGaussianBuffers {
                gaussians_buffer: GaussiansBuffer { v, key: k.clone() },
                mask_buffer: MaskBuffer { v, key: k.clone(), words: (n + 31) / 32 },
                gaussians_edit_buffer: GaussiansEditBuffer { v, key: k.clone(), n },
            }, v, key: k });
        }
        Ok(count)
    }
    /// `gsx_model_decimate`: the Gaussians of `src_key` that share a cell of a grid of edge `desc.cell` become one moment-matched
    /// Gaussian of the new model `dst_key`, on the device (one-member cells are copied as stored bits).  Returns the statistics and
    /// the `dst` index of every source Gaussian; `cells == 0` creates no model.
    pub fn decimate(&mut self, src_key: &str, dst_key: &str, desc: &sys::gsx_decimate_desc) -> Result<(sys::gsx_decimate_stats_t, Vec<u32>), Error> {
        let (s, k) = (CString::new(src_key).unwrap(), CString::new(dst_key).unwrap());
        let mut len = 0u64;
        check(unsafe { sys::gsx_model_len(self.handle.0, s.as_ptr(), &mut len) })?;
        let mut map = vec![u32::MAX; len as usize];
        let mut out = sys::gsx_decimate_stats_t::default();
        check(unsafe { sys::gsx_model_decimate(self.handle.0, s.as_ptr(), k.as_ptr(), desc, map.as_mut_ptr(), &mut out) })?;
        if out.cells > 0 {
            let (v, n) = (self.handle.0, out.cells as usize);
            self.models.insert(dst_key.to_owned(), MultiModelViewerModel { gaussian_buffers: MultiModelViewerGaussianBuffers {
                gaussians_buffer: GaussiansBuffer { v, key: k.clone() },
                mask_buffer: MaskBuffer { v, key: k.clone(), words: (n + 31) / 32 },
                gaussians_edit_buffer: GaussiansEditBuffer { v, key: k.clone(), n },
            }, v, key: k });
        }
        Ok((out, map))
    }
    /// `gsx_model_convert`: `extract` into a model of the pod kind `(sh, cov3d)`: position and colour word carried, covariance and SH
    /// dequantised exactly and quantised once into the new kind, on the device.  The same kind is `extract`.  Returns the number kept;
    /// 0 creates no model.  Models of different kinds are merged by converting first.
    pub fn convert(&mut self, src_key: &str, dst_key: &str, sh: sys::gsx_sh_kind, cov3d: sys::gsx_cov3d_kind, filter: u32, flags: u32) -> Result<u64, Error> {
        let (s, k) = (CString::new(src_key).unwrap(), CString::new(dst_key).unwrap());
        let desc = sys::gsx_convert_desc { filter, flags, sh: sh as u32, cov3d: cov3d as u32 };
        let mut count = 0u64;
        check(unsafe { sys::gsx_model_convert(self.handle.0, s.as_ptr(), k.as_ptr(), &desc, &mut count) })?;
        if count > 0 {
            let (v, n) = (self.handle.0, count as usize);
            self.models.insert(dst_key.to_owned(), MultiModelViewerModel { gaussian_buffers: MultiModelViewerGaussianBuffers {
                gaussians_buffer: GaussiansBuffer { v, key: k.clone() },
                mask_buffer: MaskBuffer { v, key: k.clone(), words: (n + 31) / 32 },
                gaussians_edit_buffer: GaussiansEditBuffer { v, key: k.clone(), n },
            }, v, key: k });
        }
        Ok(count)
    }
    /// `gsx_model_merge`: the Gaussians of the models `src_keys` that pass `filter` become the one new model `dst_key`, source after
    /// source, each source's model transform baked into its Gaussians (an identity source travels as stored bits); `dst_key` has the
    /// identity transform.  Returns the total kept and one kept count per source; a total of 0 creates no model.
    pub fn merge(&mut self, src_keys: &[&str], dst_key: &str, filter: u32, flags: u32) -> Result<(u64, Vec<u64>), Error> {
        let keys: Vec<CString> = src_keys.iter().map(|s| CString::new(*s).unwrap()).collect();
        let ptrs: Vec<*const std::os::raw::c_char> = keys.iter().map(|k| k.as_ptr()).collect();
        let k = CString::new(dst_key).unwrap();
        let desc = sys::gsx_extract_desc { filter, flags };
        let (mut counts, mut total) = (vec![0u64; keys.len().max(1)], 0u64);
        check(unsafe { sys::gsx_model_merge(self.handle.0, ptrs.as_ptr(), ptrs.len() as u32, k.as_ptr(), &desc, counts.as_mut_ptr(), &mut total) })?;
        counts.truncate(keys.len());
        if total > 0 {
            let (v, n) = (self.handle.0, total as usize);
            self.models.insert(dst_key.to_owned(), MultiModelViewerModel { gaussian_buffers: MultiModelViewerGaussianBuffers {
                gaussians_buffer: GaussiansBuffer { v, key: k.clone() },
                mask_buffer: MaskBuffer { v, key: k.clone(), words: (n + 31) / 32 },
                gaussians_edit_buffer: GaussiansEditBuffer { v, key: k.clone(), n },
            }, v, key: k });
        }
        Ok((total, counts))
    }
    /// `gsx_model_export`: the Gaussians of `key` that pass `filter` (`flags`: `sys::GSX_EXTRACT_INVERT`, `sys::GSX_EXPORT_BAKE_EDITS`)
    /// as `gsx_gaussian` records in model space, rotation and scale solved from the stored covariance on the device.  The way out
    /// for a model that only the device holds (`extract`, `merge`).
    pub fn export(&mut self, key: &str, filter: u32, flags: u32) -> Result<Vec<sys::gsx_gaussian>, Error> {
        let k = CString::new(key).unwrap();
        let desc = sys::gsx_export_desc { filter, flags, format: sys::GSX_EXPORT_GAUSSIANS, reserved: 0, staging_bytes: 0 };
        let mut count = 0u64;
        check(unsafe { sys::gsx_model_export(self.handle.0, k.as_ptr(), &desc, std::ptr::null_mut(), 0, &mut count) })?;
        let mut out: Vec<sys::gsx_gaussian> = Vec::with_capacity(count as usize);
        if count > 0 {
            let bytes = count * std::mem::size_of::<sys::gsx_gaussian>() as u64;
            check(unsafe { sys::gsx_model_export(self.handle.0, k.as_ptr(), &desc, out.as_mut_ptr() as *mut std::os::raw::c_void, bytes, &mut count) })?;
            unsafe { out.set_len(count as usize) };  // every byte of every record is written by the library
        }
        Ok(out)
    }
    /// `gsx_model_export_ply`: the same Gaussians as a binary INRIA PLY file.  The reference's `write_ply(edits, mask)` is
    /// `export_ply(key, GSX_BOUNDS_MASKED | GSX_BOUNDS_SKIP_HIDDEN, GSX_EXPORT_BAKE_EDITS)`.
    pub fn export_ply(&mut self, key: &str, filter: u32, flags: u32) -> Result<Vec<u8>, Error> {
        let k = CString::new(key).unwrap();
        let desc = sys::gsx_export_desc { filter, flags, format: sys::GSX_EXPORT_PLY_VERTICES, reserved: 0, staging_bytes: 0 };
        let mut size = 0u64;
        check(unsafe { sys::gsx_model_export_ply(self.handle.0, k.as_ptr(), &desc, std::ptr::null_mut(), 0, &mut size) })?;
        let mut out = vec![0u8; size as usize];
        check(unsafe { sys::gsx_model_export_ply(self.handle.0, k.as_ptr(), &desc, out.as_mut_ptr() as *mut std::os::raw::c_void, size, &mut size) })?;
        Ok(out)
    }
    /// `gsx_model_import_ply`: the app's load path `read_ply_header -> read_ply_gaussians -> Gaussian::from -> update_range`
    /// (app.rs:1053-1096) in one call, the rows decoded on the device: a binary INRIA PLY file becomes the new model `key` of pod `G`.
    /// Returns the count; a file of 0 vertices creates no model.
    pub fn import_ply(&mut self, key: &str, data: &[u8]) -> Result<u64, Error> {
        let k = CString::new(key).unwrap();
        let desc = sys::gsx_import_desc { flags: 0, reserved: 0, staging_bytes: 0 };
        let mut count = 0u64;
        check(unsafe { sys::gsx_model_import_ply(self.handle.0, k.as_ptr(), data.as_ptr() as *const std::os::raw::c_void, data.len() as u64, G::SH, G::COV3D, &desc, &mut count) })?;
        if count > 0 {
            let (v, n) = (self.handle.0, count as usize);
            self.models.insert(key.to_owned(), MultiModelViewerModel { gaussian_buffers: MultiModelViewerGaussianBuffers {
                gaussians_buffer: GaussiansBuffer { v, key: k.clone() },
                mask_buffer: MaskBuffer { v, key: k.clone(), words: (n + 31) / 32 },
                gaussians_edit_buffer: GaussiansEditBuffer { v, key: k.clone(), n },
            }, v, key: k });
        }
        Ok(count)
    }
    /// `viewer.remove_model(&key)` (scene.rs:2176)
    pub fn remove_model(&mut self, key: &str) {
        let k = CString::new(key).unwrap();
        check(unsafe { sys::gsx_model_remove(self.handle.0, k.as_ptr()) }).expect("remove_model");
        self.models.remove(key);
    }
    /// `viewer.update_camera(&queue, &impl CameraTrait, uvec2 size)` (scene.rs:795)
    pub fn update_camera<Q>(&mut self, _queue: &Q, camera: &impl CameraTrait, size: (u32, u32)) {
        let (view, proj) = (camera.view(), camera.projection(size.0 as f32 / size.1 as f32));
        check(unsafe { sys::gsx_update_camera(self.handle.0, view.as_ptr(), proj.as_ptr(), size.0, size.1) }).expect("update_camera")
    }
    /// `viewer.update_model_transform(&queue, key, pos, quat, scale)` (scene.rs:796-802); quat = glam x, y, z, w
    pub fn update_model_transform<Q>(&mut self, _queue: &Q, key: &str, pos: [f32; 3], quat: [f32; 4], scale: [f32; 3]) {
        let k = CString::new(key).unwrap();
        check(unsafe { sys::gsx_update_model_transform(self.handle.0, k.as_ptr(), pos.as_ptr(), quat.as_ptr(), scale.as_ptr()) }).expect("update_model_transform")
    }
    /// `viewer.update_gaussian_transform(&queue, size, display_mode, sh_deg, no_sh0)` (scene.rs:803-809)
    pub fn update_gaussian_transform<Q>(&mut self, _queue: &Q, size: f32, mode: GaussianDisplayMode, sh_deg: GaussianShDegree, no_sh0: bool) {
        let m = match mode { GaussianDisplayMode::Splat => sys::gsx_display_mode::Splat, GaussianDisplayMode::Ellipse => sys::gsx_display_mode::Ellipse,
                             GaussianDisplayMode::Point => sys::gsx_display_mode::Point };
        check(unsafe { sys::gsx_update_gaussian_transform(self.handle.0, size, m, sh_deg.degree(), no_sh0 as u32) }).expect("update_gaussian_transform")
    }
    /// `viewer.update_query(&queue, &pod)` (scene.rs:785)
    pub fn update_query<Q>(&mut self, _queue: &Q, query: &sys::gsx_query) { check(unsafe { sys::gsx_update_query(self.handle.0, query) }).expect("update_query") }
    /// `viewer.update_selection_highlight(&queue, vec4)` (scene.rs:816-829)
    pub fn update_selection_highlight<Q>(&mut self, _queue: &Q, rgba: [f32; 4]) {
        check(unsafe { sys::gsx_update_selection_highlight(self.handle.0, rgba.as_ptr()) }).expect("update_selection_highlight")
    }
    /// `viewer.update_selection_edit_with_pod(&queue, &pod)` (scene.rs:815, 821, 848)
    pub fn update_selection_edit_with_pod<Q>(&mut self, _queue: &Q, pod: &GaussianEditPod) {
        check(unsafe { sys::gsx_update_selection_edit(self.handle.0, pod) }).expect("update_selection_edit_with_pod")
    }
    /// `mask_evaluator.evaluate(&device, &queue, &MaskOpTree, &mask_buffer, &model_transform_buffer, &gaussians_buffer)` (scene.rs:2124-2131,
    /// 2201-2209): the tree in postfix order (`MaskOpTree::Reset` = no ops), evaluated on the GPU, no readback.
    pub fn evaluate_mask(&mut self, key: &str, ops: &[sys::gsx_mask_op], shapes: &[sys::gsx_mask_shape]) -> Result<(), Error> {
        let k = CString::new(key).unwrap();
        check(unsafe { sys::gsx_mask_evaluate(self.handle.0, k.as_ptr(), ops.as_ptr(), ops.len() as u32, shapes.as_ptr(), shapes.len() as u32) })
    }
    /// `queue.submit(..); device.poll(wgpu::Maintain::Wait)` (scene.rs:613-614, 872-873)
    pub fn poll(&self) { check(unsafe { sys::gsx_sync(self.handle.0) }).expect("poll") }
    /// what `SceneCallback::paint` blits instead of the `render_with_pass` loop
    pub fn download_rgba8(&self, background: [f32; 3], width: u32, height: u32) -> Result<Vec<u8>, Error> {
        let mut px = vec![0u8; 4 * width as usize * height as usize];
        check(unsafe { sys::gsx_download_rgba8(self.handle.0, background.as_ptr(), px.as_mut_ptr(), px.len() as u64) })?;
        Ok(px)
    }

    // ---- multi-GPU (no counterpart in the reference: src/main.rs:85-98 opens one wgpu device) ----
    /// One rank of an index-sharded viewer: `id` from `comm_unique_id()` on rank 0, carried to the other ranks by the host.
    pub fn comm_init(&mut self, world: u32, rank: u32, id: &[u8; 128]) -> Result<(), Error> { check(unsafe { sys::gsx_viewer_comm_init(self.handle.0, world, rank, id.as_ptr()) }) }
    /// One whole index-sharded frame of `key` (include/gsx.h "device-resident protocol"): afterwards every rank holds the frame.
    pub fn shard_render_frame(&mut self, key: &str, shard_records_max: u32, speculate: bool, margin: f32, radius: u32) -> Result<(), Error> {
        let k = CString::new(key).unwrap();
        check(unsafe { sys::gsx_shard_render_frame(self.handle.0, k.as_ptr(), shard_records_max, speculate as u32, margin, radius) })
    }
}
impl<G: GaussianPod> MultiModelViewer<G> {
    /// Layered models far -> near like `renderer.render` (scene.rs:2302-2314), every model index-sharded over the ranks.
    pub fn shard_render_frame_keys(&mut self, model_render_keys: &[String], shard_records_max: &[u32], speculate: bool, margin: f32, radius: u32) -> Result<(), Error> {
        let ks: Vec<CString> = model_render_keys.iter().map(|k| CString::new(k.as_str()).unwrap()).collect();
        let ps: Vec<*const std::os::raw::c_char> = ks.iter().map(|k| k.as_ptr()).collect();
        check(unsafe { sys::gsx_shard_render_frame_keys(self.handle.0, ps.as_ptr(), ps.len() as u32, shard_records_max.as_ptr(), speculate as u32, margin, radius) })
    }
    /// Where a sharded frame's bands go: `None` = every rank ends up with the whole frame (default), `Some(r)` = only rank `r`.
    pub fn shard_set_gather_root(&mut self, root: Option<u32>) -> Result<(), Error> { check(unsafe { sys::gsx_shard_set_gather_root(self.handle.0, root.map(|r| r as i32).unwrap_or(-1)) }) }
    /// One process, one thread + one viewer per GPU: seat `rank` of an in-process group (`sys::gsx_comm_group_create`).
    /// What the viewer's communicator really is (transport, ranks RCCL saw — `ncclCommCount` —, this rank, RCCL's version): a multi-process
    /// deployment asserts `nranks == world` before its first frame.
    pub fn comm_info(&mut self) -> Result<sys::gsx_comm_info, Error> {
        let mut info = sys::gsx_comm_info::default();
        check(unsafe { sys::gsx_viewer_comm_info(self.handle.0, &mut info) })?;
        Ok(info)
    }
    pub fn comm_init_group(&mut self, group: *mut sys::gsx_comm_group, rank: u32) -> Result<(), Error> { check(unsafe { sys::gsx_viewer_comm_init_group(self.handle.0, group, rank) }) }
}
/// `gs::QueryToolsetTool` (scene.rs:1258-1264)
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum QueryToolsetTool { Rect = 0, Brush = 1 }

/// `gs::QueryToolset` (scene.rs:766-791) of a viewer, inside the library: `start` / `update_pos` queue what they paint and `render`
/// enqueues it on the viewer's stream as one launch — the query texture never crosses the host (include/gsx.h, the toolset block).
/// Borrowed from the viewer: `viewer.query_toolset()`.
pub struct QueryToolset<'a> { v: *mut sys::gsx_viewer, _viewer: PhantomData<&'a mut ()> }
impl<'a> QueryToolset<'a> {
    pub fn set_use_texture(&mut self, on: bool) { check(unsafe { sys::gsx_toolset_set_use_texture(self.v, on as u32) }).expect("set_use_texture") }
    pub fn update_brush_radius(&mut self, radius: f32) -> Result<(), Error> { check(unsafe { sys::gsx_toolset_update_brush_radius(self.v, radius) }) }
    pub fn start(&mut self, tool: QueryToolsetTool, op: u32, pos: [f32; 2]) -> Result<(), Error> { check(unsafe { sys::gsx_toolset_start(self.v, tool as u32, op, pos.as_ptr()) }) }
    pub fn update_pos(&mut self, pos: [f32; 2]) -> Result<(), Error> { check(unsafe { sys::gsx_toolset_update_pos(self.v, pos.as_ptr()) }) }
    pub fn end(&mut self) { check(unsafe { sys::gsx_toolset_end(self.v) }).expect("end") }
    /// `query_toolset.query()`: this frame's query, for `viewer.update_query`
    pub fn query(&mut self) -> sys::gsx_query {
        let mut q = sys::gsx_query { kind: 0, selection_op: 0, p0: [0.0; 2], p1: [0.0; 2], radius: 0.0, reserved: 0 };
        check(unsafe { sys::gsx_toolset_query(self.v, &mut q) }).expect("query");
        q
    }
    /// `query_toolset.state()`: `Some((tool, op, start, pos))` while a stroke is under way
    pub fn state(&self) -> Option<(QueryToolsetTool, u32, [f32; 2], [f32; 2])> {
        let (mut active, mut tool, mut op, mut start, mut pos) = (0u32, 0u32, 0u32, [0f32; 2], [0f32; 2]);
        check(unsafe { sys::gsx_toolset_state(self.v, &mut active, &mut tool, &mut op, start.as_mut_ptr(), pos.as_mut_ptr()) }).expect("state");
        if active == 0 { return None; }
        let tool = match tool {
            0 => QueryToolsetTool::Rect,
            1 => QueryToolsetTool::Brush,
            t => unreachable!("gsx_toolset_state: tool {t} (gsx_toolset_start takes GSX_TOOL_RECT and GSX_TOOL_BRUSH only)"),
        };
        Some((tool, op, start, pos))
    }
    /// `query_toolset.render(&queue, &mut encoder, &query_texture)` (scene.rs:791)
    pub fn render(&mut self) -> Result<(), Error> { check(unsafe { sys::gsx_toolset_render(self.v) }) }
}
impl<G: GaussianPod> MultiModelViewer<G> {
    pub fn query_toolset(&mut self) -> QueryToolset<'_> { QueryToolset { v: self.handle.0, _viewer: PhantomData } }
    /// `QueryTextureOverlay` / `QueryCursor` (scene.rs:2003-2014, 2317-2325): the straight-alpha colours `download_rgba8` draws the stroke
    /// and the cursor with; alpha 0 (the default) draws nothing
    pub fn set_toolset_overlay(&mut self, texture_rgba: [f32; 4], cursor_rgba: [f32; 4], cursor_thickness: f32) -> Result<(), Error> {
        check(unsafe { sys::gsx_toolset_set_overlay(self.handle.0, texture_rgba.as_ptr(), cursor_rgba.as_ptr(), cursor_thickness) })
    }
    /// the query texture as the device holds it (the viewport's size once the toolset has rendered)
    pub fn download_query_texture(&self, width: u32, height: u32) -> Result<Vec<u8>, Error> {
        let mut t = vec![0u8; width as usize * height as usize];
        check(unsafe { sys::gsx_download_query_texture(self.handle.0, t.as_mut_ptr(), width, height) })?;
        Ok(t)
    }
}
pub fn comm_unique_id() -> Result<[u8; 128], Error> {
    let mut id = [0u8; 128];
    check(unsafe { sys::gsx_comm_unique_id(id.as_mut_ptr()) })?;
    Ok(id)
}

/// `gs::Gaussians { gaussians }`: `read_ply_header` / `PlyHeader::count` / `read_ply_gaussians` + `Gaussian::from(PlyGaussianPod)`
/// (app.rs:1053-1096) and `write_ply(writer, edits, mask)` (app.rs:897-947), over the library's host-side PLY code.
pub struct Gaussians { pub gaussians: Vec<Gaussian> }
impl Gaussians {
    pub fn read_ply(data: &[u8]) -> Result<Self, Error> {
        let mut h = std::mem::MaybeUninit::<sys::gsx_ply_header>::uninit();
        check(unsafe { sys::gsx_ply_read_header(data.as_ptr().cast(), data.len() as u64, h.as_mut_ptr()) })?;
        let h = unsafe { h.assume_init() };
        let mut g = Vec::with_capacity(h.count as usize);
        check(unsafe { sys::gsx_ply_read_gaussians(data.as_ptr().cast(), data.len() as u64, &h, 0, h.count, g.as_mut_ptr()) })?;
        unsafe { g.set_len(h.count as usize) };
        Ok(Self { gaussians: g })
    }
    pub fn write_ply(&self, edits: Option<&[GaussianEditPod]>, mask: Option<&[u32]>) -> Result<Vec<u8>, Error> {
        let (e, m) = (edits.map_or(std::ptr::null(), |e| e.as_ptr()), mask.map_or(std::ptr::null(), |m| m.as_ptr()));
        let mut size = 0u64;
        check(unsafe { sys::gsx_ply_write(self.gaussians.as_ptr(), self.gaussians.len() as u64, m, e, std::ptr::null_mut(), 0, &mut size) })?;
        let mut out = vec![0u8; size as usize];
        check(unsafe { sys::gsx_ply_write(self.gaussians.as_ptr(), self.gaussians.len() as u64, m, e, out.as_mut_ptr().cast(), size, &mut size) })?;
        Ok(out)
    }
}
