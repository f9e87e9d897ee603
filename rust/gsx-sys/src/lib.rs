//! gsx-sys — raw FFI over `include/gsx.h` (libgsx.so, the MI355X-native 3DGS render path).
//!
//! NOT COMPILED IN THIS REPOSITORY (no Rust toolchain in the build image): this is the binding source a maintainer of
//! LioQing/wgpu-3dgs-viewer-app would add, kept next to the header it mirrors.  The function list is generated from the
//! header by `tools/gen_rust_sys.py` (= what `bindgen` emits); `tests/test_oracle_cpu.py` checks that it covers every
//! exported symbol.  Safe wrappers with the crate's names live in `rust/gsx` (`gs::MultiModelViewer`, ...).
//!
//! build.rs (sketch): `println!("cargo:rustc-link-lib=dylib=gsx"); println!("cargo:rustc-link-search=native={}", env!("GSX_LIB_DIR"));`
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub const GSX_ABI_VERSION: u32 = 3;
pub const GSX_TILE: u32 = 16;
pub const GSX_SH_COEFFS: usize = 15;
pub const GSX_RECORD_BYTES: u32 = 48;
pub const GSX_MASK_MAX_OPS: u32 = 64;
pub const GSX_MASK_MAX_SHAPES: u32 = 32;
pub const GSX_QUERY_MAX_HITS: u32 = 65536;
pub const GSX_OVERLAY_MAX_LINES: u32 = 4096;
pub const GSX_GIZMO_MAX_SHAPES: u32 = 256;
pub const GSX_GIZMO_CIRCLE_SEGMENTS: u32 = 64;
pub const GSX_EDIT_ENABLED: u32 = 1;
pub const GSX_EDIT_HIDDEN: u32 = 2;
pub const GSX_EDIT_OVERRIDE_COLOR: u32 = 4;
pub const GSX_BOUNDS_MASKED: u32 = 1;
pub const GSX_BOUNDS_SKIP_HIDDEN: u32 = 2;
pub const GSX_BOUNDS_SELECTED: u32 = 4;
pub const GSX_EXTRACT_INVERT: u32 = 1;
pub const GSX_EXTRACT_DROP_EDITS: u32 = 2;
pub const GSX_MERGE_MAX_SOURCES: u32 = 64;
pub const GSX_EXPORT_GAUSSIANS: u32 = 0;
pub const GSX_EXPORT_PLY_VERTICES: u32 = 1;
pub const GSX_EXPORT_BAKE_EDITS: u32 = 4;
pub const GSX_PROP_WORLD: u32 = 1;
pub const GSX_HIST_AUTO_RANGE: u32 = 4;
pub const GSX_HIST_MAX_BINS: u32 = 4096;
pub const GSX_NEIGHBOR_MAX_COUNT: u32 = 4095;
pub const GSX_CLUSTER_NONE: u32 = 0xFFFF_FFFF;
pub const GSX_CLUSTER_BY_SIZE: u32 = 0;
pub const GSX_CLUSTER_LARGEST: u32 = 1;
pub const GSX_CLUSTER_SEEDED: u32 = 2;
pub const GSX_KNN_MAX_K: u32 = 16;
pub const GSX_KNN_SCORE_KTH: u32 = 0;
pub const GSX_KNN_SCORE_MEAN: u32 = 1;
pub const GSX_KNN_SELECT_RANGE: u32 = 0;
pub const GSX_KNN_SELECT_OUTLIERS: u32 = 1;
pub const GSX_NORMALS_MIN_K: u32 = 3;
pub const GSX_NORMALS_MAX_K: u32 = 16;
pub const GSX_NORMALS_ORIENT_CANONICAL: u32 = 0;
pub const GSX_NORMALS_ORIENT_TOWARD: u32 = 1;
pub const GSX_NORMALS_SELECT_VARIATION: u32 = 0;
pub const GSX_NORMALS_SELECT_FACING: u32 = 1;
pub const GSX_NORMALS_ABS: u32 = 1;
pub const GSX_NORMALS_NONE: u32 = 0xFFFF_FFFF;
pub const GSX_NEAREST_NONE: u32 = 0xFFFF_FFFF;
pub const GSX_NEAREST_MODEL_TRANSFORMS: u32 = 1;
pub const GSX_NEAREST_SELECT_RANGE: u32 = 0;
pub const GSX_NEAREST_SELECT_TRANSFER: u32 = 1;
pub const GSX_ALIGN_SCALE: u32 = 1;
pub const GSX_PLANE_MAX_CANDIDATES: u32 = 1024;
pub const GSX_PLANE_MAX_REFINE: u32 = 8;
pub const GSX_PLANE_NONE: u32 = 0xFFFF_FFFF;
pub const GSX_PLANE_SAMPLE_TRIPLES: u32 = 0;
pub const GSX_PLANE_SAMPLE_NORMALS: u32 = 1;
pub const GSX_PLANE_SAMPLE_CALLER: u32 = 2;
pub const GSX_VIS_ACCUMULATE: u32 = 1;
pub const GSX_VIS_PEAK: u32 = 0;
pub const GSX_VIS_WEIGHT: u32 = 1;
pub const GSX_VIS_PIXELS: u32 = 2;
pub const GSX_DEPTH_MAP_NDC: u32 = 1;
pub const GSX_DEPTH_MAP_NONE: u32 = 0xFFFF_FFFF;

pub type gsx_status = i32;
pub const GSX_OK: gsx_status = 0;
pub const GSX_ERR_INVALID_ARG: gsx_status = 1;
pub const GSX_ERR_OOM: gsx_status = 2;
pub const GSX_ERR_HIP: gsx_status = 3;
pub const GSX_ERR_RCCL: gsx_status = 4;
pub const GSX_ERR_IO: gsx_status = 5; // gs::Error::Io
pub const GSX_ERR_PLY: gsx_status = 6;
pub const GSX_ERR_NOT_FOUND: gsx_status = 7;
pub const GSX_ERR_UNSUPPORTED: gsx_status = 8;
pub const GSX_ERR_NO_DEVICE: gsx_status = 9;

/// opaque: `gs::MultiModelViewer<G>` (src/tab/scene.rs:1930)
#[repr(C)]
pub struct gsx_viewer {
    _private: [u8; 0],
}

/// `gs::Gaussian` {rot, pos, color, sh, scale}: field for field, 224 bytes — `&[gs::Gaussian]` crosses the ABI as a pointer
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_gaussian {
    pub rot: [f32; 4], // glam Quat x, y, z, w
    pub pos: [f32; 3],
    pub color: [u8; 4], // UNORM8 r, g, b (0.5 + C0 f_dc), a (sigmoid(opacity))
    pub sh: [[f32; 3]; GSX_SH_COEFFS],
    pub scale: [f32; 3],
}

#[repr(i32)]
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum gsx_sh_kind { Single = 0, Half = 1, Norm8 = 2, None = 3 } // GaussianSh{Single,Half,Norm8,None}Config, src/app.rs:386-403
#[repr(i32)]
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum gsx_cov3d_kind { Single = 0, Half = 1 } // GaussianCov3d{Single,Half}Config, src/app.rs:405-418
#[repr(i32)]
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum gsx_display_mode { Splat = 0, Ellipse = 1, Point = 2 } // gs::GaussianDisplayMode, src/app.rs:1141-1165

#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_spec_params {
    pub max_std_dev: f32, pub cull_margin: f32, pub jacobian_clamp: f32, pub low_pass: f32,
    pub alpha_max: f32, pub alpha_min: f32, pub t_epsilon: f32, pub point_radius: f32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_render_options {
    pub progressive: u32, pub first_slab_divisor: u32, pub min_slab: u32, pub growth: u32,
    pub speculative: u32, pub spec_margin: f32, pub spec_radius: u32, pub host_verify: u32,
    pub frames_in_flight: u32, pub slab_shading: u32,
}
#[repr(C)]
pub struct gsx_viewer_desc { pub abi_version: u32, pub device: i32, pub stream: *mut c_void, pub width: u32, pub height: u32 }
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_mask_shape { pub kind: u32, pub pos: [f32; 3], pub quat_xyzw: [f32; 4], pub scale: [f32; 3] } // gs::MaskOpShapePod
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_mask_op { pub opcode: u32, pub arg: u32 } // postfix MaskOpTree: 0 Shape(arg) 1 Union 2 Intersection 3 Difference 4 SymmetricDifference 5 Complement
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_frame_stats {
    pub n_gaussians: u64, pub n_visible: u64, pub n_tile_entries: u64, pub n_sorted: u64,
    pub n_repair_tiles: u64, pub n_repair_sorted: u64, pub speculated: u32, pub overflow_slabs: u32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_gaussian_edit { pub flag: u32, pub color: [f32; 3], pub contrast: f32, pub exposure: f32, pub gamma: f32, pub alpha: f32 } // gs::GaussianEditPod
/// which Gaussians gsx_model_bounds counts (GSX_BOUNDS_*), and the share (< 500) the trimmed box may leave outside at each end
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_bounds_desc { pub filter: u32, pub trim_permille: u32 }
/// the result of gsx_model_bounds, 88 bytes; model space, Gaussian centres; `center` is GaussianSplattingModel::center (src/app.rs:1019-1046)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_model_bounds_t {
    pub count: u64, pub n_nonfinite: u64, pub min: [f32; 3], pub max: [f32; 3],
    pub center: [f32; 3], pub mean: [f32; 3], pub trim_min: [f32; 3], pub trim_max: [f32; 3],
}
/// which Gaussians gsx_model_extract keeps (filter: GSX_BOUNDS_*) and how (flags: GSX_EXTRACT_*)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_extract_desc { pub filter: u32, pub flags: u32 }
/// what gsx_model_export writes (filter: GSX_BOUNDS_*; flags: GSX_EXTRACT_INVERT, GSX_EXPORT_BAKE_EDITS; format: GSX_EXPORT_*)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_export_desc { pub filter: u32, pub flags: u32, pub format: u32, pub reserved: u32, pub staging_bytes: u64 }
/// how gsx_model_import_ply and gsx_model_upload_ply_rows stage their rows (flags: none are defined; staging_bytes 0: the default)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_import_desc { pub flags: u32, pub reserved: u32, pub staging_bytes: u64 }
/// gsx_model_convert: gsx_extract_desc's filter and flags, and the pod kind of the new model (gsx_sh_kind / gsx_cov3d_kind as u32)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_convert_desc { pub filter: u32, pub flags: u32, pub sh: u32, pub cov3d: u32 }
/// one float32 per Gaussian (the functions take it as u32): stored position (world space with GSX_PROP_WORLD), the bytes of the colour
/// word / 255, their HSV, the scales gsx_model_export solves from the stored covariance
#[repr(u32)]
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum gsx_property { PosX = 0, PosY = 1, PosZ = 2, Red = 3, Green = 4, Blue = 5, Opacity = 6, Hue = 7, Saturation = 8, Value = 9, ScaleMax = 10, ScaleMid = 11, ScaleMin = 12 }
pub const GSX_PROP_COUNT: u32 = 13;
/// gsx_model_histogram: the property, GSX_PROP_WORLD | GSX_HIST_AUTO_RANGE, the GSX_BOUNDS_* filter, 1..=4096 bins over [lo, hi]; 24 bytes
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_histogram_desc { pub property: u32, pub flags: u32, pub filter: u32, pub bins: u32, pub lo: f32, pub hi: f32 }
/// the result of gsx_model_histogram, 48 bytes: counted (finite, passing the filter), below lo, above hi, NaN / inf; the range used; exact min / max
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_histogram_t { pub count: u64, pub below: u64, pub above: u64, pub n_nonfinite: u64, pub lo: f32, pub hi: f32, pub min: f32, pub max: f32 }
/// gsx_model_select_range, 40 bytes: hit = passes the filter, finite, lo <= value <= hi and (bins > 0) its bin in [bin_lo, bin_hi]
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_select_desc {
    pub property: u32, pub flags: u32, pub filter: u32, pub selection_op: u32, pub lo: f32, pub hi: f32,
    pub bins: u32, pub bin_lo: u32, pub bin_hi: u32, pub reserved: u32,
}
/// gsx_model_neighbors, 24 bytes: the GSX_BOUNDS_* filter, flags (0), the radius (model space), the cap 1..=4095 a count saturates at,
/// grid_bits (0: the library's hash table; 1..=24 forces 2^grid_bits buckets, no result changes)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_neighbor_desc { pub filter: u32, pub flags: u32, pub radius: f32, pub max_count: u32, pub grid_bits: u32, pub reserved: u32 }
/// the result of gsx_model_neighbors, 24 bytes: participants (pass the filter, finite position), those with a NaN / inf coordinate, the table used
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_neighbor_stats_t { pub count: u64, pub n_nonfinite: u64, pub grid_bits: u32, pub reserved: u32 }
/// gsx_model_select_neighbors, 40 bytes: hit = participates and count_lo <= min(neighbours, max_count) <= count_hi
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_neighbor_select_desc {
    pub filter: u32, pub flags: u32, pub selection_op: u32, pub max_count: u32, pub radius: f32,
    pub count_lo: u32, pub count_hi: u32, pub grid_bits: u32, pub reserved: [u32; 2],
}
/// gsx_model_clusters, 24 bytes: the GSX_BOUNDS_* filter, flags (0), the radius (model space), grid_bits (0: the library's hash table)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_cluster_desc { pub filter: u32, pub flags: u32, pub radius: f32, pub grid_bits: u32, pub reserved: [u32; 2] }
/// the result of gsx_model_clusters, 40 bytes: participants, those with a NaN / inf coordinate, the clusters, the largest one's size and
/// label (the smallest such label on a tie; GSX_CLUSTER_NONE without participants), the table used
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_cluster_stats_t {
    pub count: u64, pub n_nonfinite: u64, pub n_clusters: u64, pub largest_size: u64, pub largest_label: u32, pub grid_bits: u32,
}
/// gsx_model_select_clusters, 40 bytes: mode GSX_CLUSTER_BY_SIZE (size_lo <= the cluster's size <= size_hi), _LARGEST or _SEEDED (both 0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_cluster_select_desc {
    pub filter: u32, pub flags: u32, pub selection_op: u32, pub mode: u32, pub radius: f32,
    pub size_lo: u32, pub size_hi: u32, pub grid_bits: u32, pub reserved: [u32; 2],
}
/// gsx_model_knn, 32 bytes: the GSX_BOUNDS_* filter, flags (0), k 1..=16, the GSX_KNN_SCORE_* score, and three knobs that change no
/// result: radius_hint (0: the library's first search radius), grid_bits, max_rounds (0: the library's rule; 1..=64)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_knn_desc {
    pub filter: u32, pub flags: u32, pub k: u32, pub score: u32, pub radius_hint: f32, pub grid_bits: u32, pub max_rounds: u32, pub reserved: u32,
}
/// the result of gsx_model_knn, 72 bytes: participants, those with a NaN / inf coordinate, the finite scores' number, the Gaussians the
/// exact fallback answered, the scores' double mean and sample deviation, minimum and maximum, the first radius, the outlier threshold
/// (select, mode OUTLIERS; otherwise 0), the grid rounds, the table used
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_knn_stats_t {
    pub count: u64, pub n_nonfinite: u64, pub n_scored: u64, pub n_brute: u64, pub mean: f64, pub std: f64,
    pub score_min: f32, pub score_max: f32, pub first_radius: f32, pub threshold: f32, pub rounds: u32, pub grid_bits: u32,
}
/// gsx_model_select_knn, 48 bytes: mode GSX_KNN_SELECT_RANGE (lo <= score <= hi; std_ratio 0) or _OUTLIERS (score > mean + std_ratio *
/// std; lo and hi 0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_knn_select_desc {
    pub filter: u32, pub flags: u32, pub selection_op: u32, pub mode: u32, pub k: u32, pub score: u32, pub radius_hint: f32,
    pub grid_bits: u32, pub max_rounds: u32, pub lo: f32, pub hi: f32, pub std_ratio: f32,
}
/// gsx_model_nearest, 80 bytes: the GSX_BOUNDS_* filters of the queries and of the targets, flags (GSX_NEAREST_MODEL_TRANSFORMS),
/// max_distance (0: unlimited), the row-major 3x4 matrix from the source's model space into the targets', and three knobs that change
/// no result: radius_hint, grid_bits, max_rounds (gsx_knn_desc's)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_nearest_desc {
    pub src_filter: u32, pub dst_filter: u32, pub flags: u32, pub grid_bits: u32, pub max_distance: f32, pub radius_hint: f32,
    pub max_rounds: u32, pub reserved: u32, pub xform: [f32; 12],
}
/// the result of gsx_model_nearest, 136 bytes: participating queries and targets and the non-finite of both, the found queries, the
/// queries the exact fallback answered, the double mean distance (one-sided chamfer) and rms, the least and the largest distance
/// (one-sided Hausdorff), the first radius, the grid rounds, the table, the matrix used
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_nearest_stats_t {
    pub count: u64, pub n_nonfinite: u64, pub targets: u64, pub targets_nonfinite: u64, pub n_found: u64, pub n_brute: u64,
    pub mean: f64, pub rms: f64, pub d_min: f32, pub d_max: f32, pub first_radius: f32, pub rounds: u32, pub grid_bits: u32,
    pub reserved: u32, pub xform: [f32; 12],
}
/// gsx_model_select_nearest, 96 bytes: mode GSX_NEAREST_SELECT_RANGE (lo <= distance <= hi) or _TRANSFER (the nearest target is
/// selected; lo and hi 0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_nearest_select_desc { pub nearest: gsx_nearest_desc, pub selection_op: u32, pub mode: u32, pub lo: f32, pub hi: f32 }
/// gsx_model_align_step, 88 bytes: the search and flags (GSX_ALIGN_SCALE)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_align_desc { pub nearest: gsx_nearest_desc, pub flags: u32, pub reserved: u32 }
/// the result of gsx_model_align_step, 272 bytes: the delta t ~ scale R(quat) q + pos (quat x, y, z, w), xform_next = delta o the matrix
/// used, the pairs, the rms distance before the step, whether the step was degenerate, the search's statistics
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_align_step_t {
    pub pos: [f64; 3], pub quat: [f64; 4], pub scale: f64, pub xform_next: [f32; 12], pub n_pairs: u64, pub rms_before: f64,
    pub degenerate: u32, pub reserved: u32, pub nearest: gsx_nearest_stats_t,
}
/// gsx_model_apply_transform, 64 bytes: the GSX_BOUNDS_* filter, flags (GSX_EXTRACT_INVERT), the transform as
/// gsx_update_model_transform takes it (quat x, y, z, w), the pivot it rotates and scales about, reserved (0)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_transform_desc {
    pub filter: u32, pub flags: u32, pub pos: [f32; 3], pub quat: [f32; 4], pub scale: [f32; 3], pub pivot: [f32; 3], pub reserved: u32,
}
/// gsx_model_decimate, 24 bytes: the GSX_BOUNDS_* filter, flags (GSX_EXTRACT_INVERT), the cell edge (model space; must be set),
/// grid_bits (0: the library's hash table; 1..=24 forces 2^grid_bits buckets, no result changes), reserved (0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_decimate_desc { pub filter: u32, pub flags: u32, pub cell: f32, pub grid_bits: u32, pub reserved: [u32; 2] }
/// the result of gsx_model_decimate, 40 bytes: participants, kept Gaussians with a NaN / inf coordinate (dropped), occupied cells (the
/// new model's length), one-member cells, the largest member count, the table used
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_decimate_stats_t { pub count: u64, pub n_nonfinite: u64, pub cells: u64, pub singletons: u64, pub largest_cell: u32, pub grid_bits: u32 }
/// gsx_model_visibility, 16 bytes: flags (GSX_VIS_ACCUMULATE), reserved (0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_visibility_desc { pub flags: u32, pub reserved: [u32; 3] }
/// gsx_model_select_visibility, 32 bytes: the GSX_VIS_* measure, the GSX_BOUNDS_* filter, the selection op, reserved (0), the
/// inclusive range [lo, hi] of the resident measure (hi = +inf allowed)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_visibility_select_desc { pub measure: u32, pub filter: u32, pub selection_op: u32, pub reserved: u32, pub lo: f64, pub hi: f64 }
/// the result of gsx_model_visibility, 40 bytes: Gaussians after cull in this view, Gaussians with a resident peak > 0, the (pixel,
/// Gaussian) pairs blended in this view and the sum of their 2^-24 fixed-point weights, the largest resident peak, the views folded
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_visibility_stats_t { pub n_visible: u64, pub n_seen: u64, pub n_pairs: u64, pub weight_fixed: u64, pub peak_max: f32, pub views: u32 }
/// gsx_render_depth_map, 16 bytes: flags (GSX_DEPTH_MAP_NDC), the transmittance threshold of the surface (0.5: the median depth;
/// 1.0: the first record that lowers T at all), reserved (0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_depth_map_desc { pub flags: u32, pub threshold: f32, pub reserved: [u32; 2] }
/// the result of gsx_render_depth_map, 32 bytes: pixels with A > 0, pixels with a crossing, the smallest and largest surface over the
/// crossings (+inf and 0 without one), the number of models, reserved
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_depth_map_stats_t { pub n_covered: u64, pub n_crossed: u64, pub surface_min: f32, pub surface_max: f32, pub models: u32, pub reserved: u32 }
/// gsx_model_normals, 48 bytes: the GSX_BOUNDS_* filter, flags (0), k 3..=16, the GSX_NORMALS_ORIENT_* rule and its model-space point
/// `toward`, and gsx_knn_desc's three knobs that change no result
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_normals_desc {
    pub filter: u32, pub flags: u32, pub k: u32, pub orient: u32, pub radius_hint: f32, pub grid_bits: u32, pub max_rounds: u32, pub reserved: u32,
    pub toward: [f32; 3], pub reserved2: u32,
}
/// the result of gsx_model_normals, 64 bytes: participants, those with a NaN / inf coordinate, the fitted Gaussians, the Gaussians the
/// exact fallback answered, the variations' double mean, minimum and maximum, the first radius, the grid rounds, the table used
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_normals_stats_t {
    pub count: u64, pub n_nonfinite: u64, pub n_fitted: u64, pub n_brute: u64, pub mean: f64,
    pub variation_min: f32, pub variation_max: f32, pub first_radius: f32, pub rounds: u32, pub grid_bits: u32, pub reserved: u32,
}
/// gsx_model_select_normals, 80 bytes: mode GSX_NORMALS_SELECT_VARIATION (lo <= variation <= hi) or _FACING (lo <= the cosine between
/// the normal and `dir` <= hi; its absolute value with the flag GSX_NORMALS_ABS)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_normals_select_desc {
    pub filter: u32, pub flags: u32, pub selection_op: u32, pub mode: u32, pub k: u32, pub orient: u32, pub radius_hint: f32,
    pub grid_bits: u32, pub max_rounds: u32, pub lo: f32, pub hi: f32, pub reserved: u32, pub dir: [f32; 3], pub toward: [f32; 3],
    pub reserved2: [u32; 2],
}
/// gsx_model_normals_kept, 48 bytes: whether the model has kept normals, the k, orient, filter and toward they were made with, the
/// model's Gaussians then and how many of them have a plane
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_normals_kept_t {
    pub present: u32, pub k: u32, pub orient: u32, pub filter: u32, pub toward: [f32; 3], pub reserved: u32, pub count: u64, pub n_fitted: u64,
}
/// gsx_model_align_plane_step, 96 bytes: the search, flags (0) and the largest variation a target's plane may have (0: no limit)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_align_plane_desc { pub nearest: gsx_nearest_desc, pub flags: u32, pub max_variation: f32, pub reserved: [u32; 2] }
/// the result of gsx_model_align_plane_step, 568 bytes: the delta t ~ R(quat) q + pos (quat x, y, z, w), the upper triangle of the 6x6
/// normal matrix over (omega, tau), row-major, its right-hand side, its eigenvalues (descending), the centre, the pairs' rms distance
/// and rms distance along the normal before the step, the pairs used and left out, xform_next, the rank, degenerate, the search
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_align_plane_step_t {
    pub pos: [f64; 3], pub quat: [f64; 4], pub normal_matrix: [f64; 21], pub rhs: [f64; 6], pub eigenvalues: [f64; 6], pub centre: [f64; 3],
    pub rms_before: f64, pub rms_plane_before: f64, pub n_pairs: u64, pub n_unfitted: u64, pub xform_next: [f32; 12], pub rank: u32,
    pub degenerate: u32, pub nearest: gsx_nearest_stats_t,
}
/// a plane, 16 bytes: the points p with normal . p = offset (model space)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_plane_t { pub normal: [f32; 3], pub offset: f32 }
/// gsx_model_fit_plane, 64 bytes: the filter (GSX_BOUNDS_*), flags (GSX_EXTRACT_INVERT), sample (GSX_PLANE_SAMPLE_*), the candidates
/// (1 .. 1024), the seed, the inlier tolerance, min_cos (0: off), the refine rounds (0 .. 8), the sign rule of the refined normal
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_plane_fit_desc {
    pub filter: u32, pub flags: u32, pub sample: u32, pub n_candidates: u32, pub seed: u64, pub tolerance: f32, pub min_cos: f32,
    pub refine_iters: u32, pub orient: u32, pub toward: [f32; 3], pub reserved: [u32; 3],
}
/// the result of gsx_model_fit_plane, 208 bytes: the plane, the winning candidate and its index (GSX_PLANE_NONE without one), the valid
/// candidates, the participants, the filtered Gaussians without a finite position, the candidate's and the plane's inliers, and of the
/// last accepted refine round the centroid, the eigenvalues (descending), the rms residual and the sums (sum p, the scatter xx xy xz yy
/// yz zz, sum r^2); the rounds accepted; degenerate
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_plane_fit_t {
    pub plane: gsx_plane_t, pub candidate: gsx_plane_t, pub winner: u32, pub n_valid: u32, pub count: u64, pub n_nonfinite: u64,
    pub candidate_inliers: u64, pub n_inliers: u64, pub centroid: [f32; 3], pub refine_done: u32, pub eigenvalues: [f64; 3], pub rms: f64,
    pub sums: [f64; 10], pub degenerate: u32, pub reserved: u32,
}
/// gsx_model_select_plane, 48 bytes: the plane, the signed residual's range (a bound may be infinite), min_cos, the filter, the op
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_plane_select_desc {
    pub plane: gsx_plane_t, pub lo: f32, pub hi: f32, pub min_cos: f32, pub filter: u32, pub selection_op: u32, pub reserved: [u32; 3],
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_query { pub kind: u32, pub selection_op: u32, pub p0: [f32; 2], pub p1: [f32; 2], pub radius: f32, pub reserved: u32 }
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_query_hit { pub index: u32, pub depth: f32, pub alpha: f32, pub reserved: u32 } // gs::QueryHitResultPod
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_shard_layout_t {
    pub rows_per_rank: u32, pub row_lo: u32, pub row_hi: u32,
    pub band_bytes: u64, pub band_offset_bytes: u64, pub padded_framebuffer_bytes: u64,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_shard_verdict { pub need_tiles: u32, pub overflow: u32, pub max_records: u32, pub reserved: u32 }
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_ply_header { pub count: u64, pub header_bytes: u64, pub vertex_bytes: u32, pub is_ascii: u32, pub offsets: [i32; 62] }
/// opaque: an in-process group of viewers, one per GPU (gsx_comm_group_create)
#[repr(C)]
pub struct gsx_comm_group {
    _private: [u8; 0],
}
/// opaque: a ref-counted handle on a snapshot of one of a model's per-Gaussian buffers (gs:: buffers are `Clone`, src/app.rs:769-780)
#[repr(C)]
pub struct gsx_buffer {
    _private: [u8; 0],
}
#[repr(i32)]
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum gsx_buffer_kind { Mask = 0, Edits = 1, Selection = 2 }
#[repr(i32)]
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum gsx_depth_compare { Always = 0, Less = 1 } // the compare of new_with's depth_stencil, src/tab/scene.rs:1969-1980
#[repr(u32)]
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum gsx_toolset_tool { Rect = 0, Brush = 1 } // gs::QueryToolsetTool, src/tab/scene.rs:1258-1264 (the functions take it as u32)
/// the app's measurement `HitPair` (src/renderer/measurement.rs:177-184), 32 bytes: world-space ends, RGBA8 colour, width
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_overlay_line { pub p0: [f32; 3], pub color: [u8; 4], pub p1: [f32; 3], pub line_width: f32 }
/// a mask shape's gizmo (gs::MaskGizmo; src/tab/scene.rs:2211-2247), 64 bytes: a world-space `gs::MaskShape` (kind 0 box / 1 ellipsoid),
/// its straight RGBA colour in [0, 1] and a width in `gsx_overlay_line::line_width` units
#[repr(C)]
#[derive(Clone, Copy)]
pub struct gsx_mask_gizmo { pub kind: u32, pub pos: [f32; 3], pub quat_xyzw: [f32; 4], pub scale: [f32; 3], pub color: [f32; 4], pub line_width: f32 }
/// the two collectives of a caller-supplied transport: they ENQUEUE on `hip_stream` and return 0 or a gsx_status
pub type gsx_comm_all_to_all_fn = Option<unsafe extern "C" fn(ctx: *mut c_void, d_send: *const c_void, d_recv: *mut c_void, bytes_per_peer: u64, hip_stream: *mut c_void) -> gsx_status>;
pub type gsx_comm_all_gather_fn = Option<unsafe extern "C" fn(ctx: *mut c_void, d_send: *const c_void, d_recv: *mut c_void, bytes_per_rank: u64, hip_stream: *mut c_void) -> gsx_status>;
/// ... and of a transport that moves pieces of unequal size (arrays of `world` byte offsets / sizes)
pub type gsx_comm_all_to_all_v_fn = Option<unsafe extern "C" fn(ctx: *mut c_void, d_send: *const c_void, send_offsets: *const u64, send_bytes: *const u64, d_recv: *mut c_void, recv_offsets: *const u64, recv_bytes: *const u64, hip_stream: *mut c_void) -> gsx_status>;
pub type gsx_comm_gather_v_fn = Option<unsafe extern "C" fn(ctx: *mut c_void, d_send: *const c_void, send_bytes: u64, d_recv: *mut c_void, recv_offsets: *const u64, recv_bytes: *const u64, root: i32, hip_stream: *mut c_void) -> gsx_status>;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_shard_stats {
    pub frames: u64, pub redo_frames: u64, pub repair_frames: u64, pub exchange_rounds: u64,
    pub wire_bytes: u64, pub verdict_wait_ns: u64, pub last_slot_records: u32, pub last_repair_slot_records: u32,
    pub last_entries_sum: u32, pub last_entries_max: u32, pub last_work_permille: u32, pub redo_fallbacks: u32,
    pub last_repair_records: u32, pub reserved0: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_comm_info { pub transport: u32, pub nranks: u32, pub rank: u32, pub lane_comms: u32, pub device: i32, pub version: i32 }
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct gsx_launch_stats {
    pub graph_launches: u64, pub graph_nodes: u64, pub nodes_patched: u64, pub direct_launches: u64, pub graphs_built: u64, pub broken: u64, pub idle_direct_scopes: u64,
}
pub type gsx_pass = u32; // 0 project, 1 depth sort, 2 bin, 3 tile sort, 4 composite, 5 project (geometry only), 6 shade
pub const GSX_PASS_COUNT: usize = 7;

#[link(name = "gsx")]
extern "C" {
    pub fn gsx_last_error_string() -> *const c_char;
    pub fn gsx_abi_version() -> u32;
    pub fn gsx_spec_params_default(out: *mut gsx_spec_params);
    pub fn gsx_viewer_create(desc: *const gsx_viewer_desc, out: *mut *mut gsx_viewer) -> gsx_status;
    pub fn gsx_viewer_destroy(v: *mut gsx_viewer);
    pub fn gsx_viewer_set_spec_params(v: *mut gsx_viewer, p: *const gsx_spec_params) -> gsx_status;
    pub fn gsx_render_options_default(out: *mut gsx_render_options);
    pub fn gsx_viewer_set_render_options(v: *mut gsx_viewer, o: *const gsx_render_options) -> gsx_status;
    pub fn gsx_model_create(v: *mut gsx_viewer, key: *const c_char, count: u64, sh: gsx_sh_kind, cov3d: gsx_cov3d_kind) -> gsx_status;
    pub fn gsx_model_remove(v: *mut gsx_viewer, key: *const c_char) -> gsx_status;
    pub fn gsx_model_len(v: *mut gsx_viewer, key: *const c_char, out_count: *mut u64) -> gsx_status;
    pub fn gsx_model_upload_range(v: *mut gsx_viewer, key: *const c_char, start: u64, src: *const gsx_gaussian, n: u64) -> gsx_status;
    pub fn gsx_model_upload_pod_device(v: *mut gsx_viewer, key: *const c_char, start: u64, n: u64, d_pos: *const f32, d_color: *const u32, d_sh: *const f32, d_cov3d: *const f32) -> gsx_status;
    pub fn gsx_update_camera(v: *mut gsx_viewer, view: *const f32, proj: *const f32, width: u32, height: u32) -> gsx_status;
    pub fn gsx_update_model_transform(v: *mut gsx_viewer, key: *const c_char, pos: *const f32, quat_xyzw: *const f32, scale: *const f32) -> gsx_status;
    pub fn gsx_update_gaussian_transform(v: *mut gsx_viewer, size: f32, mode: gsx_display_mode, sh_deg: u32, no_sh0: u32) -> gsx_status;
    pub fn gsx_model_upload_mask(v: *mut gsx_viewer, key: *const c_char, words: *const u32, n_words: u64) -> gsx_status;
    pub fn gsx_model_download_mask(v: *mut gsx_viewer, key: *const c_char, words: *mut u32, n_words: u64) -> gsx_status;
    pub fn gsx_mask_evaluate(v: *mut gsx_viewer, key: *const c_char, ops: *const gsx_mask_op, n_ops: u32, shapes: *const gsx_mask_shape, n_shapes: u32) -> gsx_status;
    pub fn gsx_preprocess(v: *mut gsx_viewer, key: *const c_char) -> gsx_status;
    pub fn gsx_sort(v: *mut gsx_viewer, key: *const c_char) -> gsx_status;
    pub fn gsx_sync(v: *mut gsx_viewer) -> gsx_status;
    pub fn gsx_render(v: *mut gsx_viewer, keys_far_to_near: *const *const c_char, n_keys: u32) -> gsx_status;
    pub fn gsx_render_frame(v: *mut gsx_viewer, keys_far_to_near: *const *const c_char, n_keys: u32) -> gsx_status;
    pub fn gsx_viewer_set_depth_test(v: *mut gsx_viewer, compare: gsx_depth_compare) -> gsx_status;
    pub fn gsx_viewer_set_depth_buffer_device(v: *mut gsx_viewer, d_ptr: *const f32, width: u32, height: u32, row_pitch_bytes: u64) -> gsx_status;
    pub fn gsx_viewer_upload_depth_buffer(v: *mut gsx_viewer, host: *const f32, width: u32, height: u32) -> gsx_status;
    pub fn gsx_viewer_set_overlay_lines(v: *mut gsx_viewer, lines: *const gsx_overlay_line, n: u32) -> gsx_status;
    pub fn gsx_viewer_set_mask_gizmos(v: *mut gsx_viewer, gizmos: *const gsx_mask_gizmo, n: u32) -> gsx_status;
    pub fn gsx_download_overlay(v: *mut gsx_viewer, rgba: *mut f32, depth: *mut f32) -> gsx_status;
    pub fn gsx_overlay_device_ptrs(v: *mut gsx_viewer, rgba: *mut *mut c_void, tile_flags: *mut *mut c_void, depth: *mut *mut c_void) -> gsx_status;
    pub fn gsx_download_framebuffer(v: *mut gsx_viewer, rgbt: *mut f32, n_floats: u64) -> gsx_status;
    pub fn gsx_download_rgba8(v: *mut gsx_viewer, background_rgb: *const f32, rgba: *mut u8, n_bytes: u64) -> gsx_status;
    pub fn gsx_framebuffer_device_ptr(v: *mut gsx_viewer, out_ptr: *mut *mut c_void, out_w: *mut u32, out_h: *mut u32) -> gsx_status;
    pub fn gsx_model_frame_stats(v: *mut gsx_viewer, key: *const c_char, out: *mut gsx_frame_stats) -> gsx_status;
    pub fn gsx_model_download_projection(v: *mut gsx_viewer, key: *const c_char, depth_key: *mut u32, rect: *mut u32, mean2d: *mut f32, conic_opacity: *mut f32, rgb: *mut f32) -> gsx_status;
    pub fn gsx_model_download_sorted(v: *mut gsx_viewer, key: *const c_char, indices: *mut u32, capacity: u64, out_n_visible: *mut u64) -> gsx_status;
    pub fn gsx_model_download_tile_lists(v: *mut gsx_viewer, key: *const c_char, tile_offsets: *mut u32, n_offsets: u64, list: *mut u32, capacity: u64) -> gsx_status;
    pub fn gsx_model_download_pod(v: *mut gsx_viewer, key: *const c_char, pos: *mut f32, color: *mut u32, sh: *mut f32, cov3d: *mut f32) -> gsx_status;
    pub fn gsx_bounds_desc_default(d: *mut gsx_bounds_desc);
    pub fn gsx_model_bounds(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_bounds_desc, out: *mut gsx_model_bounds_t) -> gsx_status;
    pub fn gsx_extract_desc_default(d: *mut gsx_extract_desc);
    pub fn gsx_model_extract(v: *mut gsx_viewer, src_key: *const c_char, dst_key: *const c_char, desc: *const gsx_extract_desc, out_count: *mut u64) -> gsx_status;
    pub fn gsx_model_merge(v: *mut gsx_viewer, src_keys: *const *const c_char, n_src: u32, dst_key: *const c_char, desc: *const gsx_extract_desc, out_counts: *mut u64, out_total: *mut u64) -> gsx_status;
    pub fn gsx_export_desc_default(d: *mut gsx_export_desc);
    pub fn gsx_model_export(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_export_desc, out: *mut c_void, capacity_bytes: u64, out_count: *mut u64) -> gsx_status;
    pub fn gsx_model_export_ply(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_export_desc, out: *mut c_void, capacity: u64, out_size: *mut u64) -> gsx_status;
    pub fn gsx_import_desc_default(d: *mut gsx_import_desc);
    pub fn gsx_model_upload_ply_rows(v: *mut gsx_viewer, key: *const c_char, start: u64, rows: *const c_void, n: u64, header: *const gsx_ply_header, desc: *const gsx_import_desc) -> gsx_status;
    pub fn gsx_model_import_ply(v: *mut gsx_viewer, key: *const c_char, data: *const c_void, size: u64, sh: gsx_sh_kind, cov3d: gsx_cov3d_kind, desc: *const gsx_import_desc, out_count: *mut u64) -> gsx_status;
    pub fn gsx_model_pod_kind(v: *mut gsx_viewer, key: *const c_char, out_sh: *mut gsx_sh_kind, out_cov3d: *mut gsx_cov3d_kind) -> gsx_status;
    pub fn gsx_convert_desc_default(d: *mut gsx_convert_desc);
    pub fn gsx_model_convert(v: *mut gsx_viewer, src_key: *const c_char, dst_key: *const c_char, desc: *const gsx_convert_desc, out_count: *mut u64) -> gsx_status;
    pub fn gsx_model_set_pod_kind(v: *mut gsx_viewer, key: *const c_char, sh: gsx_sh_kind, cov3d: gsx_cov3d_kind) -> gsx_status;
    pub fn gsx_model_property_values(v: *mut gsx_viewer, key: *const c_char, property: u32, flags: u32, out: *mut f32, n: u64) -> gsx_status;
    pub fn gsx_model_histogram(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_histogram_desc, out_bins: *mut u64, out: *mut gsx_histogram_t) -> gsx_status;
    pub fn gsx_model_select_range(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_select_desc, out_hit: *mut u64, out_selected: *mut u64) -> gsx_status;
    pub fn gsx_neighbor_desc_default(d: *mut gsx_neighbor_desc);
    pub fn gsx_model_neighbors(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_neighbor_desc, out_counts: *mut u32, out_hist: *mut u64, out: *mut gsx_neighbor_stats_t) -> gsx_status;
    pub fn gsx_model_select_neighbors(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_neighbor_select_desc, out_hit: *mut u64, out_selected: *mut u64) -> gsx_status;
    pub fn gsx_cluster_desc_default(d: *mut gsx_cluster_desc);
    pub fn gsx_model_clusters(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_cluster_desc, out_labels: *mut u32, out_sizes: *mut u32, out: *mut gsx_cluster_stats_t) -> gsx_status;
    pub fn gsx_model_select_clusters(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_cluster_select_desc, out_hit: *mut u64, out_selected: *mut u64) -> gsx_status;
    pub fn gsx_knn_desc_default(d: *mut gsx_knn_desc);
    pub fn gsx_model_knn(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_knn_desc, out_d2: *mut f32, out_score: *mut f32, out: *mut gsx_knn_stats_t) -> gsx_status;
    pub fn gsx_model_select_knn(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_knn_select_desc, out_hit: *mut u64, out_selected: *mut u64, out_stats: *mut gsx_knn_stats_t) -> gsx_status;
    pub fn gsx_nearest_desc_default(d: *mut gsx_nearest_desc);
    pub fn gsx_model_nearest(v: *mut gsx_viewer, src_key: *const c_char, dst_key: *const c_char, desc: *const gsx_nearest_desc, out_index: *mut u32, out_d2: *mut f32, out: *mut gsx_nearest_stats_t) -> gsx_status;
    pub fn gsx_model_select_nearest(v: *mut gsx_viewer, src_key: *const c_char, dst_key: *const c_char, desc: *const gsx_nearest_select_desc, out_hit: *mut u64, out_selected: *mut u64, out_stats: *mut gsx_nearest_stats_t) -> gsx_status;
    pub fn gsx_model_align_step(v: *mut gsx_viewer, src_key: *const c_char, dst_key: *const c_char, desc: *const gsx_align_desc, out: *mut gsx_align_step_t) -> gsx_status;
    pub fn gsx_transform_desc_default(d: *mut gsx_transform_desc);
    pub fn gsx_model_apply_transform(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_transform_desc, out_count: *mut u64) -> gsx_status;
    pub fn gsx_decimate_desc_default(d: *mut gsx_decimate_desc);
    pub fn gsx_model_decimate(v: *mut gsx_viewer, src_key: *const c_char, dst_key: *const c_char, desc: *const gsx_decimate_desc, out_map: *mut u32, out: *mut gsx_decimate_stats_t) -> gsx_status;
    pub fn gsx_model_decimate_edge(v: *mut gsx_viewer, key: *const c_char, filter: u32, flags: u32, target_cells: u64, out_cell: *mut f32, out_cells: *mut u64) -> gsx_status;
    pub fn gsx_visibility_desc_default(d: *mut gsx_visibility_desc);
    pub fn gsx_visibility_select_desc_default(d: *mut gsx_visibility_select_desc);
    pub fn gsx_model_visibility(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_visibility_desc, out_peak: *mut f32, out_weight: *mut f64, out_pixels: *mut u32, out_transmittance: *mut f32, out: *mut gsx_visibility_stats_t) -> gsx_status;
    pub fn gsx_model_select_visibility(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_visibility_select_desc, out_hit: *mut u64, out_selected: *mut u64) -> gsx_status;
    pub fn gsx_model_visibility_reset(v: *mut gsx_viewer, key: *const c_char) -> gsx_status;
    pub fn gsx_depth_map_desc_default(d: *mut gsx_depth_map_desc);
    pub fn gsx_render_depth_map(v: *mut gsx_viewer, keys_far_to_near: *const *const c_char, n_keys: u32, desc: *const gsx_depth_map_desc, out_surface: *mut f32, out_sum: *mut f32, out_alpha: *mut f32, out_transmittance: *mut f32, out_index: *mut u32, out_layer: *mut u32, out: *mut gsx_depth_map_stats_t) -> gsx_status;
    pub fn gsx_depth_map_device_ptrs(v: *mut gsx_viewer, surface: *mut *mut c_void, sum: *mut *mut c_void, alpha: *mut *mut c_void, transmittance: *mut *mut c_void, index: *mut *mut c_void, layer: *mut *mut c_void, ndc: *mut *mut c_void, width: *mut u32, height: *mut u32) -> gsx_status;
    pub fn gsx_depth_map_unproject(view: *const f32, proj: *const f32, width: u32, height: u32, px: f32, py: f32, view_depth: f32, out_world: *mut f32) -> gsx_status;
    pub fn gsx_normals_desc_default(d: *mut gsx_normals_desc);
    pub fn gsx_model_normals(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_normals_desc, out_normal: *mut f32, out_variation: *mut f32, out_index: *mut u32, out: *mut gsx_normals_stats_t) -> gsx_status;
    pub fn gsx_model_select_normals(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_normals_select_desc, out_hit: *mut u64, out_selected: *mut u64, out_stats: *mut gsx_normals_stats_t) -> gsx_status;
    pub fn gsx_model_normals_keep(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_normals_desc, out: *mut gsx_normals_stats_t) -> gsx_status;
    pub fn gsx_model_normals_kept(v: *mut gsx_viewer, key: *const c_char, out: *mut gsx_normals_kept_t, out_normal: *mut f32, out_variation: *mut f32) -> gsx_status;
    pub fn gsx_model_normals_reset(v: *mut gsx_viewer, key: *const c_char) -> gsx_status;
    pub fn gsx_model_align_plane_step(v: *mut gsx_viewer, src_key: *const c_char, dst_key: *const c_char, desc: *const gsx_align_plane_desc, out: *mut gsx_align_plane_step_t) -> gsx_status;
    pub fn gsx_plane_fit_desc_default(desc: *mut gsx_plane_fit_desc);
    pub fn gsx_plane_select_desc_default(desc: *mut gsx_plane_select_desc);
    pub fn gsx_model_fit_plane(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_plane_fit_desc, candidates: *const gsx_plane_t, out_candidates: *mut gsx_plane_t, out_counts: *mut u32, out: *mut gsx_plane_fit_t) -> gsx_status;
    pub fn gsx_model_select_plane(v: *mut gsx_viewer, key: *const c_char, desc: *const gsx_plane_select_desc, out_hit: *mut u64, out_selected: *mut u64) -> gsx_status;
    pub fn gsx_plane_level(plane: *const gsx_plane_t, up: *const f32, quat_xyzw: *mut f32, pos: *mut f32) -> gsx_status;
    pub fn gsx_gaussian_edit_default(e: *mut gsx_gaussian_edit);
    pub fn gsx_update_query(v: *mut gsx_viewer, q: *const gsx_query) -> gsx_status;
    pub fn gsx_update_query_texture(v: *mut gsx_viewer, texels: *const u8, width: u32, height: u32) -> gsx_status;
    pub fn gsx_update_selection_highlight(v: *mut gsx_viewer, rgba: *const f32) -> gsx_status;
    pub fn gsx_update_selection_edit(v: *mut gsx_viewer, e: *const gsx_gaussian_edit) -> gsx_status;
    pub fn gsx_model_show_unedited(v: *mut gsx_viewer, key: *const c_char, on: u32) -> gsx_status;
    pub fn gsx_postprocess(v: *mut gsx_viewer, key: *const c_char) -> gsx_status;
    pub fn gsx_model_upload_selection(v: *mut gsx_viewer, key: *const c_char, words: *const u32, n_words: u64) -> gsx_status;
    pub fn gsx_model_download_selection(v: *mut gsx_viewer, key: *const c_char, words: *mut u32, n_words: u64) -> gsx_status;
    pub fn gsx_model_download_edits(v: *mut gsx_viewer, key: *const c_char, out: *mut gsx_gaussian_edit, n: u64) -> gsx_status;
    pub fn gsx_model_upload_edits(v: *mut gsx_viewer, key: *const c_char, edits: *const gsx_gaussian_edit, n: u64) -> gsx_status;
    pub fn gsx_query_download_hits(v: *mut gsx_viewer, key: *const c_char, out: *mut gsx_query_hit, capacity: u64, out_n: *mut u64) -> gsx_status;
    pub fn gsx_query_hit_pos_by_closest(hits: *const gsx_query_hit, n: u64, view: *const f32, proj: *const f32, width: u32, height: u32, coords: *const f32, out_index: *mut u32, out_pos: *mut f32) -> gsx_status;
    pub fn gsx_query_hit_pos_by_alpha_range(hits: *const gsx_query_hit, n: u64, view: *const f32, proj: *const f32, width: u32, height: u32, coords: *const f32, range: f32, out_index: *mut u32, out_alpha: *mut f32, out_pos: *mut f32) -> gsx_status;
    pub fn gsx_toolset_set_use_texture(v: *mut gsx_viewer, on: u32) -> gsx_status;
    pub fn gsx_toolset_update_brush_radius(v: *mut gsx_viewer, radius: f32) -> gsx_status;
    pub fn gsx_toolset_start(v: *mut gsx_viewer, tool: u32, selection_op: u32, pos: *const f32) -> gsx_status;
    pub fn gsx_toolset_update_pos(v: *mut gsx_viewer, pos: *const f32) -> gsx_status;
    pub fn gsx_toolset_end(v: *mut gsx_viewer) -> gsx_status;
    pub fn gsx_toolset_query(v: *mut gsx_viewer, out: *mut gsx_query) -> gsx_status;
    pub fn gsx_toolset_state(v: *mut gsx_viewer, active: *mut u32, tool: *mut u32, selection_op: *mut u32, start: *mut f32, pos: *mut f32) -> gsx_status;
    pub fn gsx_toolset_render(v: *mut gsx_viewer) -> gsx_status;
    pub fn gsx_toolset_set_overlay(v: *mut gsx_viewer, texture_rgba: *const f32, cursor_rgba: *const f32, cursor_thickness: f32) -> gsx_status;
    pub fn gsx_download_query_texture(v: *mut gsx_viewer, texels: *mut u8, width: u32, height: u32) -> gsx_status;
    pub fn gsx_model_buffer_retain(v: *mut gsx_viewer, key: *const c_char, kind: gsx_buffer_kind, out: *mut *mut gsx_buffer) -> gsx_status;
    pub fn gsx_buffer_retain(b: *mut gsx_buffer) -> gsx_status;
    pub fn gsx_buffer_release(b: *mut gsx_buffer);
    pub fn gsx_buffer_len(b: *mut gsx_buffer, out_elements: *mut u64) -> gsx_status;
    pub fn gsx_buffer_download(b: *mut gsx_buffer, out: *mut c_void, n_elements: u64) -> gsx_status;
    pub fn gsx_shard_layout(v: *mut gsx_viewer, world: u32, rank: u32, out: *mut gsx_shard_layout_t) -> gsx_status;
    pub fn gsx_viewer_set_band(v: *mut gsx_viewer, row_lo: u32, row_hi: u32) -> gsx_status;
    pub fn gsx_viewer_set_external_framebuffer(v: *mut gsx_viewer, d_ptr: *mut c_void, bytes: u64) -> gsx_status;
    pub fn gsx_resolve_rgba8_device(v: *mut gsx_viewer, background_rgb: *const f32, y0: u32, y1: u32, d_rgba: *mut c_void) -> gsx_status;
    pub fn gsx_shard_pack(v: *mut gsx_viewer, key: *const c_char, world: u32, d_tile_window: *const u32, d_send: *mut c_void, capacity_records: u64, counts: *mut u64) -> gsx_status;
    pub fn gsx_shard_set_windows(v: *mut gsx_viewer, key: *const c_char, d_tile_window: *const u32) -> gsx_status;
    pub fn gsx_shard_import(v: *mut gsx_viewer, key: *const c_char, d_recv: *const c_void, n_records: u64, world: u32, rank: u32, d_tile_window: *const u32) -> gsx_status;
    pub fn gsx_shard_feedback_words(v: *mut gsx_viewer, world: u32, out_words: *mut u32) -> gsx_status;
    pub fn gsx_shard_feedback(v: *mut gsx_viewer, key: *const c_char, world: u32, rank: u32, d_out_u32: *mut c_void) -> gsx_status;
    pub fn gsx_render_more(v: *mut gsx_viewer, keys: *const *const c_char, n_keys: u32) -> gsx_status;
    pub fn gsx_shard_frame_begin(v: *mut gsx_viewer, key: *const c_char, world: u32, rank: u32, speculate: u32, d_limit_override: *const u32) -> gsx_status;
    pub fn gsx_shard_slot_records(v: *mut gsx_viewer, key: *const c_char, world: u32, shard_records_max: u32, out_records: *mut u32) -> gsx_status;
    pub fn gsx_shard_pack_slots(v: *mut gsx_viewer, key: *const c_char, world: u32, round: u32, d_send: *mut c_void, slot_records: u32) -> gsx_status;
    pub fn gsx_shard_import_slots(v: *mut gsx_viewer, key: *const c_char, d_recv: *const c_void, world: u32, rank: u32, round: u32, slot_records: u32) -> gsx_status;
    pub fn gsx_shard_verify(v: *mut gsx_viewer, key: *const c_char, world: u32, d_sat_all: *const c_void, out_seq: *mut u32) -> gsx_status;
    pub fn gsx_shard_wait_verdict(v: *mut gsx_viewer, key: *const c_char, seq: u32, out: *mut gsx_shard_verdict) -> gsx_status;
    pub fn gsx_shard_repair_count(v: *mut gsx_viewer, key: *const c_char, world: u32, d_out4: *mut c_void) -> gsx_status;
    pub fn gsx_shard_post_counts(v: *mut gsx_viewer, world: u32, d_counts_all: *const c_void, out_seq: *mut u32) -> gsx_status;
    pub fn gsx_shard_next_windows(v: *mut gsx_viewer, key: *const c_char, world: u32, d_sat_all: *const c_void, margin: f32, radius: u32) -> gsx_status;
    pub fn gsx_shard_frame_end(v: *mut gsx_viewer, key: *const c_char) -> gsx_status;
    pub fn gsx_shard_download_limits(v: *mut gsx_viewer, key: *const c_char, limits: *mut u32, n_words: u64) -> gsx_status;
    pub fn gsx_comm_unique_id(out_id: *mut u8) -> gsx_status;
    pub fn gsx_viewer_comm_init(v: *mut gsx_viewer, world: u32, rank: u32, id: *const u8) -> gsx_status;
    pub fn gsx_viewer_comm_destroy(v: *mut gsx_viewer) -> gsx_status;
    pub fn gsx_viewer_comm_info(v: *mut gsx_viewer, out: *mut gsx_comm_info) -> gsx_status;
    pub fn gsx_comm_all_to_all(v: *mut gsx_viewer, d_send: *const c_void, d_recv: *mut c_void, bytes_per_peer: u64) -> gsx_status;
    pub fn gsx_comm_all_gather(v: *mut gsx_viewer, d_send: *const c_void, d_recv: *mut c_void, bytes_per_rank: u64) -> gsx_status;
    pub fn gsx_shard_render_frame(v: *mut gsx_viewer, key: *const c_char, shard_records_max: u32, speculate: u32, margin: f32, radius: u32) -> gsx_status;
    pub fn gsx_shard_render_frame_keys(v: *mut gsx_viewer, keys_far_to_near: *const *const c_char, n_keys: u32, shard_records_max: *const u32, speculate: u32, margin: f32, radius: u32) -> gsx_status;
    pub fn gsx_comm_group_create(world: u32, timeout_ms: u32, out: *mut *mut gsx_comm_group) -> gsx_status;
    pub fn gsx_comm_group_destroy(g: *mut gsx_comm_group);
    pub fn gsx_viewer_comm_init_group(v: *mut gsx_viewer, g: *mut gsx_comm_group, rank: u32) -> gsx_status;
    pub fn gsx_viewer_comm_init_custom(v: *mut gsx_viewer, world: u32, rank: u32, all_to_all: gsx_comm_all_to_all_fn, all_gather: gsx_comm_all_gather_fn, ctx: *mut c_void) -> gsx_status;
    pub fn gsx_viewer_comm_init_custom_v(v: *mut gsx_viewer, world: u32, rank: u32, all_to_all_v: gsx_comm_all_to_all_v_fn, gather_v: gsx_comm_gather_v_fn, ctx: *mut c_void) -> gsx_status;
    pub fn gsx_shard_set_band_edges(v: *mut gsx_viewer, world: u32, edges: *const u32) -> gsx_status;
    pub fn gsx_shard_get_band_edges(v: *mut gsx_viewer, world: u32, out_edges: *mut u32) -> gsx_status;
    pub fn gsx_shard_set_balance(v: *mut gsx_viewer, enabled: u32) -> gsx_status;
    pub fn gsx_shard_set_limits(v: *mut gsx_viewer, key: *const c_char, limits: *const u32) -> gsx_status;
    pub fn gsx_shard_set_slot_records(v: *mut gsx_viewer, key: *const c_char, records: u32) -> gsx_status;
    pub fn gsx_shard_get_stats(v: *mut gsx_viewer, out: *mut gsx_shard_stats, reset: u32) -> gsx_status;
    pub fn gsx_shard_set_gather_root(v: *mut gsx_viewer, root: i32) -> gsx_status;
    pub fn gsx_ply_read_header(data: *const c_void, size: u64, out: *mut gsx_ply_header) -> gsx_status;
    pub fn gsx_ply_read_gaussians(data: *const c_void, size: u64, header: *const gsx_ply_header, start: u64, n: u64, out: *mut gsx_gaussian) -> gsx_status;
    pub fn gsx_ply_write(gaussians: *const gsx_gaussian, n: u64, mask_words: *const u32, edits: *const gsx_gaussian_edit, out: *mut c_void, capacity: u64, out_size: *mut u64) -> gsx_status;
    pub fn gsx_debug_set_radix_rank_mode(mode: i32);
    pub fn gsx_debug_set_launch_graphs(enabled: i32);
    pub fn gsx_debug_launch_count() -> u64;
    pub fn gsx_debug_device_bytes() -> u64;
    pub fn gsx_debug_download_lane_framebuffer(v: *mut gsx_viewer, lane: u32, rgbt: *mut f32, n_floats: u64) -> gsx_status;
    pub fn gsx_debug_tile_profile(v: *mut gsx_viewer, out4: *mut u32, n_tiles: u64) -> gsx_status;
    pub fn gsx_viewer_launch_stats(v: *mut gsx_viewer, out: *mut gsx_launch_stats, reset: u32) -> gsx_status;
    pub fn gsx_set_pass_timing(v: *mut gsx_viewer, enabled: u32) -> gsx_status;
    pub fn gsx_get_pass_timing(v: *mut gsx_viewer, ms: *mut f32, launches: *mut u32) -> gsx_status;
}
