"""ctypes binding of libgsx.so (include/gsx.h).  The library is the product; this file is plumbing.

The shared object is built in-tree by ``__graft_entry__.build()`` (``make -C csrc``).  If it is missing
the import of the product path FAILS LOUDLY — there is no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsx.so")

GSX_ABI_VERSION = 3
(GSX_OK, GSX_ERR_INVALID_ARG, GSX_ERR_OOM, GSX_ERR_HIP, GSX_ERR_RCCL, GSX_ERR_IO, GSX_ERR_PLY, GSX_ERR_NOT_FOUND,
 GSX_ERR_UNSUPPORTED, GSX_ERR_NO_DEVICE) = range(10)
GSX_PASS_NAMES = ("project", "depth_sort", "bin", "tile_sort", "composite", "project_geom", "shade")
GSX_PASS_COUNT = len(GSX_PASS_NAMES)

#: every symbol include/gsx.h declares (tests check the library exports exactly these)
EXPORTS = (
    "gsx_last_error_string", "gsx_abi_version", "gsx_spec_params_default", "gsx_viewer_create", "gsx_viewer_destroy",
    "gsx_viewer_set_spec_params", "gsx_model_create", "gsx_model_remove", "gsx_model_len", "gsx_model_upload_range",
    "gsx_model_upload_pod_device", "gsx_update_camera", "gsx_update_model_transform", "gsx_update_gaussian_transform",
    "gsx_model_upload_mask", "gsx_model_download_mask", "gsx_preprocess", "gsx_sort", "gsx_sync", "gsx_render",
    "gsx_render_frame", "gsx_download_framebuffer", "gsx_download_rgba8", "gsx_framebuffer_device_ptr",
    "gsx_model_frame_stats", "gsx_model_download_projection", "gsx_model_download_sorted",
    "gsx_model_download_tile_lists", "gsx_model_download_pod", "gsx_set_pass_timing", "gsx_get_pass_timing",
    "gsx_mask_evaluate", "gsx_ply_read_header", "gsx_ply_read_gaussians", "gsx_ply_write", "gsx_render_options_default", "gsx_viewer_set_render_options", "gsx_shard_layout", "gsx_viewer_set_external_framebuffer", "gsx_shard_pack", "gsx_shard_import", "gsx_shard_feedback_words", "gsx_shard_feedback", "gsx_shard_set_windows", "gsx_viewer_set_band", "gsx_resolve_rgba8_device",
    "gsx_render_more", "gsx_debug_set_radix_rank_mode",
    "gsx_viewer_set_depth_test", "gsx_viewer_set_depth_buffer_device", "gsx_viewer_upload_depth_buffer",
    "gsx_viewer_set_overlay_lines", "gsx_viewer_set_mask_gizmos", "gsx_download_overlay", "gsx_overlay_device_ptrs",
    "gsx_shard_frame_begin", "gsx_shard_slot_records", "gsx_shard_pack_slots", "gsx_shard_import_slots", "gsx_shard_verify",
    "gsx_shard_wait_verdict", "gsx_shard_repair_count", "gsx_shard_post_counts", "gsx_shard_frame_end",
    "gsx_shard_next_windows", "gsx_shard_download_limits", "gsx_comm_unique_id", "gsx_viewer_comm_init", "gsx_viewer_comm_destroy",
    "gsx_comm_all_to_all", "gsx_comm_all_gather", "gsx_shard_render_frame", "gsx_shard_render_frame_keys",
    "gsx_comm_group_create", "gsx_comm_group_destroy", "gsx_viewer_comm_init_group", "gsx_viewer_comm_init_custom",
    "gsx_shard_set_limits", "gsx_shard_set_slot_records", "gsx_shard_get_stats", "gsx_shard_set_gather_root",
    "gsx_model_buffer_retain", "gsx_buffer_retain", "gsx_buffer_release", "gsx_buffer_len", "gsx_buffer_download",
    "gsx_gaussian_edit_default", "gsx_update_query", "gsx_update_query_texture", "gsx_update_selection_highlight",
    "gsx_update_selection_edit", "gsx_model_show_unedited", "gsx_postprocess", "gsx_model_upload_selection",
    "gsx_model_download_selection", "gsx_model_download_edits", "gsx_model_upload_edits", "gsx_query_download_hits",
    "gsx_query_hit_pos_by_closest", "gsx_query_hit_pos_by_alpha_range",
    "gsx_toolset_set_use_texture", "gsx_toolset_update_brush_radius", "gsx_toolset_start", "gsx_toolset_update_pos", "gsx_toolset_end",
    "gsx_toolset_query", "gsx_toolset_state", "gsx_toolset_render", "gsx_toolset_set_overlay", "gsx_download_query_texture",
    "gsx_debug_set_launch_graphs", "gsx_debug_launch_count", "gsx_debug_device_bytes", "gsx_debug_download_lane_framebuffer", "gsx_viewer_launch_stats", "gsx_debug_tile_profile",
    "gsx_viewer_comm_init_custom_v", "gsx_shard_set_band_edges", "gsx_shard_get_band_edges", "gsx_shard_set_balance",
    "gsx_viewer_comm_info",
    "gsx_bounds_desc_default", "gsx_model_bounds",
    "gsx_extract_desc_default", "gsx_model_extract", "gsx_model_merge",
    "gsx_export_desc_default", "gsx_model_export", "gsx_model_export_ply",
    "gsx_import_desc_default", "gsx_model_upload_ply_rows", "gsx_model_import_ply",
    "gsx_model_pod_kind", "gsx_convert_desc_default", "gsx_model_convert", "gsx_model_set_pod_kind",
    "gsx_model_property_values", "gsx_model_histogram", "gsx_model_select_range",
    "gsx_neighbor_desc_default", "gsx_model_neighbors", "gsx_model_select_neighbors",
    "gsx_cluster_desc_default", "gsx_model_clusters", "gsx_model_select_clusters",
    "gsx_knn_desc_default", "gsx_model_knn", "gsx_model_select_knn",
    "gsx_nearest_desc_default", "gsx_model_nearest", "gsx_model_select_nearest", "gsx_model_align_step",
    "gsx_transform_desc_default", "gsx_model_apply_transform",
    "gsx_decimate_desc_default", "gsx_model_decimate", "gsx_model_decimate_edge",
    "gsx_visibility_desc_default", "gsx_visibility_select_desc_default", "gsx_model_visibility", "gsx_model_select_visibility",
    "gsx_model_visibility_reset",
    "gsx_depth_map_desc_default", "gsx_render_depth_map", "gsx_depth_map_device_ptrs", "gsx_depth_map_unproject",
    "gsx_normals_desc_default", "gsx_model_normals", "gsx_model_select_normals",
    "gsx_model_normals_keep", "gsx_model_normals_kept", "gsx_model_normals_reset", "gsx_model_align_plane_step",
    "gsx_plane_fit_desc_default", "gsx_plane_select_desc_default", "gsx_model_fit_plane", "gsx_model_select_plane", "gsx_plane_level",
)


GSX_OVERLAY_MAX_LINES = 4096


class OverlayLine(C.Structure):
    """``gsx_overlay_line`` = the reference's measurement ``HitPair`` (32 bytes)."""
    _fields_ = [("p0", C.c_float * 3), ("color", C.c_uint8 * 4), ("p1", C.c_float * 3), ("line_width", C.c_float)]


GSX_GIZMO_MAX_SHAPES = 256
GSX_GIZMO_CIRCLE_SEGMENTS = 64


class MaskGizmo(C.Structure):
    """``gsx_mask_gizmo``: a world-space mask shape, its straight RGBA colour and a line width (64 bytes)."""
    _fields_ = [("kind", C.c_uint32), ("pos", C.c_float * 3), ("quat_xyzw", C.c_float * 4), ("scale", C.c_float * 3),
                ("color", C.c_float * 4), ("line_width", C.c_float)]


#: gsx_bounds_desc.filter
GSX_BOUNDS_MASKED, GSX_BOUNDS_SKIP_HIDDEN, GSX_BOUNDS_SELECTED = 1, 2, 4


class BoundsDesc(C.Structure):
    """``gsx_bounds_desc`` (8 bytes): which Gaussians count, and how much of them the trimmed box may leave outside."""
    _fields_ = [("filter", C.c_uint32), ("trim_permille", C.c_uint32)]


class ModelBounds(C.Structure):
    """``gsx_model_bounds_t`` (88 bytes)."""
    _fields_ = [("count", C.c_uint64), ("n_nonfinite", C.c_uint64), ("min", C.c_float * 3), ("max", C.c_float * 3),
                ("center", C.c_float * 3), ("mean", C.c_float * 3), ("trim_min", C.c_float * 3), ("trim_max", C.c_float * 3)]


#: gsx_extract_desc.flags (its filter takes the GSX_BOUNDS_* bits)
GSX_EXTRACT_INVERT, GSX_EXTRACT_DROP_EDITS = 1, 2
#: most sources one gsx_model_merge call takes
GSX_MERGE_MAX_SOURCES = 64


#: gsx_export_desc.format, and the flag that gsx_model_export takes beside GSX_EXTRACT_INVERT
GSX_EXPORT_GAUSSIANS, GSX_EXPORT_PLY_VERTICES = 0, 1
GSX_EXPORT_BAKE_EDITS = 4


class ExportDesc(C.Structure):
    """``gsx_export_desc`` (24 bytes): which Gaussians are exported (``GSX_BOUNDS_*``), ``GSX_EXTRACT_INVERT | GSX_EXPORT_BAKE_EDITS``,
    the row format (``GSX_EXPORT_*``) and the size of one device staging buffer (0: the library's default)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("format", C.c_uint32), ("reserved", C.c_uint32), ("staging_bytes", C.c_uint64)]


class ImportDesc(C.Structure):
    """``gsx_import_desc`` (16 bytes): flags (none are defined), and the size of one device staging buffer (0: the library's default)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("staging_bytes", C.c_uint64)]


class ConvertDesc(C.Structure):
    """``gsx_convert_desc`` (16 bytes): ``ExtractDesc``'s filter and flags, and the pod kind of the new model (``gsx_sh_kind``,
    ``gsx_cov3d_kind``)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("sh", C.c_uint32), ("cov3d", C.c_uint32)]


#: gsx_property: one float32 per Gaussian (spec section 17)
(GSX_PROP_POS_X, GSX_PROP_POS_Y, GSX_PROP_POS_Z, GSX_PROP_RED, GSX_PROP_GREEN, GSX_PROP_BLUE, GSX_PROP_OPACITY, GSX_PROP_HUE,
 GSX_PROP_SATURATION, GSX_PROP_VALUE, GSX_PROP_SCALE_MAX, GSX_PROP_SCALE_MID, GSX_PROP_SCALE_MIN, GSX_PROP_COUNT) = range(14)
#: flags of the property calls: positions in world space; gsx_model_histogram takes [min, max] as its range
GSX_PROP_WORLD, GSX_HIST_AUTO_RANGE = 1, 4
GSX_HIST_MAX_BINS = 4096
#: gsx_selection_op
GSX_SELECTION_SET, GSX_SELECTION_ADD, GSX_SELECTION_REMOVE = 0, 1, 2


class HistogramDesc(C.Structure):
    """``gsx_histogram_desc`` (24 bytes): the property, ``GSX_PROP_WORLD | GSX_HIST_AUTO_RANGE``, the ``GSX_BOUNDS_*`` filter, 1..4096
    bins over ``[lo, hi]``."""
    _fields_ = [("property", C.c_uint32), ("flags", C.c_uint32), ("filter", C.c_uint32), ("bins", C.c_uint32), ("lo", C.c_float), ("hi", C.c_float)]


class Histogram(C.Structure):
    """``gsx_histogram_t`` (48 bytes)."""
    _fields_ = [("count", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("lo", C.c_float), ("hi", C.c_float), ("min", C.c_float), ("max", C.c_float)]


class SelectDesc(C.Structure):
    """``gsx_select_desc`` (40 bytes): the property, ``GSX_PROP_WORLD``, the filter, the ``gsx_selection_op``, the range, and
    (``bins`` > 0) the bins ``[bin_lo, bin_hi]`` of the histogram over that range."""
    _fields_ = [("property", C.c_uint32), ("flags", C.c_uint32), ("filter", C.c_uint32), ("selection_op", C.c_uint32), ("lo", C.c_float),
                ("hi", C.c_float), ("bins", C.c_uint32), ("bin_lo", C.c_uint32), ("bin_hi", C.c_uint32), ("reserved", C.c_uint32)]


#: the most a neighbour count saturates at
GSX_NEIGHBOR_MAX_COUNT = 4095


class NeighborDesc(C.Structure):
    """``gsx_neighbor_desc`` (24 bytes): the ``GSX_BOUNDS_*`` filter, flags (0), the radius in model space, the cap 1..4095 a count
    saturates at, ``grid_bits`` (0: the library's hash table; 1..24 forces ``2**grid_bits`` buckets and changes no result)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_float), ("max_count", C.c_uint32), ("grid_bits", C.c_uint32),
                ("reserved", C.c_uint32)]


class NeighborStats(C.Structure):
    """``gsx_neighbor_stats_t`` (24 bytes)."""
    _fields_ = [("count", C.c_uint64), ("n_nonfinite", C.c_uint64), ("grid_bits", C.c_uint32), ("reserved", C.c_uint32)]


class NeighborSelectDesc(C.Structure):
    """``gsx_neighbor_select_desc`` (40 bytes): the filter, flags (0), the ``gsx_selection_op``, the cap, the radius, the counts
    ``[count_lo, count_hi]`` that are hit, ``grid_bits``."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("selection_op", C.c_uint32), ("max_count", C.c_uint32), ("radius", C.c_float),
                ("count_lo", C.c_uint32), ("count_hi", C.c_uint32), ("grid_bits", C.c_uint32), ("reserved", C.c_uint32 * 2)]


#: the label of a Gaussian that does not participate
GSX_CLUSTER_NONE = 0xFFFFFFFF
#: ``gsx_cluster_select_desc.mode``
GSX_CLUSTER_BY_SIZE, GSX_CLUSTER_LARGEST, GSX_CLUSTER_SEEDED = 0, 1, 2


class ClusterDesc(C.Structure):
    """``gsx_cluster_desc`` (24 bytes): the ``GSX_BOUNDS_*`` filter, flags (0), the radius in model space, ``grid_bits`` (0: the
    library's hash table; 1..24 forces ``2**grid_bits`` buckets and changes no result)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_float), ("grid_bits", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ClusterStats(C.Structure):
    """``gsx_cluster_stats_t`` (40 bytes)."""
    _fields_ = [("count", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_clusters", C.c_uint64), ("largest_size", C.c_uint64),
                ("largest_label", C.c_uint32), ("grid_bits", C.c_uint32)]


class ClusterSelectDesc(C.Structure):
    """``gsx_cluster_select_desc`` (40 bytes): the filter, flags (0), the ``gsx_selection_op``, the ``GSX_CLUSTER_*`` mode, the radius,
    the cluster sizes ``[size_lo, size_hi]`` that are hit (mode BY_SIZE; 0, 0 otherwise), ``grid_bits``."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("selection_op", C.c_uint32), ("mode", C.c_uint32), ("radius", C.c_float),
                ("size_lo", C.c_uint32), ("size_hi", C.c_uint32), ("grid_bits", C.c_uint32), ("reserved", C.c_uint32 * 2)]


#: the largest ``k`` of ``gsx_model_knn``
GSX_KNN_MAX_K = 16
#: ``gsx_knn_desc.score``: the distance to the k-th nearest, or the mean distance to the k nearest
GSX_KNN_SCORE_KTH, GSX_KNN_SCORE_MEAN = 0, 1
#: ``gsx_knn_select_desc.mode``
GSX_KNN_SELECT_RANGE, GSX_KNN_SELECT_OUTLIERS = 0, 1


class KnnDesc(C.Structure):
    """``gsx_knn_desc`` (32 bytes): the ``GSX_BOUNDS_*`` filter, flags (0), ``k`` (1..16), the ``GSX_KNN_SCORE_*`` score, and three
    knobs that change no result: ``radius_hint`` (0: the library's first search radius), ``grid_bits`` (0: the library's hash
    table), ``max_rounds`` (0: the library's rule; 1..64 grid rounds before the exact fallback)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("k", C.c_uint32), ("score", C.c_uint32), ("radius_hint", C.c_float),
                ("grid_bits", C.c_uint32), ("max_rounds", C.c_uint32), ("reserved", C.c_uint32)]


class KnnStats(C.Structure):
    """``gsx_knn_stats_t`` (72 bytes): the participants, the non-finite, the finite scores' number, minimum, maximum, double mean and
    sample deviation, the outlier threshold (select, mode OUTLIERS), and what ran: the first radius, the grid rounds, the Gaussians the
    exact fallback answered, the table."""
    _fields_ = [("count", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_scored", C.c_uint64), ("n_brute", C.c_uint64), ("mean", C.c_double),
                ("std", C.c_double), ("score_min", C.c_float), ("score_max", C.c_float), ("first_radius", C.c_float), ("threshold", C.c_float),
                ("rounds", C.c_uint32), ("grid_bits", C.c_uint32)]


class KnnSelectDesc(C.Structure):
    """``gsx_knn_select_desc`` (48 bytes): the filter, flags (0), the ``gsx_selection_op``, the ``GSX_KNN_SELECT_*`` mode, ``k``, the
    score, the three knobs, the score range ``[lo, hi]`` (mode RANGE) and ``std_ratio`` (mode OUTLIERS: hit above mean + std_ratio *
    std)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("selection_op", C.c_uint32), ("mode", C.c_uint32), ("k", C.c_uint32),
                ("score", C.c_uint32), ("radius_hint", C.c_float), ("grid_bits", C.c_uint32), ("max_rounds", C.c_uint32), ("lo", C.c_float),
                ("hi", C.c_float), ("std_ratio", C.c_float)]


#: the smallest and the largest ``k`` of ``gsx_model_normals``
GSX_NORMALS_MIN_K, GSX_NORMALS_MAX_K = 3, 16
#: ``gsx_normals_desc.orient``: the first non-zero component positive, or looking at ``toward``
GSX_NORMALS_ORIENT_CANONICAL, GSX_NORMALS_ORIENT_TOWARD = 0, 1
#: ``gsx_normals_select_desc.mode``
GSX_NORMALS_SELECT_VARIATION, GSX_NORMALS_SELECT_FACING = 0, 1
#: ``gsx_normals_select_desc.flags``: mode FACING tests the absolute cosine
GSX_NORMALS_ABS = 1
#: ``gsx_model_normals``: the index of a neighbour that does not exist
GSX_NORMALS_NONE = 0xFFFFFFFF


class NormalsDesc(C.Structure):
    """``gsx_normals_desc`` (48 bytes): the ``GSX_BOUNDS_*`` filter, flags (0), ``k`` (3..16), the ``GSX_NORMALS_ORIENT_*`` rule and its
    model-space point ``toward``, and ``gsx_knn_desc``'s three knobs that change no result."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("k", C.c_uint32), ("orient", C.c_uint32), ("radius_hint", C.c_float),
                ("grid_bits", C.c_uint32), ("max_rounds", C.c_uint32), ("reserved", C.c_uint32), ("toward", C.c_float * 3),
                ("reserved2", C.c_uint32)]


class NormalsStats(C.Structure):
    """``gsx_normals_stats_t`` (64 bytes): the participants, the non-finite, the fitted Gaussians' number and their variations' double
    mean, minimum and maximum, and what ran: the first radius, the grid rounds, the Gaussians the exact fallback answered, the table."""
    _fields_ = [("count", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_fitted", C.c_uint64), ("n_brute", C.c_uint64), ("mean", C.c_double),
                ("variation_min", C.c_float), ("variation_max", C.c_float), ("first_radius", C.c_float), ("rounds", C.c_uint32),
                ("grid_bits", C.c_uint32), ("reserved", C.c_uint32)]


class NormalsSelectDesc(C.Structure):
    """``gsx_normals_select_desc`` (80 bytes): the filter, flags (``GSX_NORMALS_ABS``), the ``gsx_selection_op``, the
    ``GSX_NORMALS_SELECT_*`` mode, ``k``, the orient rule, the three knobs, the range ``[lo, hi]`` of the variation or of the cosine
    between the normal and ``dir``, and ``toward``."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("selection_op", C.c_uint32), ("mode", C.c_uint32), ("k", C.c_uint32),
                ("orient", C.c_uint32), ("radius_hint", C.c_float), ("grid_bits", C.c_uint32), ("max_rounds", C.c_uint32), ("lo", C.c_float),
                ("hi", C.c_float), ("reserved", C.c_uint32), ("dir", C.c_float * 3), ("toward", C.c_float * 3), ("reserved2", C.c_uint32 * 2)]


#: ``gsx_model_nearest``: the index of a query without a target in reach
GSX_NEAREST_NONE = 0xFFFFFFFF
#: ``gsx_nearest_desc.flags``: the matrix is inv(M_dst) * M_src of the two models' transforms, not ``xform``
GSX_NEAREST_MODEL_TRANSFORMS = 1
#: ``gsx_nearest_select_desc.mode``
GSX_NEAREST_SELECT_RANGE, GSX_NEAREST_SELECT_TRANSFER = 0, 1
#: ``gsx_align_desc.flags``: solve for a uniform scale too
GSX_ALIGN_SCALE = 1


class NearestDesc(C.Structure):
    """``gsx_nearest_desc`` (80 bytes): the ``GSX_BOUNDS_*`` filters of the queries and of the targets, flags
    (``GSX_NEAREST_MODEL_TRANSFORMS``), ``max_distance`` (0: unlimited), the row-major 3x4 ``xform`` from the source's model space
    into the targets', and three knobs that change no result: ``radius_hint``, ``grid_bits``, ``max_rounds`` (``gsx_knn_desc``'s)."""
    _fields_ = [("src_filter", C.c_uint32), ("dst_filter", C.c_uint32), ("flags", C.c_uint32), ("grid_bits", C.c_uint32),
                ("max_distance", C.c_float), ("radius_hint", C.c_float), ("max_rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("xform", C.c_float * 12)]


class NearestStats(C.Structure):
    """``gsx_nearest_stats_t`` (136 bytes): the participating queries and targets and the non-finite of both, the found queries, the
    queries the exact fallback answered, the double mean distance and rms, the least and largest distance, what ran (first radius,
    grid rounds, table) and the matrix used."""
    _fields_ = [("count", C.c_uint64), ("n_nonfinite", C.c_uint64), ("targets", C.c_uint64), ("targets_nonfinite", C.c_uint64),
                ("n_found", C.c_uint64), ("n_brute", C.c_uint64), ("mean", C.c_double), ("rms", C.c_double), ("d_min", C.c_float),
                ("d_max", C.c_float), ("first_radius", C.c_float), ("rounds", C.c_uint32), ("grid_bits", C.c_uint32), ("reserved", C.c_uint32),
                ("xform", C.c_float * 12)]


class NearestSelectDesc(C.Structure):
    """``gsx_nearest_select_desc`` (96 bytes): the search, the ``gsx_selection_op``, the ``GSX_NEAREST_SELECT_*`` mode and the distance
    range ``[lo, hi]`` (mode RANGE)."""
    _fields_ = [("nearest", NearestDesc), ("selection_op", C.c_uint32), ("mode", C.c_uint32), ("lo", C.c_float), ("hi", C.c_float)]


class AlignDesc(C.Structure):
    """``gsx_align_desc`` (88 bytes): the search and flags (``GSX_ALIGN_SCALE``)."""
    _fields_ = [("nearest", NearestDesc), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class AlignStep(C.Structure):
    """``gsx_align_step_t`` (272 bytes): the delta ``t ~ scale * R(quat) q + pos`` (``quat`` x, y, z, w), ``xform_next`` = delta o
    the matrix used, the pairs, the rms distance before the step, whether the step was degenerate, the search's statistics."""
    _fields_ = [("pos", C.c_double * 3), ("quat", C.c_double * 4), ("scale", C.c_double), ("xform_next", C.c_float * 12), ("n_pairs", C.c_uint64),
                ("rms_before", C.c_double), ("degenerate", C.c_uint32), ("reserved", C.c_uint32), ("nearest", NearestStats)]


class NormalsKept(C.Structure):
    """``gsx_normals_kept_t`` (48 bytes): whether a model has kept normals, the ``k``, ``orient``, ``filter`` and ``toward`` they were made
    with, the model's Gaussian count then and how many have a plane."""
    _fields_ = [("present", C.c_uint32), ("k", C.c_uint32), ("orient", C.c_uint32), ("filter", C.c_uint32), ("toward", C.c_float * 3),
                ("reserved", C.c_uint32), ("count", C.c_uint64), ("n_fitted", C.c_uint64)]


class AlignPlaneDesc(C.Structure):
    """``gsx_align_plane_desc`` (96 bytes): the search, flags (0) and ``max_variation`` (0: no limit)."""
    _fields_ = [("nearest", NearestDesc), ("flags", C.c_uint32), ("max_variation", C.c_float), ("reserved", C.c_uint32 * 2)]


class AlignPlaneStep(C.Structure):
    """``gsx_align_plane_step_t`` (568 bytes): the delta ``t ~ R(quat) q + pos``, the upper triangle of the 6x6 normal matrix, its
    right-hand side, its eigenvalues (descending), the centre, the two rms residuals before the step, the pairs used and left out,
    ``xform_next``, the rank, whether the step was degenerate, the search's statistics."""
    _fields_ = [("pos", C.c_double * 3), ("quat", C.c_double * 4), ("normal_matrix", C.c_double * 21), ("rhs", C.c_double * 6),
                ("eigenvalues", C.c_double * 6), ("centre", C.c_double * 3), ("rms_before", C.c_double), ("rms_plane_before", C.c_double),
                ("n_pairs", C.c_uint64), ("n_unfitted", C.c_uint64), ("xform_next", C.c_float * 12), ("rank", C.c_uint32),
                ("degenerate", C.c_uint32), ("nearest", NearestStats)]


#: ``gsx_plane_fit_desc.sample``; the most candidates and refine rounds; "no winner"
GSX_PLANE_SAMPLE_TRIPLES, GSX_PLANE_SAMPLE_NORMALS, GSX_PLANE_SAMPLE_CALLER = 0, 1, 2
GSX_PLANE_MAX_CANDIDATES, GSX_PLANE_MAX_REFINE, GSX_PLANE_NONE = 1024, 8, 0xFFFFFFFF


class Plane(C.Structure):
    """``gsx_plane_t`` (16 bytes): the points ``p`` with ``normal . p = offset``."""
    _fields_ = [("normal", C.c_float * 3), ("offset", C.c_float)]


class PlaneFitDesc(C.Structure):
    """``gsx_plane_fit_desc`` (64 bytes): filter (``GSX_BOUNDS_*``), flags (``GSX_EXTRACT_INVERT``), sample (``GSX_PLANE_SAMPLE_*``),
    n_candidates (1 .. 1024), seed, tolerance, min_cos (0: off), refine_iters (0 .. 8), orient and toward (the normals' rule), reserved."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("sample", C.c_uint32), ("n_candidates", C.c_uint32), ("seed", C.c_uint64),
                ("tolerance", C.c_float), ("min_cos", C.c_float), ("refine_iters", C.c_uint32), ("orient", C.c_uint32), ("toward", C.c_float * 3),
                ("reserved", C.c_uint32 * 3)]


class PlaneFit(C.Structure):
    """``gsx_plane_fit_t`` (208 bytes): the plane, the winning candidate and its index, the valid candidates, the participants, the
    filtered Gaussians without a finite position, the candidate's and the plane's inliers, and of the last accepted fit the centroid,
    the eigenvalues (descending), the rms residual and the sums; the refine rounds accepted; degenerate."""
    _fields_ = [("plane", Plane), ("candidate", Plane), ("winner", C.c_uint32), ("n_valid", C.c_uint32), ("count", C.c_uint64),
                ("n_nonfinite", C.c_uint64), ("candidate_inliers", C.c_uint64), ("n_inliers", C.c_uint64), ("centroid", C.c_float * 3),
                ("refine_done", C.c_uint32), ("eigenvalues", C.c_double * 3), ("rms", C.c_double), ("sums", C.c_double * 10),
                ("degenerate", C.c_uint32), ("reserved", C.c_uint32)]


class PlaneSelectDesc(C.Structure):
    """``gsx_plane_select_desc`` (48 bytes): the plane, the signed residual's range ``[lo, hi]`` (a bound may be infinite), min_cos,
    filter, selection_op, reserved."""
    _fields_ = [("plane", Plane), ("lo", C.c_float), ("hi", C.c_float), ("min_cos", C.c_float), ("filter", C.c_uint32),
                ("selection_op", C.c_uint32), ("reserved", C.c_uint32 * 3)]


#: ``gsx_visibility_desc.flags``: fold this view into the model's resident planes instead of replacing them
GSX_VIS_ACCUMULATE = 1
#: ``gsx_visibility_select_desc.measure``
GSX_VIS_PEAK, GSX_VIS_WEIGHT, GSX_VIS_PIXELS = 0, 1, 2


class VisibilityDesc(C.Structure):
    """``gsx_visibility_desc`` (16 bytes): flags (``GSX_VIS_ACCUMULATE``), reserved (0)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class VisibilitySelectDesc(C.Structure):
    """``gsx_visibility_select_desc`` (32 bytes): the ``GSX_VIS_*`` measure, the ``GSX_BOUNDS_*`` filter, the ``gsx_selection_op``,
    reserved (0) and the inclusive range ``[lo, hi]`` of the resident measure (``hi`` may be ``inf``)."""
    _fields_ = [("measure", C.c_uint32), ("filter", C.c_uint32), ("selection_op", C.c_uint32), ("reserved", C.c_uint32),
                ("lo", C.c_double), ("hi", C.c_double)]


class VisibilityStats(C.Structure):
    """``gsx_visibility_stats_t`` (40 bytes): Gaussians after cull in this view, Gaussians with a resident peak > 0, the (pixel,
    Gaussian) pairs blended in this view and the sum of their 2^-24 fixed-point weights, the largest resident peak, the views folded."""
    _fields_ = [("n_visible", C.c_uint64), ("n_seen", C.c_uint64), ("n_pairs", C.c_uint64), ("weight_fixed", C.c_uint64),
                ("peak_max", C.c_float), ("views", C.c_uint32)]


#: ``gsx_depth_map_desc.flags``: also write the ndc plane (what ``gsx_viewer_set_depth_buffer_device`` takes)
GSX_DEPTH_MAP_NDC = 1
#: index and layer of a pixel without a crossing (its surface is ``inf``)
GSX_DEPTH_MAP_NONE = 0xFFFFFFFF


class DepthMapDesc(C.Structure):
    """``gsx_depth_map_desc`` (16 bytes): flags (``GSX_DEPTH_MAP_NDC``), the transmittance threshold of the surface (0.5: the median
    depth; 1.0: the first record that lowers T at all), reserved (0)."""
    _fields_ = [("flags", C.c_uint32), ("threshold", C.c_float), ("reserved", C.c_uint32 * 2)]


class DepthMapStats(C.Structure):
    """``gsx_depth_map_stats_t`` (32 bytes): pixels with ``A > 0``, pixels with a crossing, the smallest and largest surface over the
    crossings (``inf`` and 0 without one), the number of models, reserved."""
    _fields_ = [("n_covered", C.c_uint64), ("n_crossed", C.c_uint64), ("surface_min", C.c_float), ("surface_max", C.c_float),
                ("models", C.c_uint32), ("reserved", C.c_uint32)]


class TransformDesc(C.Structure):
    """``gsx_transform_desc`` (64 bytes): the ``GSX_BOUNDS_*`` filter, flags (``GSX_EXTRACT_INVERT``), the transform as
    ``gsx_update_model_transform`` takes it (``quat`` x, y, z, w), the pivot it rotates and scales about, reserved (0)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("pos", C.c_float * 3), ("quat", C.c_float * 4), ("scale", C.c_float * 3),
                ("pivot", C.c_float * 3), ("reserved", C.c_uint32)]


#: ``out_map`` of a Gaussian that does not participate in a decimate
GSX_DECIMATE_NO_CELL = 0xFFFFFFFF


class DecimateDesc(C.Structure):
    """``gsx_decimate_desc`` (24 bytes): the ``GSX_BOUNDS_*`` filter, flags (``GSX_EXTRACT_INVERT``), the cell edge in model space
    (must be set), ``grid_bits`` (0: the library's hash table; 1..24 forces ``2**grid_bits`` buckets and changes no result)."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32), ("cell", C.c_float), ("grid_bits", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class DecimateStats(C.Structure):
    """``gsx_decimate_stats_t`` (40 bytes)."""
    _fields_ = [("count", C.c_uint64), ("n_nonfinite", C.c_uint64), ("cells", C.c_uint64), ("singletons", C.c_uint64),
                ("largest_cell", C.c_uint32), ("grid_bits", C.c_uint32)]


class ExtractDesc(C.Structure):
    """``gsx_extract_desc`` (8 bytes): which Gaussians the new model keeps (``GSX_BOUNDS_*``), and ``GSX_EXTRACT_*`` flags."""
    _fields_ = [("filter", C.c_uint32), ("flags", C.c_uint32)]


class GaussianEdit(C.Structure):
    """``gsx_gaussian_edit`` = gs::GaussianEditPod (32 bytes)."""
    _fields_ = [("flag", C.c_uint32), ("color", C.c_float * 3), ("contrast", C.c_float), ("exposure", C.c_float),
                ("gamma", C.c_float), ("alpha", C.c_float)]


class Query(C.Structure):
    """``gsx_query``."""
    _fields_ = [("kind", C.c_uint32), ("selection_op", C.c_uint32), ("p0", C.c_float * 2), ("p1", C.c_float * 2),
                ("radius", C.c_float), ("reserved", C.c_uint32)]


class LaunchStats(C.Structure):
    """``gsx_launch_stats``."""
    _fields_ = [(n, C.c_uint64) for n in ("graph_launches", "graph_nodes", "nodes_patched", "direct_launches", "graphs_built", "broken", "idle_direct_scopes")]


class SpecParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("max_std_dev", "cull_margin", "jacobian_clamp", "low_pass", "alpha_max",
                                        "alpha_min", "t_epsilon", "point_radius")]


class RenderOptions(C.Structure):
    _fields_ = [("progressive", C.c_uint32), ("first_slab_divisor", C.c_uint32), ("min_slab", C.c_uint32), ("growth", C.c_uint32),
                ("speculative", C.c_uint32), ("spec_margin", C.c_float), ("spec_radius", C.c_uint32), ("host_verify", C.c_uint32),
                ("frames_in_flight", C.c_uint32), ("slab_shading", C.c_uint32)]


class PlyHeader(C.Structure):
    _fields_ = [("count", C.c_uint64), ("header_bytes", C.c_uint64), ("vertex_bytes", C.c_uint32), ("is_ascii", C.c_uint32),
                ("offsets", C.c_int32 * 62)]


class ShardLayout(C.Structure):
    _fields_ = [("rows_per_rank", C.c_uint32), ("row_lo", C.c_uint32), ("row_hi", C.c_uint32), ("band_bytes", C.c_uint64),
                ("band_offset_bytes", C.c_uint64), ("padded_framebuffer_bytes", C.c_uint64)]


class ViewerDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("stream", C.c_void_p), ("width", C.c_uint32),
                ("height", C.c_uint32)]


class FrameStats(C.Structure):
    _fields_ = [("n_gaussians", C.c_uint64), ("n_visible", C.c_uint64), ("n_tile_entries", C.c_uint64), ("n_sorted", C.c_uint64),
                ("n_repair_tiles", C.c_uint64), ("n_repair_sorted", C.c_uint64), ("speculated", C.c_uint32), ("overflow_slabs", C.c_uint32)]


class ShardVerdict(C.Structure):
    """``gsx_shard_verdict``."""
    _fields_ = [("need_tiles", C.c_uint32), ("overflow", C.c_uint32), ("max_records", C.c_uint32), ("reserved", C.c_uint32)]


class ShardStats(C.Structure):
    """``gsx_shard_stats``."""
    _fields_ = [("frames", C.c_uint64), ("redo_frames", C.c_uint64), ("repair_frames", C.c_uint64), ("exchange_rounds", C.c_uint64),
                ("wire_bytes", C.c_uint64), ("verdict_wait_ns", C.c_uint64), ("last_slot_records", C.c_uint32),
                ("last_repair_slot_records", C.c_uint32), ("last_entries_sum", C.c_uint32), ("last_entries_max", C.c_uint32),
                ("last_work_permille", C.c_uint32), ("redo_fallbacks", C.c_uint32),
                ("last_repair_records", C.c_uint32), ("reserved0", C.c_uint32)]


class CommInfo(C.Structure):
    """``gsx_comm_info``."""
    _fields_ = [("transport", C.c_uint32), ("nranks", C.c_uint32), ("rank", C.c_uint32), ("lane_comms", C.c_uint32),
                ("device", C.c_int32), ("version", C.c_int32)]


#: gsx_comm_all_to_all_fn / gsx_comm_all_gather_fn: (ctx, d_send, d_recv, bytes, hip_stream) -> gsx_status
COMM_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
#: gsx_comm_all_to_all_v_fn(ctx, d_send, send_offsets, send_bytes, d_recv, recv_offsets, recv_bytes, hip_stream)
COMM_A2A_V_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64),
                            C.POINTER(C.c_uint64), C.c_void_p)
#: gsx_comm_gather_v_fn(ctx, d_send, send_bytes, d_recv, recv_offsets, recv_bytes, root, hip_stream)
COMM_GATHER_V_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int32, C.c_void_p)


class GsxError(RuntimeError):
    """``gs::Error``: raised for every non-zero ``gsx_status``; ``status`` holds the code."""

    def __init__(self, status: int, message: str):
        super().__init__(f"gsx status {status}: {message}")
        self.status = status


_lib = None
#: names load() lets a library lack.  Empty: a library exports every declared name.  tools/bench_drag.py names the toolset's calls here,
#: before the first load(), when it runs its host rows on a build from before the toolset (GSX_LIB), and tools/bench_depth.py names
#: gsx_viewer_set_mask_gizmos for its rows on a build from before the gizmos; nothing else may.
MAY_LACK: frozenset = frozenset()


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("GSX_LIB", LIB_PATH)  # development: A/B a differently built library on the same box
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback for the render path.")
    L = C.CDLL(path)
    vp, u32, u64, f32p, u32p, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_char_p
    sig = {
        "gsx_last_error_string": ([], C.c_char_p),
        "gsx_abi_version": ([], u32),
        "gsx_spec_params_default": ([C.POINTER(SpecParams)], None),
        "gsx_viewer_create": ([C.POINTER(ViewerDesc), C.POINTER(vp)], C.c_int32),
        "gsx_viewer_destroy": ([vp], None),
        "gsx_viewer_set_spec_params": ([vp, C.POINTER(SpecParams)], C.c_int32),
        "gsx_model_create": ([vp, cp, u64, C.c_int, C.c_int], C.c_int32),
        "gsx_model_remove": ([vp, cp], C.c_int32),
        "gsx_model_len": ([vp, cp, C.POINTER(u64)], C.c_int32),
        "gsx_model_upload_range": ([vp, cp, u64, vp, u64], C.c_int32),
        "gsx_model_upload_pod_device": ([vp, cp, u64, u64, vp, vp, vp, vp], C.c_int32),
        "gsx_update_camera": ([vp, f32p, f32p, u32, u32], C.c_int32),
        "gsx_update_model_transform": ([vp, cp, f32p, f32p, f32p], C.c_int32),
        "gsx_update_gaussian_transform": ([vp, C.c_float, C.c_int, u32, u32], C.c_int32),
        "gsx_model_upload_mask": ([vp, cp, u32p, u64], C.c_int32),
        "gsx_model_download_mask": ([vp, cp, u32p, u64], C.c_int32),
        "gsx_mask_evaluate": ([vp, cp, vp, u32, vp, u32], C.c_int32),
        "gsx_ply_read_header": ([vp, u64, C.POINTER(PlyHeader)], C.c_int32),
        "gsx_ply_read_gaussians": ([vp, u64, C.POINTER(PlyHeader), u64, u64, vp], C.c_int32),
        "gsx_ply_write": ([vp, u64, u32p, vp, vp, u64, C.POINTER(u64)], C.c_int32),
        "gsx_gaussian_edit_default": ([vp], None),
        "gsx_update_query": ([vp, vp], C.c_int32),
        "gsx_update_query_texture": ([vp, vp, u32, u32], C.c_int32),
        "gsx_update_selection_highlight": ([vp, f32p], C.c_int32),
        "gsx_update_selection_edit": ([vp, vp], C.c_int32),
        "gsx_model_show_unedited": ([vp, cp, u32], C.c_int32),
        "gsx_postprocess": ([vp, cp], C.c_int32),
        "gsx_model_upload_selection": ([vp, cp, u32p, u64], C.c_int32),
        "gsx_model_download_selection": ([vp, cp, u32p, u64], C.c_int32),
        "gsx_model_download_edits": ([vp, cp, vp, u64], C.c_int32),
        "gsx_model_upload_edits": ([vp, cp, vp, u64], C.c_int32),
        "gsx_query_download_hits": ([vp, cp, vp, u64, C.POINTER(u64)], C.c_int32),
        "gsx_query_hit_pos_by_closest": ([vp, u64, f32p, f32p, u32, u32, f32p, u32p, f32p], C.c_int32),
        "gsx_query_hit_pos_by_alpha_range": ([vp, u64, f32p, f32p, u32, u32, f32p, C.c_float, u32p, f32p, f32p], C.c_int32),
        "gsx_toolset_set_use_texture": ([vp, u32], C.c_int32),
        "gsx_toolset_update_brush_radius": ([vp, C.c_float], C.c_int32),
        "gsx_toolset_start": ([vp, u32, u32, f32p], C.c_int32),
        "gsx_toolset_update_pos": ([vp, f32p], C.c_int32),
        "gsx_toolset_end": ([vp], C.c_int32),
        "gsx_toolset_query": ([vp, C.POINTER(Query)], C.c_int32),
        "gsx_toolset_state": ([vp, u32p, u32p, u32p, f32p, f32p], C.c_int32),
        "gsx_toolset_render": ([vp], C.c_int32),
        "gsx_toolset_set_overlay": ([vp, f32p, f32p, C.c_float], C.c_int32),
        "gsx_download_query_texture": ([vp, vp, u32, u32], C.c_int32),
        "gsx_preprocess": ([vp, cp], C.c_int32),
        "gsx_sort": ([vp, cp], C.c_int32),
        "gsx_sync": ([vp], C.c_int32),
        "gsx_render": ([vp, C.POINTER(cp), u32], C.c_int32),
        "gsx_render_frame": ([vp, C.POINTER(cp), u32], C.c_int32),
        "gsx_download_framebuffer": ([vp, f32p, u64], C.c_int32),
        "gsx_download_rgba8": ([vp, f32p, C.POINTER(C.c_uint8), u64], C.c_int32),
        "gsx_resolve_rgba8_device": ([vp, f32p, u32, u32, vp], C.c_int32),
        "gsx_framebuffer_device_ptr": ([vp, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)], C.c_int32),
        "gsx_model_frame_stats": ([vp, cp, C.POINTER(FrameStats)], C.c_int32),
        "gsx_model_download_projection": ([vp, cp, u32p, u32p, f32p, f32p, f32p], C.c_int32),
        "gsx_model_download_sorted": ([vp, cp, u32p, u64, C.POINTER(u64)], C.c_int32),
        "gsx_model_download_tile_lists": ([vp, cp, u32p, u64, u32p, u64], C.c_int32),
        "gsx_model_download_pod": ([vp, cp, f32p, u32p, f32p, f32p], C.c_int32),
        "gsx_render_options_default": ([C.POINTER(RenderOptions)], None),
        "gsx_viewer_set_render_options": ([vp, C.POINTER(RenderOptions)], C.c_int32),
        "gsx_shard_layout": ([vp, u32, u32, C.POINTER(ShardLayout)], C.c_int32),
        "gsx_viewer_set_external_framebuffer": ([vp, vp, u64], C.c_int32),
        "gsx_viewer_set_depth_test": ([vp, C.c_int], C.c_int32),
        "gsx_viewer_set_depth_buffer_device": ([vp, vp, u32, u32, u64], C.c_int32),
        "gsx_viewer_upload_depth_buffer": ([vp, f32p, u32, u32], C.c_int32),
        "gsx_viewer_set_overlay_lines": ([vp, vp, u32], C.c_int32),
        "gsx_viewer_set_mask_gizmos": ([vp, vp, u32], C.c_int32),
        "gsx_download_overlay": ([vp, f32p, f32p], C.c_int32),
        "gsx_overlay_device_ptrs": ([vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)], C.c_int32),
        "gsx_shard_pack": ([vp, cp, u32, vp, vp, u64, C.POINTER(u64)], C.c_int32),
        "gsx_shard_import": ([vp, cp, vp, u64, u32, u32, vp], C.c_int32),
        "gsx_shard_set_windows": ([vp, cp, vp], C.c_int32),
        "gsx_viewer_set_band": ([vp, u32, u32], C.c_int32),
        "gsx_shard_feedback_words": ([vp, u32, C.POINTER(u32)], C.c_int32),
        "gsx_shard_feedback": ([vp, cp, u32, u32, vp], C.c_int32),
        "gsx_render_more": ([vp, C.POINTER(cp), u32], C.c_int32),
        "gsx_debug_set_radix_rank_mode": ([C.c_int32], None),
        "gsx_shard_frame_begin": ([vp, cp, u32, u32, u32, vp], C.c_int32),
        "gsx_shard_slot_records": ([vp, cp, u32, u32, C.POINTER(u32)], C.c_int32),
        "gsx_shard_wait_verdict": ([vp, cp, u32, C.POINTER(ShardVerdict)], C.c_int32),
        "gsx_shard_repair_count": ([vp, cp, u32, vp], C.c_int32),
        "gsx_shard_post_counts": ([vp, u32, vp, C.POINTER(u32)], C.c_int32),
        "gsx_shard_frame_end": ([vp, cp], C.c_int32),
        "gsx_shard_pack_slots": ([vp, cp, u32, u32, vp, u32], C.c_int32),
        "gsx_shard_import_slots": ([vp, cp, vp, u32, u32, u32, u32], C.c_int32),
        "gsx_shard_verify": ([vp, cp, u32, vp, C.POINTER(u32)], C.c_int32),
        "gsx_shard_next_windows": ([vp, cp, u32, vp, C.c_float, u32], C.c_int32),
        "gsx_shard_download_limits": ([vp, cp, u32p, u64], C.c_int32),
        "gsx_comm_unique_id": ([vp], C.c_int32),
        "gsx_viewer_comm_init": ([vp, u32, u32, vp], C.c_int32),
        "gsx_viewer_comm_destroy": ([vp], C.c_int32),
        "gsx_comm_all_to_all": ([vp, vp, vp, u64], C.c_int32),
        "gsx_comm_all_gather": ([vp, vp, vp, u64], C.c_int32),
        "gsx_shard_render_frame": ([vp, cp, u32, u32, C.c_float, u32], C.c_int32),
        "gsx_shard_render_frame_keys": ([vp, C.POINTER(cp), u32, u32p, u32, C.c_float, u32], C.c_int32),
        "gsx_comm_group_create": ([u32, u32, C.POINTER(vp)], C.c_int32),
        "gsx_comm_group_destroy": ([vp], None),
        "gsx_viewer_comm_init_group": ([vp, vp, u32], C.c_int32),
        "gsx_viewer_comm_init_custom": ([vp, u32, u32, COMM_FN, COMM_FN, vp], C.c_int32),
        "gsx_viewer_comm_init_custom_v": ([vp, u32, u32, COMM_A2A_V_FN, COMM_GATHER_V_FN, vp], C.c_int32),
        "gsx_shard_set_band_edges": ([vp, u32, u32p], C.c_int32),
        "gsx_shard_get_band_edges": ([vp, u32, u32p], C.c_int32),
        "gsx_shard_set_balance": ([vp, u32], C.c_int32),
        "gsx_shard_set_limits": ([vp, cp, vp], C.c_int32),
        "gsx_shard_set_slot_records": ([vp, cp, u32], C.c_int32),
        "gsx_shard_set_gather_root": ([vp, C.c_int32], C.c_int32),
        "gsx_shard_get_stats": ([vp, C.POINTER(ShardStats), u32], C.c_int32),
        "gsx_viewer_comm_info": ([vp, C.POINTER(CommInfo)], C.c_int32),
        "gsx_model_buffer_retain": ([vp, cp, C.c_int, C.POINTER(vp)], C.c_int32),
        "gsx_buffer_retain": ([vp], C.c_int32),
        "gsx_buffer_release": ([vp], None),
        "gsx_buffer_len": ([vp, C.POINTER(u64)], C.c_int32),
        "gsx_buffer_download": ([vp, vp, u64], C.c_int32),
        "gsx_debug_set_launch_graphs": ([C.c_int32], None),
        "gsx_debug_launch_count": ([], C.c_uint64),
        "gsx_debug_device_bytes": ([], C.c_uint64),
        "gsx_debug_tile_profile": ([vp, u32p, u64], C.c_int32),
        "gsx_debug_download_lane_framebuffer": ([vp, C.c_uint32, C.c_void_p, u64], C.c_int32),
        "gsx_viewer_launch_stats": ([vp, C.POINTER(LaunchStats), u32], C.c_int32),
        "gsx_set_pass_timing": ([vp, u32], C.c_int32),
        "gsx_get_pass_timing": ([vp, f32p, u32p], C.c_int32),
        "gsx_bounds_desc_default": ([C.POINTER(BoundsDesc)], None),
        "gsx_model_bounds": ([vp, cp, C.POINTER(BoundsDesc), C.POINTER(ModelBounds)], C.c_int32),
        "gsx_extract_desc_default": ([C.POINTER(ExtractDesc)], None),
        "gsx_model_extract": ([vp, cp, cp, C.POINTER(ExtractDesc), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_export_desc_default": ([C.POINTER(ExportDesc)], None),
        "gsx_model_export": ([vp, cp, C.POINTER(ExportDesc), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_model_export_ply": ([vp, cp, C.POINTER(ExportDesc), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_import_desc_default": ([C.POINTER(ImportDesc)], None),
        "gsx_model_upload_ply_rows": ([vp, cp, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(PlyHeader), C.POINTER(ImportDesc)], C.c_int32),
        "gsx_model_import_ply": ([vp, cp, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(ImportDesc), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_model_pod_kind": ([vp, cp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)], C.c_int32),
        "gsx_convert_desc_default": ([C.POINTER(ConvertDesc)], None),
        "gsx_model_convert": ([vp, cp, cp, C.POINTER(ConvertDesc), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_model_set_pod_kind": ([vp, cp, C.c_int32, C.c_int32], C.c_int32),
        "gsx_model_property_values": ([vp, cp, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64], C.c_int32),
        "gsx_model_histogram": ([vp, cp, C.POINTER(HistogramDesc), C.POINTER(C.c_uint64), C.POINTER(Histogram)], C.c_int32),
        "gsx_model_select_range": ([vp, cp, C.POINTER(SelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_neighbor_desc_default": ([C.POINTER(NeighborDesc)], None),
        "gsx_model_neighbors": ([vp, cp, C.POINTER(NeighborDesc), C.c_void_p, C.c_void_p, C.POINTER(NeighborStats)], C.c_int32),
        "gsx_model_select_neighbors": ([vp, cp, C.POINTER(NeighborSelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_cluster_desc_default": ([C.POINTER(ClusterDesc)], None),
        "gsx_model_clusters": ([vp, cp, C.POINTER(ClusterDesc), C.c_void_p, C.c_void_p, C.POINTER(ClusterStats)], C.c_int32),
        "gsx_model_select_clusters": ([vp, cp, C.POINTER(ClusterSelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_knn_desc_default": ([C.POINTER(KnnDesc)], None),
        "gsx_model_knn": ([vp, cp, C.POINTER(KnnDesc), C.c_void_p, C.c_void_p, C.POINTER(KnnStats)], C.c_int32),
        "gsx_model_select_knn": ([vp, cp, C.POINTER(KnnSelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(KnnStats)], C.c_int32),
        "gsx_normals_desc_default": ([C.POINTER(NormalsDesc)], None),
        "gsx_model_normals": ([vp, cp, C.POINTER(NormalsDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NormalsStats)], C.c_int32),
        "gsx_model_select_normals": ([vp, cp, C.POINTER(NormalsSelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(NormalsStats)],
                                     C.c_int32),
        "gsx_model_normals_keep": ([vp, cp, C.POINTER(NormalsDesc), C.POINTER(NormalsStats)], C.c_int32),
        "gsx_model_normals_kept": ([vp, cp, C.POINTER(NormalsKept), C.c_void_p, C.c_void_p], C.c_int32),
        "gsx_model_normals_reset": ([vp, cp], C.c_int32),
        "gsx_model_align_plane_step": ([vp, cp, cp, C.POINTER(AlignPlaneDesc), C.POINTER(AlignPlaneStep)], C.c_int32),
        "gsx_plane_fit_desc_default": ([C.POINTER(PlaneFitDesc)], None),
        "gsx_plane_select_desc_default": ([C.POINTER(PlaneSelectDesc)], None),
        "gsx_model_fit_plane": ([vp, cp, C.POINTER(PlaneFitDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PlaneFit)], C.c_int32),
        "gsx_model_select_plane": ([vp, cp, C.POINTER(PlaneSelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_plane_level": ([C.POINTER(Plane), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 4), C.POINTER(C.c_float * 3)], C.c_int32),
        "gsx_nearest_desc_default": ([C.POINTER(NearestDesc)], None),
        "gsx_model_nearest": ([vp, cp, cp, C.POINTER(NearestDesc), C.c_void_p, C.c_void_p, C.POINTER(NearestStats)], C.c_int32),
        "gsx_model_select_nearest": ([vp, cp, cp, C.POINTER(NearestSelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(NearestStats)], C.c_int32),
        "gsx_model_align_step": ([vp, cp, cp, C.POINTER(AlignDesc), C.POINTER(AlignStep)], C.c_int32),
        "gsx_transform_desc_default": ([C.POINTER(TransformDesc)], None),
        "gsx_model_apply_transform": ([vp, cp, C.POINTER(TransformDesc), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_visibility_desc_default": ([C.POINTER(VisibilityDesc)], None),
        "gsx_visibility_select_desc_default": ([C.POINTER(VisibilitySelectDesc)], None),
        "gsx_model_visibility": ([vp, cp, C.POINTER(VisibilityDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(VisibilityStats)], C.c_int32),
        "gsx_model_select_visibility": ([vp, cp, C.POINTER(VisibilitySelectDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_model_visibility_reset": ([vp, cp], C.c_int32),
        "gsx_depth_map_desc_default": ([C.POINTER(DepthMapDesc)], None),
        "gsx_render_depth_map": ([vp, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(DepthMapDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.POINTER(DepthMapStats)], C.c_int32),
        "gsx_depth_map_device_ptrs": ([vp] + [C.POINTER(C.c_void_p)] * 7 + [C.POINTER(C.c_uint32)] * 2, C.c_int32),
        "gsx_depth_map_unproject": ([C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                     C.POINTER(C.c_float)], C.c_int32),
        "gsx_decimate_desc_default": ([C.POINTER(DecimateDesc)], None),
        "gsx_model_decimate": ([vp, cp, cp, C.POINTER(DecimateDesc), C.c_void_p, C.POINTER(DecimateStats)], C.c_int32),
        "gsx_model_decimate_edge": ([vp, cp, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint64)], C.c_int32),
        "gsx_model_merge": ([vp, C.POINTER(C.c_char_p), C.c_uint32, cp, C.POINTER(ExtractDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int32),
    }
    assert set(sig) == set(EXPORTS)
    for name, (args, res) in sig.items():
        if name in MAY_LACK and not hasattr(L, name):
            continue
        fn = getattr(L, name)  # AttributeError here = the library does not export what gsx.h declares
        fn.argtypes = args
        fn.restype = res
    if L.gsx_abi_version() != GSX_ABI_VERSION:
        raise ImportError(f"libgsx ABI {L.gsx_abi_version()} != binding {GSX_ABI_VERSION}")
    _lib = L
    return L


def check(status: int) -> None:
    if status != GSX_OK:
        raise GsxError(status, load().gsx_last_error_string().decode("utf-8", "replace"))
