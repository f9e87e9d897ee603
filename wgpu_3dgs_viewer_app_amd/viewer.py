"""Host-side mirror of the ``wgpu-3dgs-viewer`` (``gs::``) surface the app uses for the render path.

The reference's host language is Rust (no toolchain in this image), so this mirror over the C ABI is
Python; names, argument order and error behaviour follow the reference call sites so tests read like
the app's frame loop (src/tab/scene.rs:699-874, 2263-2326):

    viewer = MultiModelViewer(size=(1, 1))                      # MultiModelViewer::new_with   scene.rs:1969
    viewer.add_model("a", count)                                # new_empty + BindGroups::new   scene.rs:2111
    viewer.models["a"].gaussian_buffers.gaussians_buffer.update_range(start, gaussians)  # scene.rs:2083
    viewer.update_camera(camera, (w, h))                        # scene.rs:795
    viewer.update_model_transform("a", pos, quat, scale)        # scene.rs:796
    viewer.update_gaussian_transform(1.0, Splat, GaussianShDegree.new(3), False)  # scene.rs:803
    viewer.preprocessor.preprocess("a"); viewer.radix_sorter.sort("a")           # scene.rs:856, 865
    viewer.poll()                                               # device.poll(Maintain::Wait)    scene.rs:873
    viewer.renderer.render(keys_far_to_near)                    # render_with_pass loop          scene.rs:2302

Every call goes into libgsx.so (HIP kernels); nothing here computes pixels.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
from typing import Iterable, Sequence

import numpy as np

from . import _lib
from ._lib import GsxError, SpecParams  # noqa: F401  (re-exported)
from .scene import GAUSSIAN_DTYPE


class GaussianDisplayMode(enum.IntEnum):
    """``gs::GaussianDisplayMode`` (src/app.rs:1147, src/tab/transform.rs:106-146)."""

    Splat = 0
    Ellipse = 1
    Point = 2


class GaussianShDegree:
    """``gs::GaussianShDegree``: 0..=3; ``new`` returns ``None`` out of range (src/tab/transform.rs:139)."""

    def __init__(self, deg: int):
        self.deg = int(deg)

    @classmethod
    def new(cls, deg: int):
        return cls(deg) if 0 <= int(deg) <= 3 else None

    @classmethod
    def new_unchecked(cls, deg: int) -> "GaussianShDegree":
        return cls(deg)

    def degree(self) -> int:
        return self.deg


class DepthCompare(enum.IntEnum):
    """``wgpu::CompareFunction`` of the viewer's depth test (gsx_depth_compare): Always = no test, Less = the reference's."""

    Always = 0
    Less = 1


class ShKind(enum.IntEnum):
    """``GaussianSh{Single,Half,Norm8,None}Config`` (src/app.rs:386-403)."""

    Single = 0
    Half = 1
    Norm8 = 2
    Remove = 3


class Cov3dKind(enum.IntEnum):
    """``GaussianCov3d{Single,Half}Config`` (src/app.rs:405-418)."""

    Single = 0
    Half = 1


#: ``gsx_overlay_line``: the reference's measurement ``HitPair`` (src/renderer/measurement.rs:177-184), 32 bytes
HIT_PAIR_DTYPE = np.dtype([("p0", "<f4", 3), ("color", "u1", 4), ("p1", "<f4", 3), ("line_width", "<f4")])


def HitPair(p0, p1, color=(255, 255, 255, 255), line_width: float = 1.0) -> np.ndarray:
    """One measurement line as a 32-byte record: world-space ends ``p0`` / ``p1``, an RGBA8 colour, a width (its on-screen
    half-width at an end is ``0.01 * line_width * height / (2 * distance from the eye)``).  Concatenate records (or pass a
    list of them) to ``MultiModelViewer.update_hit_pairs``."""
    r = np.zeros(1, HIT_PAIR_DTYPE)
    r["p0"] = np.asarray(p0, np.float32)
    r["p1"] = np.asarray(p1, np.float32)
    r["color"] = np.asarray(color, np.uint8)
    r["line_width"] = np.float32(line_width)
    return r


#: ``gsx_mask_gizmo``: a world-space mask shape, its straight RGBA colour in [0, 1] and a width in ``HitPair.line_width`` units, 64 bytes
MASK_GIZMO_DTYPE = np.dtype([("kind", "<u4"), ("pos", "<f4", 3), ("quat_xyzw", "<f4", 4), ("scale", "<f4", 3), ("color", "<f4", 4),
                             ("line_width", "<f4")])


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class GaussiansBuffer:
    """``gs::GaussiansBuffer<G>``: the model's resident pod planes in HBM."""

    def __init__(self, viewer: "MultiModelViewer", key: str):
        self._v, self._key = viewer, key

    def len(self) -> int:
        n = C.c_uint64()
        _lib.check(self._v._L.gsx_model_len(self._v._h, self._key.encode(), C.byref(n)))
        return int(n.value)

    __len__ = len

    def update_range(self, start: int, gaussians: np.ndarray) -> None:
        """``gaussians_buffer.update_range(queue, start, &[gs::Gaussian])`` (src/tab/scene.rs:2083-2084)."""
        g = np.ascontiguousarray(gaussians, dtype=GAUSSIAN_DTYPE)
        _lib.check(self._v._L.gsx_model_upload_range(self._v._h, self._key.encode(), int(start), g.ctypes.data, g.shape[0]))

    def update_range_ply(self, start: int, rows, header, staging_bytes: int = 0) -> None:
        """``gsx_model_upload_ply_rows``: binary PLY vertex rows (a bytes-like object of ``header.raw.vertex_bytes`` each; ``header`` a
        ``ply.PlyHeader`` or a ``_lib.PlyHeader``) decoded on the device into the Gaussians from ``start`` on: ``update_range`` of the
        rows' Gaussians without the records in between (spec §15)."""
        raw = getattr(header, "raw", header)
        buf = np.frombuffer(rows, dtype=np.uint8)
        if raw.vertex_bytes == 0 or buf.size % raw.vertex_bytes:
            raise ValueError("rows must be whole vertices of header.vertex_bytes bytes")
        desc = _lib.ImportDesc(0, 0, int(staging_bytes))
        _lib.check(self._v._L.gsx_model_upload_ply_rows(self._v._h, self._key.encode(), int(start), buf.ctypes.data if buf.size else None,
                                                        buf.size // raw.vertex_bytes, C.byref(raw), C.byref(desc)))

    def update_range_pod_device(self, start: int, n: int, d_pos: int, d_color: int, d_sh: int, d_cov3d: int) -> None:
        """Zero-copy upload of pod planes that already live in device memory (raw device pointers)."""
        _lib.check(self._v._L.gsx_model_upload_pod_device(self._v._h, self._key.encode(), int(start), int(n), d_pos,
                                                          d_color, d_sh, d_cov3d))

    def download_pod(self):
        n = self.len()
        pos = np.empty((n, 3), np.float32)
        color = np.empty(n, np.uint32)
        sh = np.empty((n, 45), np.float32)
        cov = np.empty((n, 6), np.float32)
        _lib.check(self._v._L.gsx_model_download_pod(self._v._h, self._key.encode(), _f32p(pos), _u32p(color), _f32p(sh), _f32p(cov)))
        return pos, color, sh, cov


class BufferHandle:
    """A cloned buffer handle (``buffer.clone()`` in the app, src/app.rs:769-780): owns a device-side snapshot of the buffer as
    of the clone; ``download()`` may run on any thread while the viewer keeps rendering (``gsx_buffer_*``)."""

    KINDS = {"mask": 0, "edits": 1, "selection": 2}

    def __init__(self, viewer: "MultiModelViewer", key: str, kind: str):
        self._L, self.kind = viewer._L, kind
        self._h = C.c_void_p()
        _lib.check(self._L.gsx_model_buffer_retain(viewer._h, key.encode(), self.KINDS[kind], C.byref(self._h)))

    def clone(self) -> "BufferHandle":
        other = object.__new__(BufferHandle)
        other._L, other.kind, other._h = self._L, self.kind, C.c_void_p(self._h.value)
        _lib.check(self._L.gsx_buffer_retain(self._h))
        return other

    def len(self) -> int:
        n = C.c_uint64()
        _lib.check(self._L.gsx_buffer_len(self._h, C.byref(n)))
        return int(n.value)

    def download(self) -> np.ndarray:
        if self.kind == "edits":
            from .query import EDIT_DTYPE

            out = np.zeros(self.len(), EDIT_DTYPE)
        else:
            out = np.empty(self.len(), np.uint32)
        _lib.check(self._L.gsx_buffer_download(self._h, out.ctypes.data, out.size))
        return out

    def release(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.gsx_buffer_release(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class MaskBuffer:
    """``gs::MaskBuffer``: one bit per Gaussian, 1 = kept (src/tab/scene.rs:1851, src/app.rs:806-807)."""

    def __init__(self, viewer: "MultiModelViewer", key: str):
        self._v, self._key = viewer, key

    def upload(self, words: np.ndarray | None) -> None:
        if words is None:
            _lib.check(self._v._L.gsx_model_upload_mask(self._v._h, self._key.encode(), None, 0))
            return
        w = np.ascontiguousarray(words, dtype=np.uint32)
        _lib.check(self._v._L.gsx_model_upload_mask(self._v._h, self._key.encode(), _u32p(w), w.size))

    def download(self) -> np.ndarray:
        n = (self._v.models[self._key].gaussian_buffers.gaussians_buffer.len() + 31) // 32
        w = np.empty(n, np.uint32)
        _lib.check(self._v._L.gsx_model_download_mask(self._v._h, self._key.encode(), _u32p(w), n))
        return w

    def clone(self) -> BufferHandle:
        """``mask_buffer.clone()`` (src/app.rs:775): a handle for a download on another thread."""
        return BufferHandle(self._v, self._key, "mask")


class SelectionBuffer:
    """``gs::SelectionBuffer``: one bit per Gaussian, 1 = selected (src/tab/scene.rs:1846-1850)."""

    def __init__(self, viewer: "MultiModelViewer", key: str):
        self._v, self._key = viewer, key

    def upload(self, words: np.ndarray | None) -> None:
        if words is None:
            _lib.check(self._v._L.gsx_model_upload_selection(self._v._h, self._key.encode(), None, 0))
            return
        w = np.ascontiguousarray(words, dtype=np.uint32)
        _lib.check(self._v._L.gsx_model_upload_selection(self._v._h, self._key.encode(), _u32p(w), w.size))

    def download(self) -> np.ndarray:
        n = (self._v.models[self._key].gaussian_buffers.gaussians_buffer.len() + 31) // 32
        w = np.empty(n, np.uint32)
        _lib.check(self._v._L.gsx_model_download_selection(self._v._h, self._key.encode(), _u32p(w), n))
        return w

    def clone(self) -> BufferHandle:
        return BufferHandle(self._v, self._key, "selection")


class GaussiansEditBuffer:
    """``gs::GaussiansEditBuffer``: one ``GaussianEditPod`` per Gaussian (src/tab/scene.rs:1816-1830, app.rs:789)."""

    def __init__(self, viewer: "MultiModelViewer", key: str):
        self._v, self._key = viewer, key

    def download(self) -> np.ndarray:
        from .query import EDIT_DTYPE

        n = self._v.models[self._key].gaussian_buffers.gaussians_buffer.len()
        out = np.zeros(n, EDIT_DTYPE)
        _lib.check(self._v._L.gsx_model_download_edits(self._v._h, self._key.encode(), out.ctypes.data, n))
        return out

    def clone(self) -> BufferHandle:
        """``gaussians_edit_buffer.clone()`` (src/app.rs:772): a handle for a download on another thread."""
        return BufferHandle(self._v, self._key, "edits")

    def upload(self, edits: np.ndarray | None) -> None:
        from .query import EDIT_DTYPE

        if edits is None:
            _lib.check(self._v._L.gsx_model_upload_edits(self._v._h, self._key.encode(), None, 0))
            return
        e = np.ascontiguousarray(edits, EDIT_DTYPE)
        _lib.check(self._v._L.gsx_model_upload_edits(self._v._h, self._key.encode(), e.ctypes.data, e.size))


class MultiModelViewerGaussianBuffers:
    """``gs::MultiModelViewerGaussianBuffers<G>`` (src/tab/scene.rs:2111-2112)."""

    def __init__(self, viewer: "MultiModelViewer", key: str):
        self.gaussians_buffer = GaussiansBuffer(viewer, key)
        self.mask_buffer = MaskBuffer(viewer, key)
        self.selection_buffer = SelectionBuffer(viewer, key)
        self.gaussians_edit_buffer = GaussiansEditBuffer(viewer, key)


@dataclasses.dataclass
class ModelBounds:
    """``gsx_model_bounds_t``: what ``MultiModelViewerModel.bounds`` returns.  Model space, Gaussian centres only; the vectors
    are float32[3].  ``center`` is ``GaussianSplattingModel::center`` (src/app.rs:1019-1046)."""

    count: int
    n_nonfinite: int
    min: np.ndarray
    max: np.ndarray
    center: np.ndarray
    mean: np.ndarray
    trim_min: np.ndarray
    trim_max: np.ndarray


@dataclasses.dataclass
class PropertyHistogram:
    """``gsx_histogram_t`` and its bins: what ``MultiModelViewerModel.histogram`` returns.  ``count``: Gaussians that pass the filter
    and have a finite value; ``below`` / ``above``: those of them outside ``[lo, hi]``; ``bins`` (uint64) holds the others;
    ``n_nonfinite``: NaN and infinities; ``min`` / ``max``: exact over the counted values."""

    bins: np.ndarray
    count: int
    below: int
    above: int
    n_nonfinite: int
    lo: np.float32
    hi: np.float32
    min: np.float32
    max: np.float32


@dataclasses.dataclass
class ModelNeighbors:
    """What ``MultiModelViewerModel.neighbors`` returns.  ``counts`` (uint32, one per Gaussian): neighbours within the radius,
    saturated at the cap, 0 for a Gaussian that does not participate; ``hist`` (uint64, cap + 1): participants per count; ``count``:
    participants (pass the filter, finite position); ``n_nonfinite``: passed the filter with a NaN or infinite coordinate;
    ``grid_bits``: the hash table used."""

    counts: np.ndarray
    hist: np.ndarray
    count: int
    n_nonfinite: int
    grid_bits: int


@dataclasses.dataclass
class ModelClusters:
    """What ``MultiModelViewerModel.clusters`` returns.  ``labels`` (uint32, one per Gaussian): the smallest Gaussian index of its
    cluster, ``_lib.GSX_CLUSTER_NONE`` for a Gaussian that does not participate; ``sizes`` (uint32): the size of its cluster, 0 for
    one that does not participate; ``count``: participants (pass the filter, finite position); ``n_nonfinite``: passed the filter
    with a NaN or infinite coordinate; ``n_clusters``; ``largest_size`` and ``largest_label``: the largest cluster (the smallest
    label on a tie; ``GSX_CLUSTER_NONE`` without participants); ``grid_bits``: the hash table used."""

    labels: np.ndarray
    sizes: np.ndarray
    count: int
    n_nonfinite: int
    n_clusters: int
    largest_size: int
    largest_label: int
    grid_bits: int


@dataclasses.dataclass
class ModelKnn:
    """What ``MultiModelViewerModel.knn`` returns.  ``d2`` (float32, ``(n, k)``, or ``None`` without ``rows=True``): every Gaussian's k
    smallest squared distances to the other participants, ascending, ``+inf`` where there are fewer and for a Gaussian that does not
    participate; ``score`` (float32, one per Gaussian): the distance to the k-th nearest or the mean distance to the k nearest,
    ``+inf`` where the row holds one; ``count``: participants (pass the filter, finite position); ``n_nonfinite``; ``n_scored``,
    ``score_min``, ``score_max``, ``mean``, ``std`` (the sample deviation): over the finite scores; ``first_radius``, ``rounds``,
    ``n_brute``, ``grid_bits``: what the search ran (they may differ with the knobs; nothing else does)."""

    d2: np.ndarray | None
    score: np.ndarray
    count: int
    n_nonfinite: int
    n_scored: int
    score_min: np.float32
    score_max: np.float32
    mean: float
    std: float
    threshold: np.float32
    first_radius: np.float32
    rounds: int
    n_brute: int
    grid_bits: int


def _knn_stats(out, d2, score) -> ModelKnn:
    return ModelKnn(d2, score, int(out.count), int(out.n_nonfinite), int(out.n_scored), np.float32(out.score_min), np.float32(out.score_max),
                    float(out.mean), float(out.std), np.float32(out.threshold), np.float32(out.first_radius), int(out.rounds),
                    int(out.n_brute), int(out.grid_bits))


@dataclasses.dataclass
class ModelNormals:
    """What ``MultiModelViewerModel.normals`` returns.  ``normal`` (float32, ``(n, 3)``): the unit normal of the plane fitted to every
    Gaussian and its k nearest, ``(0, 0, 0)`` where none is fitted; ``variation`` (float32, one per Gaussian): the smallest
    eigenvalue's share of the neighbourhood's scatter, 0 on a plane, 1/3 where it is isotropic, ``+inf`` where none is fitted;
    ``index`` (uint32, ``(n, k)``, or ``None`` without ``indices=True``): the k nearest by (squared distance, index),
    ``_lib.GSX_NORMALS_NONE`` where there is none; ``count``: participants; ``n_nonfinite``; ``n_fitted``, ``variation_min``,
    ``variation_max``, ``mean``: over the fitted; ``first_radius``, ``rounds``, ``n_brute``, ``grid_bits``: what the search ran (they
    may differ with the knobs; nothing else does)."""

    normal: np.ndarray | None
    variation: np.ndarray | None
    index: np.ndarray | None
    count: int
    n_nonfinite: int
    n_fitted: int
    variation_min: np.float32
    variation_max: np.float32
    mean: float
    first_radius: np.float32
    rounds: int
    n_brute: int
    grid_bits: int


def _normals_stats(out, normal, variation, index) -> ModelNormals:
    return ModelNormals(normal, variation, index, int(out.count), int(out.n_nonfinite), int(out.n_fitted), np.float32(out.variation_min),
                        np.float32(out.variation_max), float(out.mean), np.float32(out.first_radius), int(out.rounds), int(out.n_brute),
                        int(out.grid_bits))


@dataclasses.dataclass
class ModelNearest:
    """What ``MultiModelViewerModel.nearest`` returns.  ``index`` (uint32, one per Gaussian of this model, or ``None``): the nearest
    participating Gaussian of the target model, ``_lib.GSX_NEAREST_NONE`` where this one does not participate or nothing is in
    reach; ``d2`` (float32): the squared distance in the target's model space, ``+inf`` there; ``count`` / ``n_nonfinite``: the
    participating queries and those that pass the filter without a finite position; ``targets`` / ``targets_nonfinite``: the same
    of the target model; ``n_found``; ``d_min``, ``d_max`` (the one-sided Hausdorff distance), ``mean`` (the one-sided chamfer
    distance), ``rms``: over the found queries; ``first_radius``, ``rounds``, ``n_brute``, ``grid_bits``: what the search ran;
    ``xform`` (float32, ``(3, 4)``): the matrix used."""

    index: np.ndarray | None
    d2: np.ndarray | None
    count: int
    n_nonfinite: int
    targets: int
    targets_nonfinite: int
    n_found: int
    d_min: np.float32
    d_max: np.float32
    mean: float
    rms: float
    first_radius: np.float32
    rounds: int
    n_brute: int
    grid_bits: int
    xform: np.ndarray


def _nearest_stats(out, index, d2) -> ModelNearest:
    return ModelNearest(index, d2, int(out.count), int(out.n_nonfinite), int(out.targets), int(out.targets_nonfinite), int(out.n_found),
                        np.float32(out.d_min), np.float32(out.d_max), float(out.mean), float(out.rms), np.float32(out.first_radius),
                        int(out.rounds), int(out.n_brute), int(out.grid_bits), np.array(out.xform[:], np.float32).reshape(3, 4))


def _nearest_desc(xform, model_transforms, src_filter, dst_filter, max_distance, radius_hint, grid_bits, max_rounds) -> "_lib.NearestDesc":
    m = np.eye(3, 4, dtype=np.float32) if xform is None else np.ascontiguousarray(xform, np.float32).reshape(3, 4)
    return _lib.NearestDesc(int(src_filter), int(dst_filter), _lib.GSX_NEAREST_MODEL_TRANSFORMS if model_transforms else 0, int(grid_bits),
                            float(max_distance), float(radius_hint), int(max_rounds), 0, (C.c_float * 12)(*m.reshape(-1)))


@dataclasses.dataclass
class ModelAlignStep:
    """What ``MultiModelViewerModel.align_step`` returns: the delta ``t ~ scale * R(quat) q + pos`` in the target's model space
    (``quat`` x, y, z, w with w >= 0; float64), ``xform_next`` (float32, ``(3, 4)``) = delta o the matrix used, the next step's ``xform``;
    ``n_pairs``; ``rms_before``: the pairs' rms distance before the step; ``degenerate``: too few pairs or no single best rotation,
    the delta is the identity; ``nearest``: the search's statistics, without arrays."""

    pos: np.ndarray
    quat: np.ndarray
    scale: float
    xform_next: np.ndarray
    n_pairs: int
    rms_before: float
    degenerate: bool
    nearest: ModelNearest


@dataclasses.dataclass
class ModelNormalsKept:
    """What ``MultiModelViewerModel.kept_normals`` returns: ``present``; the ``k``, ``orient`` (``_lib.GSX_NORMALS_ORIENT_*``),
    ``filter`` and ``toward`` the plane was made with; ``count``: the model's Gaussians then; ``n_fitted``; ``normal`` (float32,
    ``(n, 3)``) and ``variation`` (float32, ``n``): the resident plane's contents, ``None`` without a plane or with ``rows=False``."""

    present: bool
    k: int
    orient: int
    filter: int
    toward: np.ndarray
    count: int
    n_fitted: int
    normal: np.ndarray | None
    variation: np.ndarray | None


@dataclasses.dataclass
class ModelPlaneFit:
    """What ``MultiModelViewerModel.fit_plane`` returns.  ``plane`` and ``candidate`` are float32 ``(nx, ny, nz, offset)``: the points
    ``p`` with ``n . p = offset`` in model space, the result and the winning candidate; ``winner`` its index (``None`` without a valid
    candidate); ``n_valid`` candidates; ``count`` participants; ``n_nonfinite``; ``candidate_inliers``; ``n_inliers`` (never fewer); of
    the last accepted refine round ``centroid`` (float32), ``eigenvalues`` (float64, descending), ``rms`` and ``sums`` (float64, 10: sum p,
    the scatter xx xy xz yy yz zz, sum r^2); ``refine_done``; ``degenerate``; ``candidates`` (float32, ``(H, 4)``) and ``counts``
    (uint32, ``H``): every candidate and its exact inlier count, ``None`` with ``rows=False``."""

    plane: np.ndarray
    candidate: np.ndarray
    winner: int | None
    n_valid: int
    count: int
    n_nonfinite: int
    candidate_inliers: int
    n_inliers: int
    centroid: np.ndarray
    eigenvalues: np.ndarray
    rms: float
    sums: np.ndarray
    refine_done: int
    degenerate: bool
    candidates: np.ndarray | None
    counts: np.ndarray | None


def plane_level(plane, up=(0.0, 0.0, 1.0)) -> tuple[np.ndarray, np.ndarray]:
    """``gsx_plane_level`` (host only): ``(quat, pos)``, float32 — the shortest-arc rotation (x, y, z, w; w >= 0) that takes the unit
    normal of ``plane`` (``nx, ny, nz, offset``) to ``up / |up|``, and the translation that puts the rotated plane through the
    origin's height: what ``update_model_transform`` or ``apply_transform`` takes with scale 1 to stand a capture level."""
    pl = np.ascontiguousarray(plane, np.float32).reshape(4)
    c_plane = _lib.Plane((C.c_float * 3)(*[float(x) for x in pl[:3]]), float(pl[3]))
    c_up = (C.c_float * 3)(*[float(x) for x in up])
    quat, pos = (C.c_float * 4)(), (C.c_float * 3)()
    _lib.check(_lib.load().gsx_plane_level(C.byref(c_plane), C.byref(c_up), C.byref(quat), C.byref(pos)))
    return np.array(quat[:], np.float32), np.array(pos[:], np.float32)


@dataclasses.dataclass
class ModelAlignPlaneStep:
    """What ``MultiModelViewerModel.align_plane_step`` returns: the delta ``t ~ R(quat) q + pos`` in the target's model space (``quat``
    x, y, z, w with w >= 0; float64); ``normal_matrix`` (float64, 21: the upper triangle of the 6x6 ``A = sum J J^T`` over
    ``(omega, tau)``, row-major), ``rhs`` (``b``), ``eigenvalues`` (descending), ``centre``; ``rms_before`` and ``rms_plane_before``: the
    used pairs' rms distance and rms distance along the target's normal before the step; ``n_pairs`` used and ``n_unfitted`` left
    out; ``xform_next`` (float32, ``(3, 4)``); ``rank``: how many of the six motions the pairs determine; ``degenerate``; ``nearest``:
    the search's statistics, without arrays.  ``matrix()`` is ``A`` in full."""

    pos: np.ndarray
    quat: np.ndarray
    normal_matrix: np.ndarray
    rhs: np.ndarray
    eigenvalues: np.ndarray
    centre: np.ndarray
    rms_before: float
    rms_plane_before: float
    n_pairs: int
    n_unfitted: int
    xform_next: np.ndarray
    rank: int
    degenerate: bool
    nearest: ModelNearest
    scale: float = 1.0

    def matrix(self) -> np.ndarray:
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = self.normal_matrix
        return A + np.triu(A, 1).T


def _compose34(a, b):
    """a o b of two 3x4 similarities, in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]], axis=1)


@dataclasses.dataclass
class ModelVisibility:
    """What ``MultiModelViewerModel.visibility`` returns: the model's resident planes after the call and this view's statistics.
    ``peak`` (float32, one per Gaussian, or ``None``): the largest blending weight ``T * alpha`` any pixel of any folded view gave
    it; ``weight`` (float64): the sum of those weights over the pixels, in 2^-24 fixed point; ``pixels`` (uint32): the pixels that
    blended it; ``transmittance`` (float32 ``(H, W)``, or ``None``): the final ``T`` of every pixel of THIS view; ``n_visible``: after
    cull, this view; ``n_seen``: Gaussians with ``peak > 0``; ``n_pairs`` and ``weight_fixed``: this view's blended (pixel, Gaussian)
    pairs and the integer sum of their fixed-point weights; ``peak_max``; ``views``: the views folded into the planes."""

    peak: np.ndarray | None
    weight: np.ndarray | None
    pixels: np.ndarray | None
    transmittance: np.ndarray | None
    n_visible: int
    n_seen: int
    n_pairs: int
    weight_fixed: int
    peak_max: np.float32
    views: int


@dataclasses.dataclass
class DepthMap:
    """What ``MultiModelViewer.render_depth_map`` returns: per pixel, ``(H, W)`` arrays (or ``None`` with ``planes=False``).
    ``surface`` (float32): the view depth of the first record after whose blend ``T < threshold``, ``inf`` without such a crossing;
    ``sum`` and ``alpha`` (float32): ``S = sum w * d`` and ``A = sum w`` in walk order — the expected depth is ``sum / alpha`` where
    ``alpha > 0``; ``transmittance`` (float32): the final ``T``, the rendered frame's bit for bit; ``index`` and ``layer`` (uint32):
    the surface record's Gaussian index and its model's position in the keys, ``_lib.GSX_DEPTH_MAP_NONE`` without a crossing;
    ``n_covered``: pixels with ``alpha > 0``; ``n_crossed``: pixels with a crossing; ``surface_min`` / ``surface_max`` over the
    crossings; ``models``."""

    surface: np.ndarray | None
    sum: np.ndarray | None
    alpha: np.ndarray | None
    transmittance: np.ndarray | None
    index: np.ndarray | None
    layer: np.ndarray | None
    n_covered: int
    n_crossed: int
    surface_min: np.float32
    surface_max: np.float32
    models: int


def depth_map_unproject(view, proj, size, px: float, py: float, view_depth: float) -> np.ndarray:
    """``gsx_depth_map_unproject`` (host only): the world-space point the camera sees at pixel position ``(px, py)`` — pixel
    ``(i, j)`` has its centre at ``(i + 0.5, j + 0.5)`` — at view depth ``view_depth`` (a value of ``DepthMap.surface``)."""
    v = np.ascontiguousarray(view, np.float32).reshape(16)
    p = np.ascontiguousarray(proj, np.float32).reshape(16)
    out = np.empty(3, np.float32)
    _lib.check(_lib.load().gsx_depth_map_unproject(_f32p(v), _f32p(p), int(size[0]), int(size[1]), float(px), float(py), float(view_depth), _f32p(out)))
    return out


@dataclasses.dataclass
class ModelDecimate:
    """What ``MultiModelViewerModel.decimate`` and ``decimate_count`` return.  ``count``: participants (pass the filter, finite
    position); ``n_nonfinite``: passed the filter with a NaN or infinite coordinate (dropped); ``cells``: occupied cells, the new
    model's length; ``singletons``: one-member cells; ``largest_cell``: the largest member count; ``grid_bits``: the hash table used;
    ``map`` (uint32, one per source Gaussian, or ``None``): the index in the new model it went into, ``_lib.GSX_DECIMATE_NO_CELL``
    where it does not participate."""

    count: int
    n_nonfinite: int
    cells: int
    singletons: int
    largest_cell: int
    grid_bits: int
    map: np.ndarray | None


class MultiModelViewerModel:
    """``gs::MultiModelViewerModel {gaussian_buffers, bind_groups}`` (src/tab/scene.rs:2133-2139)."""

    def __init__(self, viewer: "MultiModelViewer", key: str):
        self.gaussian_buffers = MultiModelViewerGaussianBuffers(viewer, key)
        self._v, self._key = viewer, key

    def bounds(self, masked: bool = False, skip_hidden: bool = False, selected: bool = False, trim_permille: int = 0) -> ModelBounds:
        """``gsx_model_bounds``: the box, its centre, the centroid and the trimmed box of the model's Gaussian centres, computed on
        the device from the resident positions.  ``masked``: only what the model's mask keeps; ``skip_hidden``: without the
        Gaussians whose stored edit hides them; ``selected``: only the selection; ``trim_permille`` (< 500): per axis the trimmed box
        leaves at most ``count * trim_permille // 1000`` of the counted Gaussians below it and as many above.  After the last
        ``update_range`` of a load, ``model.center = viewer.models[key].bounds().center`` (the reference leaves it zero)."""
        desc = _lib.BoundsDesc((_lib.GSX_BOUNDS_MASKED if masked else 0) | (_lib.GSX_BOUNDS_SKIP_HIDDEN if skip_hidden else 0)
                               | (_lib.GSX_BOUNDS_SELECTED if selected else 0), int(trim_permille))
        out = _lib.ModelBounds()
        _lib.check(self._v._L.gsx_model_bounds(self._v._h, self._key.encode(), C.byref(desc), C.byref(out)))
        vec = lambda a: np.array(a[:], np.float32)  # noqa: E731
        return ModelBounds(int(out.count), int(out.n_nonfinite), vec(out.min), vec(out.max), vec(out.center), vec(out.mean),
                           vec(out.trim_min), vec(out.trim_max))

    def extract(self, dst_key: str, filter: int = 0, invert: bool = False, drop_edits: bool = False) -> int:  # noqa: A002
        """``gsx_model_extract``: the Gaussians of this model that pass ``filter`` (``_lib.GSX_BOUNDS_*`` bits, with ``bounds``'
        meaning; ``invert``: exactly those that do not) become the new model ``dst_key``, in their order, on the device: every
        resident plane as stored bits, the model transform, and the stored edit records unless ``drop_edits``.  Returns the number
        kept; 0 creates no model.  The new model is ``viewer.models[dst_key]``.  "Separate selection into a model" is
        ``extract(a, SELECTED)`` and ``extract(b, SELECTED, invert=True)``; "apply the mask" is ``extract(a, MASKED | SKIP_HIDDEN)``
        and ``viewer.remove_model`` of this one."""
        desc = _lib.ExtractDesc(int(filter), (_lib.GSX_EXTRACT_INVERT if invert else 0) | (_lib.GSX_EXTRACT_DROP_EDITS if drop_edits else 0))
        count = C.c_uint64()
        _lib.check(self._v._L.gsx_model_extract(self._v._h, self._key.encode(), dst_key.encode(), C.byref(desc), C.byref(count)))
        if count.value:
            self._v.models[dst_key] = MultiModelViewerModel(self._v, dst_key)
        return int(count.value)

    @property
    def pod_kind(self):
        """``gsx_model_pod_kind``: the ``(ShKind, Cov3dKind)`` this model's planes are stored in: the kinds it was created with, or
        those of the last ``set_pod_kind``."""
        sh, cov = C.c_int32(), C.c_int32()
        _lib.check(self._v._L.gsx_model_pod_kind(self._v._h, self._key.encode(), C.byref(sh), C.byref(cov)))
        return ShKind(sh.value), Cov3dKind(cov.value)

    def convert(self, dst_key: str, sh, cov3d, filter: int = 0, invert: bool = False, drop_edits: bool = False) -> int:  # noqa: A002
        """``gsx_model_convert``: ``extract`` into a model of the pod kind ``(sh, cov3d)``: the same kept set, order, transform and
        edit records; position and colour word carried, covariance and SH dequantised exactly and quantised once into the new kind
        (what an upload of this model's ``download_pod`` into a model of that kind stores), on the device.  The same kind is
        ``extract``.  Returns the number kept; 0 creates no model.  "Convert, then merge" joins models of different kinds."""
        desc = _lib.ConvertDesc(int(filter), (_lib.GSX_EXTRACT_INVERT if invert else 0) | (_lib.GSX_EXTRACT_DROP_EDITS if drop_edits else 0),
                                int(sh), int(cov3d))
        count = C.c_uint64()
        _lib.check(self._v._L.gsx_model_convert(self._v._h, self._key.encode(), dst_key.encode(), C.byref(desc), C.byref(count)))
        if count.value:
            self._v.models[dst_key] = MultiModelViewerModel(self._v, dst_key)
        return int(count.value)

    def set_pod_kind(self, sh, cov3d) -> None:
        """``gsx_model_set_pod_kind``: the app's Compression Settings applied to this loaded model: its planes become what
        ``convert`` makes, under the same key; length, transform, mask, selection, edit records and ``show_unedited`` stay (the
        buffers are moved).  The next frame is an unspeculated one.  The same kind does nothing."""
        _lib.check(self._v._L.gsx_model_set_pod_kind(self._v._h, self._key.encode(), int(sh), int(cov3d)))

    def apply_transform(self, pos=(0.0, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0), scale=(1.0, 1.0, 1.0), pivot=(0.0, 0.0, 0.0),
                        filter: int = 0, invert: bool = False) -> int:  # noqa: A002
        """``gsx_model_apply_transform``: the Gaussians that pass ``filter`` (``_lib.GSX_BOUNDS_*`` bits, ``extract``'s kept set;
        ``invert``: exactly those that do not) are moved, rotated, scaled or mirrored about ``pivot`` where they lie, on the device:
        positions, covariances, SH and shade records as ``merge`` bakes a model transform (``quat`` x, y, z, w, taken as given).
        The Gaussian order, the mask, the selection, the edit records and the model transform stay.  A translation writes
        positions only; the identity writes nothing.  "Rotate the selection about its centre":
        ``pivot=model.bounds(selected=True).center, filter=GSX_BOUNDS_SELECTED``.  Returns the number of Gaussians moved."""
        f3 = lambda a: (C.c_float * 3)(*(float(x) for x in a))  # noqa: E731
        desc = _lib.TransformDesc(int(filter), _lib.GSX_EXTRACT_INVERT if invert else 0, f3(pos), (C.c_float * 4)(*(float(x) for x in quat)),
                                  f3(scale), f3(pivot), 0)
        count = C.c_uint64()
        _lib.check(self._v._L.gsx_model_apply_transform(self._v._h, self._key.encode(), C.byref(desc), C.byref(count)))
        return int(count.value)

    def property_values(self, prop: int, world: bool = False) -> np.ndarray:
        """``gsx_model_property_values``: the property ``prop`` (``_lib.GSX_PROP_*``) of every Gaussian as float32, computed on the
        device from the stored values (edits are not applied): the stored position (``world``: with the model transform applied as
        ``merge`` bakes it), the bytes of the colour word / 255, their HSV, or the scales ``export`` solves from the covariance."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        out = np.empty(n, np.float32)
        _lib.check(self._v._L.gsx_model_property_values(self._v._h, self._key.encode(), int(prop), _lib.GSX_PROP_WORLD if world else 0,
                                                        out.ctypes.data, n))
        return out

    def histogram(self, prop: int, bins: int, lo: float | None = None, hi: float | None = None, filter: int = 0,  # noqa: A002
                  world: bool = False) -> PropertyHistogram:
        """``gsx_model_histogram``: ``bins`` (1..4096) equal bins of the property over ``[lo, hi]`` — or, with both ``None``, over
        the ``[min, max]`` of the counted values — among the Gaussians that pass ``filter`` (``_lib.GSX_BOUNDS_*``) and have a finite
        value.  Returns the bins, ``count``, ``below``, ``above``, ``n_nonfinite``, the range used and the exact ``min`` / ``max``;
        ``bins.sum() == count - below - above``.  Pass the returned ``lo`` / ``hi`` to ``select_range``."""
        auto = lo is None and hi is None
        desc = _lib.HistogramDesc(int(prop), (_lib.GSX_PROP_WORLD if world else 0) | (_lib.GSX_HIST_AUTO_RANGE if auto else 0), int(filter),
                                  int(bins), 0.0 if auto else float(lo), 0.0 if auto else float(hi))
        counts = np.zeros(max(int(bins), 1), np.uint64)
        out = _lib.Histogram()
        _lib.check(self._v._L.gsx_model_histogram(self._v._h, self._key.encode(), C.byref(desc), counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  C.byref(out)))
        return PropertyHistogram(counts, int(out.count), int(out.below), int(out.above), int(out.n_nonfinite), np.float32(out.lo),
                                 np.float32(out.hi), np.float32(out.min), np.float32(out.max))

    def select_range(self, prop: int, lo: float, hi: float, op: int = 0, filter: int = 0, world: bool = False,  # noqa: A002
                     bins: int = 0, bin_lo: int = 0, bin_hi: int = 0) -> tuple[int, int]:
        """``gsx_model_select_range``: the Gaussians that pass ``filter``, have a finite value and ``lo <= value <= hi`` — and, with
        ``bins`` > 0, whose bin of the histogram over ``(lo, hi, bins)`` lies in ``[bin_lo, bin_hi]`` — are the hit set; ``op``
        (``_lib.GSX_SELECTION_*``) makes it the selection, adds it or removes it, on the device.  Returns ``(hit, selected)``: the
        hit count and the selected count afterwards.  The next frame highlights it; ``extract(dst, SELECTED)`` splits it off."""
        desc = _lib.SelectDesc(int(prop), _lib.GSX_PROP_WORLD if world else 0, int(filter), int(op), float(lo), float(hi), int(bins),
                               int(bin_lo), int(bin_hi), 0)
        hit, selected = C.c_uint64(), C.c_uint64()
        _lib.check(self._v._L.gsx_model_select_range(self._v._h, self._key.encode(), C.byref(desc), C.byref(hit), C.byref(selected)))
        return int(hit.value), int(selected.value)

    def neighbors(self, radius: float, max_count: int = _lib.GSX_NEIGHBOR_MAX_COUNT, filter: int = 0,  # noqa: A002
                  grid_bits: int = 0) -> ModelNeighbors:
        """``gsx_model_neighbors``: for every Gaussian, how many others lie within ``radius`` of it in model space (stored positions,
        ``d2 <= r2`` in float32), saturated at ``max_count`` (1..4095), among the Gaussians that pass ``filter``
        (``_lib.GSX_BOUNDS_*``) and have a finite position; computed on the device with a hashed grid.  ``hist.sum() == count``.
        ``grid_bits`` forces the table size and changes no result."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        desc = _lib.NeighborDesc(int(filter), 0, float(radius), int(max_count), int(grid_bits), 0)
        counts = np.zeros(n, np.uint32)
        hist = np.zeros(min(max(int(max_count), 0), _lib.GSX_NEIGHBOR_MAX_COUNT) + 1, np.uint64)
        out = _lib.NeighborStats()
        _lib.check(self._v._L.gsx_model_neighbors(self._v._h, self._key.encode(), C.byref(desc), counts.ctypes.data, hist.ctypes.data,
                                                  C.byref(out)))
        return ModelNeighbors(counts, hist, int(out.count), int(out.n_nonfinite), int(out.grid_bits))

    def select_neighbors(self, radius: float, count_lo: int, count_hi: int, max_count: int | None = None, op: int = 0,
                         filter: int = 0, grid_bits: int = 0) -> tuple[int, int]:  # noqa: A002
        """``gsx_model_select_neighbors``: the participants whose neighbour count, saturated at ``max_count`` (default: ``count_hi``
        + 1, the cheapest cap that still tells the range apart), lies in ``[count_lo, count_hi]`` are the hit set; ``op``
        (``_lib.GSX_SELECTION_*``) makes it the selection, adds it or removes it, on the device.  Floaters with fewer than ``k``
        neighbours: ``select_neighbors(r, 0, k - 1)``, then ``extract(dst, SELECTED, invert=True)``.  Returns ``(hit, selected)``."""
        cap = min(int(count_hi) + 1, _lib.GSX_NEIGHBOR_MAX_COUNT) if max_count is None else int(max_count)
        desc = _lib.NeighborSelectDesc(int(filter), 0, int(op), cap, float(radius), int(count_lo), int(count_hi), int(grid_bits))
        hit, selected = C.c_uint64(), C.c_uint64()
        _lib.check(self._v._L.gsx_model_select_neighbors(self._v._h, self._key.encode(), C.byref(desc), C.byref(hit), C.byref(selected)))
        return int(hit.value), int(selected.value)

    def clusters(self, radius: float, filter: int = 0, grid_bits: int = 0) -> ModelClusters:  # noqa: A002
        """``gsx_model_clusters``: the connected pieces of the model under "within ``radius`` of one another" (stored positions,
        ``d2 <= r2`` in float32, model space), among the Gaussians that pass ``filter`` (``_lib.GSX_BOUNDS_*``) and have a finite
        position; computed on the device by a union-find over a hashed grid.  ``grid_bits`` forces the table size and changes no
        result."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        desc = _lib.ClusterDesc(int(filter), 0, float(radius), int(grid_bits))
        labels = np.full(n, _lib.GSX_CLUSTER_NONE, np.uint32)
        sizes = np.zeros(n, np.uint32)
        out = _lib.ClusterStats()
        _lib.check(self._v._L.gsx_model_clusters(self._v._h, self._key.encode(), C.byref(desc), labels.ctypes.data, sizes.ctypes.data,
                                                 C.byref(out)))
        return ModelClusters(labels, sizes, int(out.count), int(out.n_nonfinite), int(out.n_clusters), int(out.largest_size),
                             int(out.largest_label), int(out.grid_bits))

    def select_clusters(self, radius: float, mode: int, size_lo: int = 0, size_hi: int = 0, op: int = 0, filter: int = 0,  # noqa: A002
                        grid_bits: int = 0) -> tuple[int, int]:
        """``gsx_model_select_clusters``: the hit set is, by ``mode`` (``_lib.GSX_CLUSTER_*``), the clusters whose size lies in
        ``[size_lo, size_hi]`` (debris below ``k``: ``(1, k - 1)``), the largest cluster, or the clusters that hold a Gaussian
        selected before the call; ``op`` (``_lib.GSX_SELECTION_*``) makes it the selection, adds it or removes it, on the device.
        Keep the object: ``select_clusters(r, GSX_CLUSTER_LARGEST)``, then ``extract(dst, SELECTED)``.  Returns ``(hit, selected)``."""
        desc = _lib.ClusterSelectDesc(int(filter), 0, int(op), int(mode), float(radius), int(size_lo), int(size_hi), int(grid_bits))
        hit, selected = C.c_uint64(), C.c_uint64()
        _lib.check(self._v._L.gsx_model_select_clusters(self._v._h, self._key.encode(), C.byref(desc), C.byref(hit), C.byref(selected)))
        return int(hit.value), int(selected.value)

    def knn(self, k: int = 3, score: int = _lib.GSX_KNN_SCORE_MEAN, filter: int = 0, radius_hint: float = 0.0,  # noqa: A002
            grid_bits: int = 0, max_rounds: int = 0, rows: bool = False) -> ModelKnn:
        """``gsx_model_knn``: for every Gaussian the ``k`` (1..16) smallest squared distances to the others (stored positions, float32,
        model space; ``rows=True`` downloads them), a score from them (``_lib.GSX_KNN_SCORE_*``) and the score's statistics, among
        the Gaussians that pass ``filter`` (``_lib.GSX_BOUNDS_*``) and have a finite position; computed on the device, bit for bit
        the brute-force answer.  ``knn(k, GSX_KNN_SCORE_KTH).mean`` is a radius for ``neighbors`` and ``clusters``.  ``radius_hint``,
        ``grid_bits`` and ``max_rounds`` steer the search and change no result."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        desc = _lib.KnnDesc(int(filter), 0, int(k), int(score), float(radius_hint), int(grid_bits), int(max_rounds), 0)
        d2 = np.full((n, min(max(int(k), 1), _lib.GSX_KNN_MAX_K)), np.inf, np.float32) if rows else None
        values = np.full(n, np.inf, np.float32)
        out = _lib.KnnStats()
        _lib.check(self._v._L.gsx_model_knn(self._v._h, self._key.encode(), C.byref(desc), d2.ctypes.data if rows else None,
                                            values.ctypes.data, C.byref(out)))
        return _knn_stats(out, d2, values)

    def select_knn(self, k: int = 3, score: int = _lib.GSX_KNN_SCORE_MEAN, lo: float = 0.0, hi: float = 0.0,
                   std_ratio: float | None = None, op: int = 0, filter: int = 0, radius_hint: float = 0.0,  # noqa: A002
                   grid_bits: int = 0, max_rounds: int = 0) -> tuple[int, int, ModelKnn]:
        """``gsx_model_select_knn``: the participants whose score lies in ``[lo, hi]`` (``hi`` may be ``inf``) or, with ``std_ratio``
        given, the statistical outliers (score above mean + ``std_ratio`` * std over the model, as in PCL and Open3D) are the hit
        set; ``op`` (``_lib.GSX_SELECTION_*``) makes it the selection, adds it or removes it, on the device.  Floaters:
        ``select_knn(k, std_ratio=2.0)``, then ``extract(dst, SELECTED, invert=True)``.  Returns ``(hit, selected, stats)``; the
        stats carry the threshold and no arrays."""
        outliers = std_ratio is not None
        desc = _lib.KnnSelectDesc(int(filter), 0, int(op), _lib.GSX_KNN_SELECT_OUTLIERS if outliers else _lib.GSX_KNN_SELECT_RANGE, int(k),
                                  int(score), float(radius_hint), int(grid_bits), int(max_rounds), float(lo), float(hi),
                                  float(std_ratio) if outliers else 0.0)
        hit, selected, out = C.c_uint64(), C.c_uint64(), _lib.KnnStats()
        _lib.check(self._v._L.gsx_model_select_knn(self._v._h, self._key.encode(), C.byref(desc), C.byref(hit), C.byref(selected),
                                                   C.byref(out)))
        return int(hit.value), int(selected.value), _knn_stats(out, None, None)

    def normals(self, k: int = 8, toward=None, filter: int = 0, radius_hint: float = 0.0, grid_bits: int = 0,  # noqa: A002
                max_rounds: int = 0, indices: bool = False) -> ModelNormals:
        """``gsx_model_normals``: a plane fitted in double to every Gaussian and its ``k`` (3..16) nearest (stored positions, model
        space), among the Gaussians that pass ``filter`` and have a finite position: the plane's unit normal, the surface variation
        and, with ``indices=True``, who the k nearest are, on the device.  The normal's first non-zero component is positive, or,
        with ``toward`` (a model-space point), the normal looks at that point.  ``radius_hint``, ``grid_bits`` and ``max_rounds``
        steer the search and change no result."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        desc = _lib.NormalsDesc(int(filter), 0, int(k), _lib.GSX_NORMALS_ORIENT_CANONICAL if toward is None else _lib.GSX_NORMALS_ORIENT_TOWARD,
                                float(radius_hint), int(grid_bits), int(max_rounds), 0,
                                (C.c_float * 3)(*([0.0] * 3 if toward is None else [float(x) for x in toward])), 0)
        normal = np.zeros((n, 3), np.float32)
        variation = np.full(n, np.inf, np.float32)
        index = np.full((n, min(max(int(k), 1), _lib.GSX_NORMALS_MAX_K)), _lib.GSX_NORMALS_NONE, np.uint32) if indices else None
        out = _lib.NormalsStats()
        _lib.check(self._v._L.gsx_model_normals(self._v._h, self._key.encode(), C.byref(desc), normal.ctypes.data, variation.ctypes.data,
                                                index.ctypes.data if indices else None, C.byref(out)))
        return _normals_stats(out, normal, variation, index)

    def select_normals(self, k: int = 8, lo: float = 0.0, hi: float = 0.0, direction=None, absolute: bool = False, toward=None,
                       op: int = 0, filter: int = 0, radius_hint: float = 0.0, grid_bits: int = 0,  # noqa: A002
                       max_rounds: int = 0) -> tuple[int, int, ModelNormals]:
        """``gsx_model_select_normals``: the fitted Gaussians whose variation lies in ``[lo, hi]`` or, with ``direction`` given, whose
        normal's cosine with it does (its absolute value with ``absolute``) are the hit set; ``op`` (``_lib.GSX_SELECTION_*``) makes
        it the selection, adds it or removes it, on the device.  The floor: ``select_normals(8, 0.95, 1.0, direction=up,
        absolute=True)``, then ``bounds(SELECTED)``.  Returns ``(hit, selected, stats)``; the stats carry no arrays."""
        facing = direction is not None
        vec = lambda x: (C.c_float * 3)(*([0.0] * 3 if x is None else [float(c) for c in x]))  # noqa: E731
        desc = _lib.NormalsSelectDesc(int(filter), _lib.GSX_NORMALS_ABS if absolute else 0, int(op),
                                      _lib.GSX_NORMALS_SELECT_FACING if facing else _lib.GSX_NORMALS_SELECT_VARIATION, int(k),
                                      _lib.GSX_NORMALS_ORIENT_CANONICAL if toward is None else _lib.GSX_NORMALS_ORIENT_TOWARD,
                                      float(radius_hint), int(grid_bits), int(max_rounds), float(lo), float(hi), 0, vec(direction), vec(toward),
                                      (C.c_uint32 * 2)(0, 0))
        hit, selected, out = C.c_uint64(), C.c_uint64(), _lib.NormalsStats()
        _lib.check(self._v._L.gsx_model_select_normals(self._v._h, self._key.encode(), C.byref(desc), C.byref(hit), C.byref(selected),
                                                       C.byref(out)))
        return int(hit.value), int(selected.value), _normals_stats(out, None, None, None)

    def nearest(self, dst_key: str, xform=None, model_transforms: bool = False, src_filter: int = 0, dst_filter: int = 0,
                max_distance: float = 0.0, radius_hint: float = 0.0, grid_bits: int = 0, max_rounds: int = 0,
                rows: bool = True) -> ModelNearest:
        """``gsx_model_nearest``: for every Gaussian of this model the nearest Gaussian of ``viewer.models[dst_key]`` (index and
        squared distance; ``rows=False`` returns the statistics alone), on the device, bit for bit the brute-force answer with ties
        going to the smaller index.  ``xform`` (3x4, default the identity) maps this model's space into the target's;
        ``model_transforms=True`` takes it from the two models' transforms instead.  The filters are ``_lib.GSX_BOUNDS_*`` bits;
        ``max_distance`` (0: unlimited) bounds both the answer and the cost.  ``.mean`` is the one-sided chamfer distance, ``.d_max``
        the one-sided Hausdorff distance."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        desc = _nearest_desc(xform, model_transforms, src_filter, dst_filter, max_distance, radius_hint, grid_bits, max_rounds)
        index = np.full(n, _lib.GSX_NEAREST_NONE, np.uint32) if rows else None
        d2 = np.full(n, np.inf, np.float32) if rows else None
        out = _lib.NearestStats()
        _lib.check(self._v._L.gsx_model_nearest(self._v._h, self._key.encode(), dst_key.encode(), C.byref(desc), index.ctypes.data if rows else None,
                                                d2.ctypes.data if rows else None, C.byref(out)))
        return _nearest_stats(out, index, d2)

    def select_nearest(self, dst_key: str, lo: float = 0.0, hi: float = 0.0, transfer: bool = False, op: int = 0, xform=None,
                       model_transforms: bool = False, src_filter: int = 0, dst_filter: int = 0, max_distance: float = 0.0,
                       radius_hint: float = 0.0, grid_bits: int = 0, max_rounds: int = 0) -> tuple[int, int, ModelNearest]:
        """``gsx_model_select_nearest``: writes THIS model's selection.  The hit set is the Gaussians whose distance to the target
        model lies in ``[lo, hi]`` (``hi`` may be ``inf``: also those without a target in reach) or, with ``transfer=True``, those
        whose nearest target is selected in ``dst_key``: a selection carried across models.  Overlap before a merge:
        ``b.select_nearest("a", 0.0, d)``, then ``extract(..., SELECTED, invert=True)``.  Returns ``(hit, selected, stats)``."""
        desc = _lib.NearestSelectDesc(_nearest_desc(xform, model_transforms, src_filter, dst_filter, max_distance, radius_hint, grid_bits, max_rounds),
                                      int(op), _lib.GSX_NEAREST_SELECT_TRANSFER if transfer else _lib.GSX_NEAREST_SELECT_RANGE, float(lo), float(hi))
        hit, selected, out = C.c_uint64(), C.c_uint64(), _lib.NearestStats()
        _lib.check(self._v._L.gsx_model_select_nearest(self._v._h, self._key.encode(), dst_key.encode(), C.byref(desc), C.byref(hit),
                                                       C.byref(selected), C.byref(out)))
        return int(hit.value), int(selected.value), _nearest_stats(out, None, None)

    def align_step(self, dst_key: str, xform=None, model_transforms: bool = False, with_scale: bool = False, src_filter: int = 0,
                   dst_filter: int = 0, max_distance: float = 0.0, radius_hint: float = 0.0, grid_bits: int = 0,
                   max_rounds: int = 0) -> ModelAlignStep:
        """``gsx_model_align_step``: one least-squares step of point-to-point registration of this model onto ``dst_key``: the
        nearest search (``max_distance`` rejects correspondences), the pairs' sums on the device, Horn's closed form on the host."""
        desc = _lib.AlignDesc(_nearest_desc(xform, model_transforms, src_filter, dst_filter, max_distance, radius_hint, grid_bits, max_rounds),
                              _lib.GSX_ALIGN_SCALE if with_scale else 0, 0)
        out = _lib.AlignStep()
        _lib.check(self._v._L.gsx_model_align_step(self._v._h, self._key.encode(), dst_key.encode(), C.byref(desc), C.byref(out)))
        vec = lambda a: np.array(a[:], np.float32)  # noqa: E731
        return ModelAlignStep(np.array(out.pos[:], np.float64), np.array(out.quat[:], np.float64), float(out.scale), vec(out.xform_next).reshape(3, 4), int(out.n_pairs),
                              float(out.rms_before), bool(out.degenerate), _nearest_stats(out.nearest, None, None))

    def keep_normals(self, k: int = 8, toward=None, filter: int = 0, radius_hint: float = 0.0, grid_bits: int = 0,  # noqa: A002
                     max_rounds: int = 0) -> ModelNormals:
        """``gsx_model_normals_keep``: ``normals`` with the same arguments, whose normals and variations stay on the device with the
        model (16 bytes a Gaussian) for ``align_plane_step``; a second keep replaces the first.  An upload, an import, a transform
        and a pod kind change drop the plane; a selection, a mask, an edit and a frame do not.  Returns the statistics, no arrays."""
        desc = _lib.NormalsDesc(int(filter), 0, int(k), _lib.GSX_NORMALS_ORIENT_CANONICAL if toward is None else _lib.GSX_NORMALS_ORIENT_TOWARD,
                                float(radius_hint), int(grid_bits), int(max_rounds), 0,
                                (C.c_float * 3)(*([0.0] * 3 if toward is None else [float(x) for x in toward])), 0)
        out = _lib.NormalsStats()
        _lib.check(self._v._L.gsx_model_normals_keep(self._v._h, self._key.encode(), C.byref(desc), C.byref(out)))
        return _normals_stats(out, None, None, None)

    def kept_normals(self, rows: bool = True) -> ModelNormalsKept:
        """``gsx_model_normals_kept``: whether a plane is resident, what it was made with and (``rows``) its contents."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        normal = np.zeros((n, 3), np.float32) if rows else None
        variation = np.full(n, np.inf, np.float32) if rows else None
        out = _lib.NormalsKept()
        _lib.check(self._v._L.gsx_model_normals_kept(self._v._h, self._key.encode(), C.byref(out), normal.ctypes.data if rows else None,
                                                     variation.ctypes.data if rows else None))
        present = bool(out.present)
        return ModelNormalsKept(present, int(out.k), int(out.orient), int(out.filter), np.array(out.toward[:], np.float32), int(out.count),
                                int(out.n_fitted), normal if present else None, variation if present else None)

    def reset_normals(self) -> None:
        """``gsx_model_normals_reset``: frees the kept plane."""
        _lib.check(self._v._L.gsx_model_normals_reset(self._v._h, self._key.encode()))

    def align_plane_step(self, dst_key: str, xform=None, model_transforms: bool = False, max_variation: float = 0.0, src_filter: int = 0,
                         dst_filter: int = 0, max_distance: float = 0.0, radius_hint: float = 0.0, grid_bits: int = 0,
                         max_rounds: int = 0) -> ModelAlignPlaneStep:
        """``gsx_model_align_plane_step``: one Gauss-Newton step of point-to-plane registration of this model onto ``dst_key``, which
        needs ``keep_normals`` first: ``align_step``'s search, the 6x6 normal equations on the device, a spectral solve on the host
        that moves only along what the pairs determine (``rank``).  ``max_variation`` (0: no limit) leaves out targets whose
        neighbourhood is far from a plane."""
        desc = _lib.AlignPlaneDesc(_nearest_desc(xform, model_transforms, src_filter, dst_filter, max_distance, radius_hint, grid_bits, max_rounds),
                                   0, float(max_variation), (C.c_uint32 * 2)(0, 0))
        out = _lib.AlignPlaneStep()
        _lib.check(self._v._L.gsx_model_align_plane_step(self._v._h, self._key.encode(), dst_key.encode(), C.byref(desc), C.byref(out)))
        vec = lambda a: np.array(a[:], np.float64)  # noqa: E731
        return ModelAlignPlaneStep(vec(out.pos), vec(out.quat), vec(out.normal_matrix), vec(out.rhs), vec(out.eigenvalues), vec(out.centre),
                                   float(out.rms_before), float(out.rms_plane_before), int(out.n_pairs), int(out.n_unfitted),
                                   np.array(out.xform_next[:], np.float32).reshape(3, 4), int(out.rank), bool(out.degenerate),
                                   _nearest_stats(out.nearest, None, None))

    def fit_plane(self, tolerance: float, n_candidates: int = 256, sample: int = _lib.GSX_PLANE_SAMPLE_TRIPLES, seed: int = 0,
                  min_cos: float = 0.0, refine_iters: int = 2, toward=None, filter: int = 0, invert: bool = False,  # noqa: A002
                  candidates=None, rows: bool = True) -> ModelPlaneFit:
        """``gsx_model_fit_plane``: the model's dominant plane by consensus, on the device.  ``n_candidates`` planes (1 .. 1024) are
        made from three sampled participants (``GSX_PLANE_SAMPLE_TRIPLES``), from one sampled participant and its kept normal
        (``_NORMALS``: ``keep_normals`` first) or taken from ``candidates`` (``(H, 4)`` float32, used as given; sets ``_CALLER``); every
        participant is tested against every plane (inlier: ``|r| <= tolerance`` and, with ``min_cos > 0``, a kept normal within that
        cosine of the plane's); the plane with the most inliers wins and is refined by up to ``refine_iters`` least-squares rounds.
        Level a capture: ``q, t = plane_level(fit.plane, up)``, then ``update_model_transform``.  Remove the floor:
        ``select_plane(fit.plane, -inf, tolerance)``, then ``extract`` with ``SELECTED`` inverted.  Peel the next plane:
        ``select_plane(fit.plane, -tolerance, tolerance, op=GSX_SELECTION_ADD)``, then ``fit_plane(..., filter=SELECTED,
        invert=True)``."""
        if candidates is not None:
            cand = np.ascontiguousarray(candidates, np.float32).reshape(-1, 4)
            sample, n_candidates = _lib.GSX_PLANE_SAMPLE_CALLER, len(cand)
        H = int(n_candidates)
        desc = _lib.PlaneFitDesc(int(filter), _lib.GSX_EXTRACT_INVERT if invert else 0, int(sample), H, int(seed) & 0xFFFFFFFFFFFFFFFF, float(tolerance),
                                 float(min_cos), int(refine_iters), _lib.GSX_NORMALS_ORIENT_CANONICAL if toward is None else _lib.GSX_NORMALS_ORIENT_TOWARD,
                                 (C.c_float * 3)(*([0.0] * 3 if toward is None else [float(x) for x in toward])), (C.c_uint32 * 3)(0, 0, 0))
        want = rows and 1 <= H <= _lib.GSX_PLANE_MAX_CANDIDATES
        planes = np.zeros((H, 4), np.float32) if want else None
        counts = np.zeros(H, np.uint32) if want else None
        out = _lib.PlaneFit()
        _lib.check(self._v._L.gsx_model_fit_plane(self._v._h, self._key.encode(), C.byref(desc), cand.ctypes.data if candidates is not None else None,
                                                  planes.ctypes.data if want else None, counts.ctypes.data if want else None, C.byref(out)))
        pl = lambda q: np.array([q.normal[0], q.normal[1], q.normal[2], q.offset], np.float32)  # noqa: E731
        return ModelPlaneFit(pl(out.plane), pl(out.candidate), None if out.winner == _lib.GSX_PLANE_NONE else int(out.winner), int(out.n_valid),
                             int(out.count), int(out.n_nonfinite), int(out.candidate_inliers), int(out.n_inliers), np.array(out.centroid[:], np.float32),
                             np.array(out.eigenvalues[:], np.float64), float(out.rms), np.array(out.sums[:], np.float64), int(out.refine_done),
                             bool(out.degenerate), planes, counts)

    def select_plane(self, plane, lo: float, hi: float, min_cos: float = 0.0, op: int = 0, filter: int = 0) -> tuple[int, int]:  # noqa: A002
        """``gsx_model_select_plane``: the participants whose signed residual ``r = n . p - offset`` against ``plane`` (``nx, ny, nz,
        offset``) lies in ``[lo, hi]`` (a bound may be infinite: everything above the floor is ``lo=tolerance, hi=inf``) and, with
        ``min_cos > 0``, whose kept normal is within that cosine of the plane's, are the hit set; ``op`` (``_lib.GSX_SELECTION_*``)
        makes it the selection, adds it or removes it, on the device.  Returns ``(hit, selected)``."""
        pl = np.ascontiguousarray(plane, np.float32).reshape(4)
        desc = _lib.PlaneSelectDesc(_lib.Plane((C.c_float * 3)(*[float(x) for x in pl[:3]]), float(pl[3])), float(lo), float(hi), float(min_cos),
                                    int(filter), int(op), (C.c_uint32 * 3)(0, 0, 0))
        hit, selected = C.c_uint64(), C.c_uint64()
        _lib.check(self._v._L.gsx_model_select_plane(self._v._h, self._key.encode(), C.byref(desc), C.byref(hit), C.byref(selected)))
        return int(hit.value), int(selected.value)

    def align(self, dst_key: str, max_iters: int = 30, tol: float = 1e-6, xform=None, model_transforms: bool = False, method: str = "point",
              **step_args):
        """Iterative closest point: ``align_step`` until ``rms_before`` changes by less than ``tol`` relatively or does not fall any
        more (with exact correspondences it ends at the float32 rounding of the positions, where it only flickers: a rise is the
        end, whatever ``tol``), a step is degenerate or ``max_iters`` steps ran.  Returns ``(xform_final, D, steps)``: the final float32 3x4 matrix, the composed similarity
        ``D`` (float64 3x4) with ``xform_final = D o xform_initial`` up to the steps' roundings, and the list of steps.  With an
        identity start ``D`` is what ``apply_transform`` bakes or ``update_model_transform`` shows.  ``method="plane"`` runs the same
        loop over ``align_plane_step`` (``dst_key`` needs ``keep_normals`` first) and stops on ``rms_plane_before``."""
        if method not in ("point", "plane"):
            raise ValueError(f"align: method {method!r} is not 'point' or 'plane'")
        plane = method == "plane"
        steps, D, last = [], np.eye(3, 4), None
        for _ in range(int(max_iters)):
            st = (self.align_plane_step if plane else self.align_step)(dst_key, xform=xform, model_transforms=model_transforms and not steps, **step_args)
            steps.append(st)
            if xform is None:
                xform = st.nearest.xform
            rms = st.rms_plane_before if plane else st.rms_before
            if st.degenerate or (last is not None and (rms >= last or last - rms <= tol * last)):
                break
            last = rms
            q = st.quat.astype(np.float64)
            x, y, z, w = q / np.linalg.norm(q)
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            D = _compose34(np.concatenate([float(st.scale) * R, st.pos.astype(np.float64)[:, None]], axis=1), D)
            xform = st.xform_next
        return np.asarray(xform, np.float32).reshape(3, 4), D, steps

    def _decimate(self, dst_key, cell, filter, invert, grid_bits, want_map):  # noqa: A002
        desc = _lib.DecimateDesc(int(filter), _lib.GSX_EXTRACT_INVERT if invert else 0, float(cell), int(grid_bits))
        out = _lib.DecimateStats()
        out_map = np.full(self.gaussian_buffers.gaussians_buffer.len(), _lib.GSX_DECIMATE_NO_CELL, np.uint32) if want_map else None
        _lib.check(self._v._L.gsx_model_decimate(self._v._h, self._key.encode(), None if dst_key is None else dst_key.encode(), C.byref(desc),
                                                 out_map.ctypes.data if want_map else None, C.byref(out)))
        if dst_key is not None and out.cells:
            self._v.models[dst_key] = MultiModelViewerModel(self._v, dst_key)
        return ModelDecimate(int(out.count), int(out.n_nonfinite), int(out.cells), int(out.singletons), int(out.largest_cell), int(out.grid_bits),
                             out_map)

    def decimate(self, dst_key: str, cell: float, filter: int = 0, invert: bool = False, grid_bits: int = 0,  # noqa: A002
                 want_map: bool = False) -> ModelDecimate:
        """``gsx_model_decimate``: the Gaussians that pass ``filter`` (``extract``'s kept set), have a finite position and share a
        cell of a uniform grid of edge ``cell`` (model space) become ONE moment-matched Gaussian of the new model ``dst_key``, on the
        device: mean and covariance of the mixture weighted by opacity times volume, opacity conserving that mass, colour and SH the
        weighted means; a one-member cell is copied as stored bits.  The new model has this one's pod kind and transform and no mask,
        selection or edits; it is ``viewer.models[dst_key]``.  ``cells == 0`` creates no model.  ``want_map`` downloads where every
        Gaussian went.  ``decimate_edge`` finds a ``cell`` for a target count."""
        return self._decimate(dst_key, cell, filter, invert, grid_bits, want_map)

    def decimate_count(self, cell: float, filter: int = 0, invert: bool = False, grid_bits: int = 0,  # noqa: A002
                       want_map: bool = False) -> ModelDecimate:
        """``gsx_model_decimate`` without a destination: the statistics (and the map) ``decimate`` would return; nothing is created."""
        return self._decimate(None, cell, filter, invert, grid_bits, want_map)

    def decimate_edge(self, target: int, filter: int = 0, invert: bool = False) -> tuple[float, int]:  # noqa: A002
        """``gsx_model_decimate_edge``: the smallest probed cell edge that leaves at most ``target`` cells, by 20 count-only bisection
        steps on the device.  Returns ``(cell, cells)``: ``cell`` as a numpy float32, ready for ``decimate``."""
        cell, cells = C.c_float(), C.c_uint64()
        _lib.check(self._v._L.gsx_model_decimate_edge(self._v._h, self._key.encode(), int(filter), _lib.GSX_EXTRACT_INVERT if invert else 0,
                                                      int(target), C.byref(cell), C.byref(cells)))
        return np.float32(cell.value), int(cells.value)

    def visibility(self, accumulate: bool = False, rows: bool = True, transmittance: bool = False) -> ModelVisibility:
        """``gsx_model_visibility``: draws this model ALONE with the viewer's current camera, viewport, transforms and spec
        parameters (what ``render_frame([key])`` would draw) and keeps, per Gaussian and on the device, what the compositor throws
        away: the peak blending weight, the summed weight and the pixel count.  ``accumulate`` folds the view into the planes an
        earlier call left (maximum, sums) instead of replacing them.  ``rows=False`` returns the statistics alone.  The model must go
        through ``preprocess`` + ``sort`` again before ``render``; ``render_frame`` needs nothing."""
        n = self.gaussian_buffers.gaussians_buffer.len()
        w, h = self._v.size
        desc = _lib.VisibilityDesc(_lib.GSX_VIS_ACCUMULATE if accumulate else 0)
        peak = np.zeros(n, np.float32) if rows else None
        weight = np.zeros(n, np.float64) if rows else None
        pixels = np.zeros(n, np.uint32) if rows else None
        trans = np.empty((h, w), np.float32) if transmittance else None
        out = _lib.VisibilityStats()
        _lib.check(self._v._L.gsx_model_visibility(self._v._h, self._key.encode(), C.byref(desc), peak.ctypes.data if rows else None,
                                                   weight.ctypes.data if rows else None, pixels.ctypes.data if rows else None,
                                                   trans.ctypes.data if transmittance else None, C.byref(out)))
        return ModelVisibility(peak, weight, pixels, trans, int(out.n_visible), int(out.n_seen), int(out.n_pairs), int(out.weight_fixed),
                               np.float32(out.peak_max), int(out.views))

    def select_visibility(self, measure: int = 0, lo: float = 0.0, hi: float = float("inf"), op: int = 0, filter: int = 0) -> tuple[int, int]:  # noqa: A002
        """``gsx_model_select_visibility``: selects the Gaussians that pass ``filter`` (``_lib.GSX_BOUNDS_*`` bits) and whose resident
        measure (``_lib.GSX_VIS_PEAK`` / ``_WEIGHT`` / ``_PIXELS``) lies in ``[lo, hi]``.  "Never seen" is ``select_visibility(GSX_VIS_PEAK,
        0, 0)``; a contribution prune is that, then ``extract(dst, SELECTED, invert=True)``.  Returns ``(hit, selected)``."""
        desc = _lib.VisibilitySelectDesc(int(measure), int(filter), int(op), 0, float(lo), float(hi))
        hit, selected = C.c_uint64(), C.c_uint64()
        _lib.check(self._v._L.gsx_model_select_visibility(self._v._h, self._key.encode(), C.byref(desc), C.byref(hit), C.byref(selected)))
        return int(hit.value), int(selected.value)

    def visibility_reset(self) -> None:
        """``gsx_model_visibility_reset``: frees the resident planes."""
        _lib.check(self._v._L.gsx_model_visibility_reset(self._v._h, self._key.encode()))

    def visibility_orbit(self, cameras, size=None, rows: bool = True) -> ModelVisibility:
        """Resets the planes, then folds one view per camera of ``cameras`` (``update_camera`` with ``size``, default the viewer's
        current viewport): the planes then hold every Gaussian's best and summed contribution over the orbit.  Returns the last
        call's result (the planes after all views).  The viewer keeps the last camera."""
        size = self._v.size if size is None else size
        self.visibility_reset()
        cameras = list(cameras)
        out = None
        for k, cam in enumerate(cameras):
            self._v.update_camera(cam, size)
            out = self.visibility(accumulate=True, rows=rows and k + 1 == len(cameras))
        return out

    def _export_desc(self, filter, invert, bake_edits, fmt, staging_bytes):  # noqa: A002
        return _lib.ExportDesc(int(filter), (_lib.GSX_EXTRACT_INVERT if invert else 0) | (_lib.GSX_EXPORT_BAKE_EDITS if bake_edits else 0),
                               fmt, 0, int(staging_bytes))

    def export(self, filter: int = 0, invert: bool = False, bake_edits: bool = False, staging_bytes: int = 0):  # noqa: A002
        """``gsx_model_export``: the Gaussians of this model that pass ``filter`` (``_lib.GSX_BOUNDS_*`` bits, ``extract``'s meaning;
        ``invert``: exactly those that do not) as ``ply.Gaussians``, built on the device from the resident planes: positions, colours
        and SH as stored (dequantised exactly), rotation and scale solved from the stored covariance.  Model space: the model
        transform is not applied (``viewer.merge`` bakes it).  ``bake_edits``: enabled edit records are baked into the colours as
        ``write_ply`` does.  The way out for a model that only the device holds, and from one pod kind to another."""
        from .ply import Gaussians
        from .scene import GAUSSIAN_DTYPE

        desc = self._export_desc(filter, invert, bake_edits, _lib.GSX_EXPORT_GAUSSIANS, staging_bytes)
        count = C.c_uint64()
        _lib.check(self._v._L.gsx_model_export(self._v._h, self._key.encode(), C.byref(desc), None, 0, C.byref(count)))
        out = np.empty(count.value, GAUSSIAN_DTYPE)  # every byte is written by the library
        if count.value:
            _lib.check(self._v._L.gsx_model_export(self._v._h, self._key.encode(), C.byref(desc), out.ctypes.data, out.nbytes, C.byref(count)))
        return Gaussians(out)

    def export_ply(self, filter: int = 0, invert: bool = False, bake_edits: bool = False, staging_bytes: int = 0) -> bytes:  # noqa: A002
        """``gsx_model_export_ply``: the same Gaussians as a binary INRIA PLY file, ``Gaussians.write_ply``'s header and rows.  The
        reference's ``write_ply(edits, mask)`` is ``export_ply(MASKED | SKIP_HIDDEN, bake_edits=True)``; ``Gaussians.read_ply`` loads
        the result back."""
        desc = self._export_desc(filter, invert, bake_edits, _lib.GSX_EXPORT_PLY_VERTICES, staging_bytes)
        size = C.c_uint64()
        _lib.check(self._v._L.gsx_model_export_ply(self._v._h, self._key.encode(), C.byref(desc), None, 0, C.byref(size)))
        out = np.empty(size.value, np.uint8)
        _lib.check(self._v._L.gsx_model_export_ply(self._v._h, self._key.encode(), C.byref(desc), out.ctypes.data, out.size, C.byref(size)))
        return out.tobytes()


class _Preprocessor:
    def __init__(self, v):
        self._v = v

    def preprocess(self, key: str) -> None:
        """``preprocessor.preprocess(encoder, bind_group, gaussian_count)`` (src/tab/scene.rs:856-863)."""
        _lib.check(self._v._L.gsx_preprocess(self._v._h, key.encode()))


class _Postprocessor:
    def __init__(self, v):
        self._v = v

    def postprocess(self, key: str) -> None:
        """``postprocessor.postprocess(encoder, bg0, bg1, gaussian_count, indirect_args)`` (src/tab/scene.rs:601-611)."""
        _lib.check(self._v._L.gsx_postprocess(self._v._h, key.encode()))


class _RadixSorter:
    def __init__(self, v):
        self._v = v

    def sort(self, key: str) -> None:
        """``radix_sorter.sort(encoder, bind_group, indirect_args)`` (src/tab/scene.rs:865-869)."""
        _lib.check(self._v._L.gsx_sort(self._v._h, key.encode()))


class _Renderer:
    def __init__(self, v):
        self._v = v

    def render(self, model_render_keys: Sequence[str]) -> None:
        """The ``render_with_pass`` loop over ``model_render_keys`` far -> near (src/tab/scene.rs:2302-2314)."""
        keys = [k.encode() for k in model_render_keys]
        arr = (C.c_char_p * max(len(keys), 1))(*keys)
        _lib.check(self._v._L.gsx_render(self._v._h, arr, len(keys)))


class CommGroup:
    """``gsx_comm_group``: the in-process transport for `world` viewers of ONE process (one host thread each)."""

    def __init__(self, world: int, timeout_ms: int = 0):
        self._L = _lib.load()
        self._h = C.c_void_p()
        self.world = int(world)
        _lib.check(self._L.gsx_comm_group_create(self.world, int(timeout_ms), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.gsx_comm_group_destroy(self._h)
            self._h = C.c_void_p()


class MultiModelViewer:
    """``gs::MultiModelViewer<G>`` over libgsx.so."""

    def __init__(self, size=(1, 1), device: int = 0, stream: int | None = None, sh: ShKind = ShKind.Single,
                 cov3d: Cov3dKind = Cov3dKind.Single):
        self._L = _lib.load()
        self._h = C.c_void_p()
        desc = _lib.ViewerDesc(_lib.GSX_ABI_VERSION, int(device), stream, int(size[0]), int(size[1]))
        _lib.check(self._L.gsx_viewer_create(C.byref(desc), C.byref(self._h)))
        self.sh, self.cov3d = ShKind(sh), Cov3dKind(cov3d)
        self.models: dict[str, MultiModelViewerModel] = {}
        self.preprocessor = _Preprocessor(self)
        self.radix_sorter = _RadixSorter(self)
        self.renderer = _Renderer(self)
        self.postprocessor = _Postprocessor(self)
        self.size = (int(size[0]), int(size[1]))

    # -- lifetime --
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._L.gsx_viewer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- models --
    def add_model(self, key: str, count: int) -> MultiModelViewerModel:
        """``GaussianBuffers::new_empty(device, count)`` + ``BindGroups::new`` + ``models.insert`` (scene.rs:2111-2139)."""
        _lib.check(self._L.gsx_model_create(self._h, key.encode(), int(count), int(self.sh), int(self.cov3d)))
        self.models[key] = MultiModelViewerModel(self, key)
        return self.models[key]

    def import_ply(self, key: str, data, staging_bytes: int = 0) -> int:
        """``gsx_model_import_ply``: the app's load path ``read_ply_header -> read_ply_gaussians -> Gaussian::from -> update_range``
        (src/app.rs:1053-1096) in one call, the rows decoded on the device: the binary INRIA PLY file ``data`` (bytes-like) becomes the
        new model ``key`` of this viewer's pod kinds.  Returns the count; a file of 0 vertices creates no model."""
        buf = np.frombuffer(data, dtype=np.uint8)
        desc = _lib.ImportDesc(0, 0, int(staging_bytes))
        count = C.c_uint64()
        _lib.check(self._L.gsx_model_import_ply(self._h, key.encode(), buf.ctypes.data if buf.size else None, buf.size, int(self.sh), int(self.cov3d),
                                                C.byref(desc), C.byref(count)))
        if count.value:
            self.models[key] = MultiModelViewerModel(self, key)
        return int(count.value)

    def merge(self, dst_key: str, src_keys, filter: int = 0, invert: bool = False, drop_edits: bool = False):  # noqa: A002
        """``gsx_model_merge``: the Gaussians of the models ``src_keys`` that pass ``filter`` (``_lib.GSX_BOUNDS_*`` bits, applied to
        every source with ``extract``'s meaning) become the one new model ``dst_key`` on the device, source after source in the order
        given, with each source's model transform baked into its Gaussians (positions, covariances and SH coefficients; a source
        under the identity transform travels as stored bits).  ``dst_key`` has the identity transform.  A key may appear twice.
        Returns ``(total, counts)``; a total of 0 creates no model.  The way back from ``extract`` + ``update_model_transform``."""
        keys = [k.encode() for k in src_keys]
        arr = (C.c_char_p * max(len(keys), 1))(*keys)
        desc = _lib.ExtractDesc(int(filter), (_lib.GSX_EXTRACT_INVERT if invert else 0) | (_lib.GSX_EXTRACT_DROP_EDITS if drop_edits else 0))
        counts, total = (C.c_uint64 * max(len(keys), 1))(), C.c_uint64()
        _lib.check(self._L.gsx_model_merge(self._h, arr, len(keys), dst_key.encode(), C.byref(desc), counts, C.byref(total)))
        if total.value:
            self.models[dst_key] = MultiModelViewerModel(self, dst_key)
        return int(total.value), [int(c) for c in counts[: len(keys)]]

    def remove_model(self, key: str) -> None:
        """``viewer.remove_model(&key)`` (src/tab/scene.rs:2176)."""
        _lib.check(self._L.gsx_model_remove(self._h, key.encode()))
        self.models.pop(key, None)

    # -- per-frame uniforms --
    def update_camera(self, camera, size) -> None:
        """``viewer.update_camera(queue, &impl CameraTrait, uvec2 size)`` (src/tab/scene.rs:795)."""
        w, h = int(size[0]), int(size[1])
        self.update_camera_with_matrices(camera.view(), camera.projection(w / h), (w, h))

    def update_camera_with_matrices(self, view, proj, size) -> None:
        v = np.ascontiguousarray(view, np.float32).reshape(16)
        p = np.ascontiguousarray(proj, np.float32).reshape(16)
        _lib.check(self._L.gsx_update_camera(self._h, _f32p(v), _f32p(p), int(size[0]), int(size[1])))
        self.size = (int(size[0]), int(size[1]))

    def update_model_transform(self, key: str, pos, quat, scale) -> None:
        """``viewer.update_model_transform(queue, key, pos, quat, scale)`` (src/tab/scene.rs:796-802)."""
        p = np.ascontiguousarray(pos, np.float32).reshape(3)
        q = np.ascontiguousarray(quat, np.float32).reshape(4)
        s = np.ascontiguousarray(scale, np.float32).reshape(3)
        _lib.check(self._L.gsx_update_model_transform(self._h, key.encode(), _f32p(p), _f32p(q), _f32p(s)))

    def update_gaussian_transform(self, size: float, display_mode: GaussianDisplayMode, sh_deg, no_sh0: bool) -> None:
        """``viewer.update_gaussian_transform(queue, size, display_mode, sh_deg, no_sh0)`` (src/tab/scene.rs:803-809)."""
        deg = sh_deg.degree() if isinstance(sh_deg, GaussianShDegree) else int(sh_deg)
        _lib.check(self._L.gsx_update_gaussian_transform(self._h, float(size), int(display_mode), deg, 1 if no_sh0 else 0))

    # -- selection / edits / queries (spec §7) --
    def update_query(self, pod) -> None:
        """``viewer.update_query(queue, &query_pod)`` (src/tab/scene.rs:785)."""
        raw = pod.raw()
        _lib.check(self._L.gsx_update_query(self._h, C.byref(raw)))

    def update_query_texture(self, texels: np.ndarray) -> None:
        """``viewer.update_query_texture_size`` + ``query_toolset.render(.., &query_texture)`` (scene.rs:740, 791)."""
        t = np.ascontiguousarray(texels, np.uint8)
        _lib.check(self._L.gsx_update_query_texture(self._h, t.ctypes.data, t.shape[1], t.shape[0]))

    def download_query_texture(self) -> np.ndarray:
        """uint8 [H, W]: the query texture as the device holds it (the viewport's size once the toolset has rendered)."""
        w, h = self.size
        out = np.empty((h, w), np.uint8)
        _lib.check(self._L.gsx_download_query_texture(self._h, out.ctypes.data, w, h))
        return out

    def set_toolset_overlay(self, texture_rgba=(0.0, 0.0, 0.0, 0.0), cursor_rgba=(0.0, 0.0, 0.0, 0.0), cursor_thickness: float = 1.0) -> None:
        """``QueryTextureOverlay`` / ``QueryCursor`` (src/tab/scene.rs:2003-2014, 2317-2325): the straight-alpha colours the RGBA8 resolve
        draws the stroke and the cursor with; alpha 0 (the default) draws nothing."""
        t = np.ascontiguousarray(texture_rgba, np.float32).reshape(4)
        c = np.ascontiguousarray(cursor_rgba, np.float32).reshape(4)
        _lib.check(self._L.gsx_toolset_set_overlay(self._h, _f32p(t), _f32p(c), float(cursor_thickness)))

    def update_selection_highlight(self, rgba) -> None:
        """``viewer.update_selection_highlight(queue, vec4)`` / ``_with_pod`` (src/tab/scene.rs:816-829)."""
        c = np.ascontiguousarray(rgba, np.float32).reshape(4)
        _lib.check(self._L.gsx_update_selection_highlight(self._h, _f32p(c)))

    def update_selection_edit_with_pod(self, pod) -> None:
        """``viewer.update_selection_edit_with_pod(queue, &gs::GaussianEditPod)`` (src/tab/scene.rs:815, 821, 848)."""
        raw = pod.raw()
        _lib.check(self._L.gsx_update_selection_edit(self._h, C.byref(raw)))

    def show_unedited(self, key: str, on: bool) -> None:
        """Preprocess with the unedited model's bind group (src/tab/scene.rs:856-863)."""
        _lib.check(self._L.gsx_model_show_unedited(self._h, key.encode(), 1 if on else 0))

    def download_query_hits(self, key: str) -> np.ndarray:
        """``gs::query::download(&device, &queue, &count_buffer, &results_buffer)`` (src/tab/scene.rs:651-657)."""
        from .query import HIT_DTYPE

        n = C.c_uint64()
        out = np.zeros(65536, HIT_DTYPE)
        _lib.check(self._L.gsx_query_download_hits(self._h, key.encode(), out.ctypes.data, out.size, C.byref(n)))
        return out[: int(n.value)].copy()

    def set_spec_params(self, **kw) -> SpecParams:
        sp = SpecParams()
        self._L.gsx_spec_params_default(C.byref(sp))
        for k, val in kw.items():
            if not hasattr(sp, k):
                raise KeyError(k)
            setattr(sp, k, float(val))
        _lib.check(self._L.gsx_viewer_set_spec_params(self._h, C.byref(sp)))
        return sp

    # -- depth test against the caller's depth buffer (gs::MultiModelViewer::new_with's depth_stencil, scene.rs:1969-1980) --
    def set_depth_test(self, compare) -> None:
        """``DepthStencilState { Depth32Float, depth_write_enabled: false, compare }``: ``DepthCompare.Less`` hides a splat behind the
        depth buffer at that pixel, ``DepthCompare.Always`` (default) turns the test off.  With ``frames_in_flight > 1`` a depth-tested
        frame is dealt to a lane like any other and the lane takes its own snapshot: the buffer is read as if on the viewer's stream at
        the ``render_frame`` that uses it — what is set or enqueued there afterwards waits for that read (no host wait), not for the
        frame (``gsx.h``, the depth block)."""
        _lib.check(self._L.gsx_viewer_set_depth_test(self._h, int(compare)))

    def update_depth_buffer(self, depth: np.ndarray) -> None:
        """float32 [height, width] NDC depth in [0, 1], row 0 at the top (what the gizmo and measurement passes wrote); copied."""
        d = np.ascontiguousarray(depth, np.float32)
        if d.ndim != 2:
            raise ValueError("depth buffer must be [height, width]")
        _lib.check(self._L.gsx_viewer_upload_depth_buffer(self._h, _f32p(d), int(d.shape[1]), int(d.shape[0])))

    def set_depth_buffer_device(self, ptr, width: int, height: int, row_pitch_bytes: int) -> None:
        """Caller-owned device memory (e.g. ``tensor.data_ptr()``), read in place; ``ptr = None`` detaches it.  Frames in flight that
        were dealt before the call keep reading the buffer they were dealt with (each lane's snapshot is its own)."""
        _lib.check(self._L.gsx_viewer_set_depth_buffer_device(self._h, C.c_void_p(ptr) if ptr else None, int(width), int(height),
                                                              int(row_pitch_bytes)))

    # -- overlay lines: the app's measurement pass, drawn by the library with depth write (src/renderer/measurement.rs) --
    def update_hit_pairs(self, lines) -> None:
        """``MeasurementRenderer::update_hit_pairs``: ``HitPair`` records (an array of ``HIT_PAIR_DTYPE``, or a sequence of them);
        empty or ``None`` clears.  The lines are drawn by the first ``preprocess`` of every frame from then on, `Less` with depth
        write against the caller's depth buffer (1 where there is none); with ``DepthCompare.Less`` the splats are tested against
        the result (``gsx.h``, the overlay block)."""
        if lines is None or len(lines) == 0:
            _lib.check(self._L.gsx_viewer_set_overlay_lines(self._h, None, 0))
            return
        if not isinstance(lines, np.ndarray):
            lines = np.concatenate([np.asarray(x, HIT_PAIR_DTYPE).reshape(-1) for x in lines])
        a = np.ascontiguousarray(lines, HIT_PAIR_DTYPE).reshape(-1)
        _lib.check(self._L.gsx_viewer_set_overlay_lines(self._h, a.ctypes.data, int(a.shape[0])))

    # -- mask gizmos: the mask shapes' wireframes (gs::MaskGizmo, src/tab/scene.rs:2211-2247, 2283-2293), drawn before the lines --
    def set_mask_gizmos(self, gizmos) -> None:
        """Records of ``MASK_GIZMO_DTYPE`` (an array, or a sequence of them: ``mask.gizmo_records``) in draw order: for each render
        key that model's visible boxes, then its visible ellipsoids, in world space; empty or ``None`` clears.  Drawn by the first
        ``preprocess`` of every frame from then on, before the measurement lines and with their depth state (``gsx.h``, the gizmo
        block)."""
        if gizmos is None or len(gizmos) == 0:
            _lib.check(self._L.gsx_viewer_set_mask_gizmos(self._h, None, 0))
            return
        if not isinstance(gizmos, np.ndarray):
            gizmos = np.concatenate([np.asarray(x, MASK_GIZMO_DTYPE).reshape(-1) for x in gizmos])
        a = np.ascontiguousarray(gizmos, MASK_GIZMO_DTYPE).reshape(-1)
        _lib.check(self._L.gsx_viewer_set_mask_gizmos(self._h, a.ctypes.data, int(a.shape[0])))

    def download_overlay(self):
        """``(rgba, depth)`` of the last frame's overlay: premultiplied float32 [H, W, 4] (zeros where no line is) and the effective
        depth float32 [H, W] the splats were (or would be) tested against."""
        w, h = self.size
        rgba, depth = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
        _lib.check(self._L.gsx_download_overlay(self._h, _f32p(rgba), _f32p(depth)))
        return rgba, depth

    def overlay_device_ptrs(self):
        """Device addresses ``(rgba, tile_flags, depth)`` of the last frame's overlay (zero-copy consumers)."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(self._L.gsx_overlay_device_ptrs(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_render_options(self, **kw) -> None:
        """``gsx_render_options``: progressive depth slabs (default on), first_slab_divisor, min_slab, growth."""
        o = _lib.RenderOptions()
        self._L.gsx_render_options_default(C.byref(o))
        for k, val in kw.items():
            if not hasattr(o, k):
                raise KeyError(k)
            setattr(o, k, float(val) if k == "spec_margin" else int(val))
        _lib.check(self._L.gsx_viewer_set_render_options(self._h, C.byref(o)))

    # -- frame execution --
    def poll(self) -> None:
        """``device.poll(wgpu::Maintain::Wait)`` (src/tab/scene.rs:614, 873)."""
        _lib.check(self._L.gsx_sync(self._h))

    def render_frame(self, model_render_keys: Sequence[str]) -> None:
        """preprocess + sort every key, then render: the whole per-frame protocol in one call."""
        keys = [k.encode() for k in model_render_keys]
        arr = (C.c_char_p * max(len(keys), 1))(*keys)
        _lib.check(self._L.gsx_render_frame(self._h, arr, len(keys)))

    # -- the splats' depth per pixel (spec section 25) --
    def render_depth_map(self, model_render_keys: Sequence[str], threshold: float = 0.5, ndc: bool = False, planes: bool = True) -> DepthMap:
        """``gsx_render_depth_map``: walks the models in the order ``render_frame`` composites them (the last key first) with the
        viewer's current camera and keeps per pixel the surface depth (first record after whose blend ``T < threshold``), its Gaussian
        and model, ``sum w * d``, ``sum w`` and the final ``T``.  The planes stay on the device (``depth_map_device_ptrs``); with
        ``ndc=True`` an NDC depth plane is written as well, which ``set_depth_buffer_device`` takes as it is.  The framebuffer keeps
        the last frame; the next ``render_frame`` is the frame it would have been.  ``planes=False`` downloads nothing."""
        keys = [k.encode() for k in model_render_keys]
        arr = (C.c_char_p * max(len(keys), 1))(*keys)
        desc = _lib.DepthMapDesc(_lib.GSX_DEPTH_MAP_NDC if ndc else 0, float(threshold))
        w, h = self.size
        f32 = [np.empty((h, w), np.float32) if planes else None for _ in range(4)]
        u32 = [np.empty((h, w), np.uint32) if planes else None for _ in range(2)]
        out = _lib.DepthMapStats()
        _lib.check(self._L.gsx_render_depth_map(self._h, arr, len(keys), C.byref(desc), *[a.ctypes.data if planes else None for a in f32 + u32],
                                                C.byref(out)))
        return DepthMap(*f32, *u32, int(out.n_covered), int(out.n_crossed), np.float32(out.surface_min), np.float32(out.surface_max), int(out.models))

    def depth_map_device_ptrs(self) -> dict:
        """Device addresses of the last depth map's planes by name (``surface``, ``sum``, ``alpha``, ``transmittance``, ``index``,
        ``layer``, ``ndc`` — ``None`` unless the call asked for it) and its ``size``; valid until the next ``render_depth_map``, a
        viewport change or the viewer's end."""
        names = ("surface", "sum", "alpha", "transmittance", "index", "layer", "ndc")
        ptrs = [C.c_void_p() for _ in names]
        w, h = C.c_uint32(), C.c_uint32()
        _lib.check(self._L.gsx_depth_map_device_ptrs(self._h, *[C.byref(p) for p in ptrs], C.byref(w), C.byref(h)))
        out = {n: p.value for n, p in zip(names, ptrs)}
        out["size"] = (int(w.value), int(h.value))
        return out

    # -- several GPUs: the index-sharded frame as one library call (include/gsx.h "multi-GPU"; no reference counterpart) --
    def comm_init_group(self, group: "CommGroup", rank: int) -> None:
        """Seat `rank` of an in-process group: one host thread + one viewer per GPU, collectives as peer copies."""
        _lib.check(self._L.gsx_viewer_comm_init_group(self._h, group._h, int(rank)))
        self._group = group  # keeps the group alive as long as the viewer

    def comm_init_rccl(self, world: int, rank: int, unique_id: bytes) -> None:
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _lib.check(self._L.gsx_viewer_comm_init(self._h, int(world), int(rank), buf))

    def comm_init_custom(self, world: int, rank: int, all_to_all, all_gather) -> None:
        """A transport of the caller's own: two callables (d_send, d_recv, bytes, hip_stream) -> gsx_status that enqueue."""
        self._comm_fns = (_lib.COMM_FN(lambda ctx, s, r, b, st: int(all_to_all(s, r, b, st) or 0)),
                          _lib.COMM_FN(lambda ctx, s, r, b, st: int(all_gather(s, r, b, st) or 0)))
        _lib.check(self._L.gsx_viewer_comm_init_custom(self._h, int(world), int(rank), self._comm_fns[0], self._comm_fns[1], None))

    def comm_init_custom_v(self, world: int, rank: int, all_to_all_v, gather_v) -> None:
        """A transport of the caller's own that moves pieces of UNEQUAL size (``gsx_viewer_comm_init_custom_v``):
        ``all_to_all_v(d_send, send_offsets, send_bytes, d_recv, recv_offsets, recv_bytes, hip_stream)`` and
        ``gather_v(d_send, send_bytes, d_recv, recv_offsets, recv_bytes, root, hip_stream)`` -> gsx_status; the offset / size
        arguments arrive as lists of `world` ints.  Both enqueue on ``hip_stream``."""
        w = int(world)

        def a2a(ctx, s, so, sb, r, ro, rb, st):
            return int(all_to_all_v(s, [so[i] for i in range(w)], [sb[i] for i in range(w)], r, [ro[i] for i in range(w)], [rb[i] for i in range(w)], st) or 0)

        def gat(ctx, s, n, r, ro, rb, root, st):
            return int(gather_v(s, n, r, [ro[i] for i in range(w)], [rb[i] for i in range(w)], root, st) or 0)

        self._comm_fns = (_lib.COMM_A2A_V_FN(a2a), _lib.COMM_GATHER_V_FN(gat))
        _lib.check(self._L.gsx_viewer_comm_init_custom_v(self._h, w, int(rank), self._comm_fns[0], self._comm_fns[1], None))

    def comm_init_custom_v_native(self, world: int, rank: int, all_to_all_v_ptr, gather_v_ptr, ctx) -> None:
        """The same with two NATIVE functions (addresses or ctypes function objects of a shared library) and their context pointer:
        nothing of the transport runs in Python (tools/replay_transport.cpp)."""
        a = C.cast(all_to_all_v_ptr, _lib.COMM_A2A_V_FN)
        g = C.cast(gather_v_ptr, _lib.COMM_GATHER_V_FN)
        self._comm_fns = (a, g)
        _lib.check(self._L.gsx_viewer_comm_init_custom_v(self._h, int(world), int(rank), a, g, C.c_void_p(ctx)))

    def comm_destroy(self) -> None:
        _lib.check(self._L.gsx_viewer_comm_destroy(self._h))

    def debug_download_lane_framebuffer(self, lane: int, size=None) -> np.ndarray:
        """Tests: lane `lane`'s framebuffer once its stream has drained, WITHOUT completing the frames in flight (size: the viewport of
        the frame that lane holds, if the viewer's has changed since)."""
        w, h = size if size is not None else self.size
        out = np.empty((h, w, 4), np.float32)
        _lib.check(self._L.gsx_debug_download_lane_framebuffer(self._h, int(lane), out.ctypes.data, out.size))
        return out

    def shard_render_frame(self, key: str, shard_records_max: int, speculate: bool = True, margin: float = 0.25, radius: int = 3) -> None:
        """One whole index-sharded frame of this rank (``gsx_shard_render_frame``)."""
        _lib.check(self._L.gsx_shard_render_frame(self._h, key.encode(), int(shard_records_max), 1 if speculate else 0, float(margin), int(radius)))

    def shard_render_frame_keys(self, model_render_keys: Sequence[str], shard_records_max: Sequence[int], speculate: bool = True,
                                margin: float = 0.25, radius: int = 3) -> None:
        """Layered models, far -> near like ``renderer.render`` (``gsx_shard_render_frame_keys``)."""
        keys = [k.encode() for k in model_render_keys]
        arr = (C.c_char_p * len(keys))(*keys)
        mx = (C.c_uint32 * len(keys))(*[int(x) for x in shard_records_max])
        _lib.check(self._L.gsx_shard_render_frame_keys(self._h, arr, len(keys), mx, 1 if speculate else 0, float(margin), int(radius)))

    def shard_set_limits(self, key: str, limits: np.ndarray) -> None:
        """Per-tile depth-key limits (uint32 [tiles_y, tiles_x]) the next sharded frame uses instead of the last frame's."""
        a = np.ascontiguousarray(limits, np.uint32)
        _lib.check(self._L.gsx_shard_set_limits(self._h, key.encode(), a.ctypes.data))

    def shard_set_slot_records(self, key: str, records: int) -> None:
        _lib.check(self._L.gsx_shard_set_slot_records(self._h, key.encode(), int(records)))

    def shard_set_gather_root(self, root: int) -> None:
        """-1: every rank's framebuffer holds the whole frame after a sharded frame (default); r >= 0: only rank r's does."""
        _lib.check(self._L.gsx_shard_set_gather_root(self._h, int(root)))

    def shard_set_band_edges(self, world: int, edges) -> None:
        """Rank g owns the tile rows [edges[g], edges[g + 1]) in every following sharded frame (None: the library's own layout)."""
        if edges is None:
            _lib.check(self._L.gsx_shard_set_band_edges(self._h, int(world), None))
            return
        a = np.ascontiguousarray(edges, np.uint32)
        assert a.size == world + 1
        _lib.check(self._L.gsx_shard_set_band_edges(self._h, int(world), _u32p(a)))

    def shard_get_band_edges(self, world: int) -> np.ndarray:
        """The band layout the last sharded frame used (uint32 [world + 1] tile rows)."""
        out = np.empty(world + 1, np.uint32)
        _lib.check(self._L.gsx_shard_get_band_edges(self._h, int(world), _u32p(out)))
        return out

    def shard_set_balance(self, enabled: bool) -> None:
        """Balance the bands by the previous frame's per-row work (default, where the transport moves unequal pieces) or keep them equal."""
        _lib.check(self._L.gsx_shard_set_balance(self._h, 1 if enabled else 0))

    def shard_download_limits(self, key: str) -> np.ndarray:
        w, h = self.size
        out = np.empty(((h + 15) // 16, (w + 15) // 16), np.uint32)
        _lib.check(self._L.gsx_shard_download_limits(self._h, key.encode(), _u32p(out), out.size))
        return out

    def comm_info(self) -> dict:
        """What the communicator itself says (``gsx_viewer_comm_info``): transport, the ranks RCCL counted, its version."""
        ci = _lib.CommInfo()
        _lib.check(self._L.gsx_viewer_comm_info(self._h, C.byref(ci)))
        out = {n: int(getattr(ci, n)) for n, _ in _lib.CommInfo._fields_}
        out["transport"] = ("none", "rccl", "in-process group", "custom")[min(out["transport"], 3)]
        return out

    def shard_stats(self, reset: bool = False) -> dict:
        st = _lib.ShardStats()
        _lib.check(self._L.gsx_shard_get_stats(self._h, C.byref(st), 1 if reset else 0))
        return {n: int(getattr(st, n)) for n, _ in _lib.ShardStats._fields_}

    # -- readback --
    def download_framebuffer(self) -> np.ndarray:
        """float32 [H, W, 4]: premultiplied r,g,b and transmittance T."""
        w, h = self.size
        out = np.empty((h, w, 4), np.float32)
        _lib.check(self._L.gsx_download_framebuffer(self._h, _f32p(out), out.size))
        return out

    def download_rgba8(self, background=(0.0, 0.0, 0.0)) -> np.ndarray:
        w, h = self.size
        out = np.empty((h, w, 4), np.uint8)
        bg = np.ascontiguousarray(background, np.float32).reshape(3)
        _lib.check(self._L.gsx_download_rgba8(self._h, _f32p(bg), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out

    def framebuffer_device_ptr(self):
        p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
        _lib.check(self._L.gsx_framebuffer_device_ptr(self._h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, int(w.value), int(h.value)

    # -- parity / introspection --
    def frame_stats(self, key: str) -> dict:
        st = _lib.FrameStats()
        _lib.check(self._L.gsx_model_frame_stats(self._h, key.encode(), C.byref(st)))
        return dict(n_gaussians=int(st.n_gaussians), n_visible=int(st.n_visible), n_tile_entries=int(st.n_tile_entries),
                    n_sorted=int(st.n_sorted), n_repair_tiles=int(st.n_repair_tiles), n_repair_sorted=int(st.n_repair_sorted),
                    speculated=bool(st.speculated), overflow_slabs=int(st.overflow_slabs))

    def download_projection(self, key: str) -> dict:
        n = self.models[key].gaussian_buffers.gaussians_buffer.len()
        out = dict(key=np.empty(n, np.uint32), rect=np.empty((n, 4), np.uint32), mean2d=np.empty((n, 2), np.float32),
                   conic_opacity=np.empty((n, 4), np.float32), rgb=np.empty((n, 3), np.float32))
        _lib.check(self._L.gsx_model_download_projection(self._h, key.encode(), _u32p(out["key"]), _u32p(out["rect"]),
                                                         _f32p(out["mean2d"]), _f32p(out["conic_opacity"]), _f32p(out["rgb"])))
        out["n_visible"] = int(np.count_nonzero(out["key"] != 0xFFFFFFFF))
        return out

    def download_sorted(self, key: str) -> np.ndarray:
        nv = C.c_uint64()
        _lib.check(self._L.gsx_model_download_sorted(self._h, key.encode(), None, 0, C.byref(nv)))
        idx = np.empty(max(int(nv.value), 1), np.uint32)
        _lib.check(self._L.gsx_model_download_sorted(self._h, key.encode(), _u32p(idx), idx.size, C.byref(nv)))
        return idx[: int(nv.value)]

    def download_tile_lists(self, key: str):
        st = self.frame_stats(key)
        w, h = self.size
        tiles = ((w + 15) // 16) * ((h + 15) // 16)
        off = np.empty(tiles + 1, np.uint32)
        lst = np.empty(max(st["n_tile_entries"], 1), np.uint32)
        _lib.check(self._L.gsx_model_download_tile_lists(self._h, key.encode(), _u32p(off), off.size, _u32p(lst), lst.size))
        return off, lst[: st["n_tile_entries"]]

    # -- timing --
    def launch_stats(self, reset: bool = False) -> dict:
        """How this viewer's (and its lanes') kernel launches reached the device: ``gsx_launch_stats`` (csrc/gsx_launch.h)."""
        ls = _lib.LaunchStats()
        _lib.check(self._L.gsx_viewer_launch_stats(self._h, C.byref(ls), 1 if reset else 0))
        return {n: int(getattr(ls, n)) for n, _ in ls._fields_}

    def set_pass_timing(self, enabled, passes=None) -> None:
        """``passes``: names from ``_lib.GSX_PASS_NAMES`` to bracket with events (default: all)."""
        code = 0
        if enabled:
            code = 1 if passes is None else sum(1 << (_lib.GSX_PASS_NAMES.index(p) + 1) for p in passes)
        _lib.check(self._L.gsx_set_pass_timing(self._h, code))

    def get_pass_timing(self) -> dict:
        ms = (C.c_float * _lib.GSX_PASS_COUNT)()
        launches = (C.c_uint32 * _lib.GSX_PASS_COUNT)()
        _lib.check(self._L.gsx_get_pass_timing(self._h, ms, launches))
        return {n: dict(ms=float(ms[i]), launches=int(launches[i])) for i, n in enumerate(_lib.GSX_PASS_NAMES)}


def set_launch_graphs(enabled) -> None:
    """Process-wide: frame-level entry points submit their launches as cached HIP graphs while their stream is busy (True / 1), always
    (2: tests) or never (False / 0, the default: the graphs save host time, not device time — csrc/gsx_launch.h)."""
    _lib.load().gsx_debug_set_launch_graphs(int(enabled))


def launch_count() -> int:
    """Kernel launches this process has asked libgsx for so far."""
    return int(_lib.load().gsx_debug_launch_count())


def device_bytes() -> int:
    """Device memory the library's buffers hold in this process right now (``gsx_debug_device_bytes``)."""
    return int(_lib.load().gsx_debug_device_bytes())


def render_keys_far_to_near(viewer_models_centers: dict, camera_pos) -> list:
    """``model_render_keys`` exactly as the app builds them (src/tab/scene.rs:533-558)."""
    from .camera import model_render_order

    return model_render_order(camera_pos, viewer_models_centers)
