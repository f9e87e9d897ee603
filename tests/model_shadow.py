"""A host shadow of a viewer's models, for tests/test_model_shadow_cpu.py and tests/test_gpu_model_fuzz.py: what a long session of
model operations (gsx_model_extract, _merge, _convert, _set_pod_kind, _apply_transform, _import_ply, _decimate, the selects by
property, neighbour count, cluster, nearest neighbours, nearest in another model and visibility, gsx_mask_evaluate, the uploads,
gsx_model_visibility and gsx_render_depth_map) leaves in every model, kept on the host, without a GPU and without libgsx.  Per model
key: the pod kind, the dequantised planes as gsx_model_download_pod returns them, the model transform, the mask bits, the selection
bits, the stored edit records (each or none), show-unedited and the resident visibility planes (or none).

No arithmetic is stated here.  Every operation is applied with the restatements the repository already has: the kept set, its order
and the participation set of the spatial calls are tests/extract_ref.py's `kept`; the selects are property_ref / neighbors_ref /
clusters_ref / knn_ref (bit-exact float32 answers: the words are compared exactly); a mask program is oracle.mask_evaluate over the
shadow's positions; positions after a transform or a baked merge are transform_ref.position, bit for bit; bounds are
bounds_ref.reference.  Extract, an identity-source merge and a translation reproduce the shadow's own rows for the kept indices,
byte for byte, and every row outside a transform's kept set stays as it was.  A decimate's cells, map, statistics and order are
decimate_ref.assign's; its one-member cells are the shadow's own rows; its merged rows are VERIFIED, not adopted: they are the float32
rows of tests/decimate_driver.cpp (which shares csrc/decimate_math.h with the kernels) played on the shadow's planes of the source,
uploaded in the source's kind into the other viewer, and the two downloads must be the same bytes in every plane.  The nearest calls
across two models are nearest_ref's `brute` under the matrix nearest_ref.model_matrix gives (index, d2 and every selection word bit for
bit); the delta of an align step is BOUNDED, not exact: within tests/test_gpu_nearest.py's formula of the float64 SVD solve.

What the shadow ADOPTS from the device instead of verifying, on purpose (the per-op suites bound these against float64): the baked
covariance and SH of gsx_model_merge and of a scaling or rotating gsx_model_apply_transform (the kept rows only), the covariance and
SH a conversion requantises (their yardstick is an upload of the shadow's planes into a model of the new kind, compared on the device
by the GPU test), the colour, SH and covariance a PLY round trip writes (the positions are checked), the planes of a fresh upload in a
compressed kind, and the selection and stored edits a frame itself writes (a rectangle query's postprocess, a selection edit that
persists: both viewers of the fuzz run those, their downloads are compared, the shadow takes them).  `verify` checks the count, the
order and every row the shadow does know before `adopt` takes the rest.

The calls that draw a model's own unspeculated frame in the middle of a session (csrc/frame_isolation.h) are three op kinds.  "visibility"
is the CAMERA op that hides models, so they go by other names.  `vis_view` (READ_ONLY: gsx_model_visibility of `key`, `accumulate`;
`prime` is the pose of a first view where an accumulating call finds no planes), `depth_map` (READ_ONLY: gsx_render_depth_map over the
step's painter's order, hidden models left out, `threshold` one of THRESHOLDS, `ndc`, and `as_depth_buffer`: the ndc plane becomes the
depth buffer of the frames that follow; `hide` and `size` hide one more model and change the viewport first) and `select_visibility`
(SELECTS: `measure`, `op`, `flt`, the range as two quantile fractions `q_lo`, `q_hi` of the positive values or None for "never seen" —
the draw cannot know the planes, so `lo` and `hi` are resolved when the op is applied, from the shadow's adopted planes; `view`: a model
without planes gets a view first, `touch`: a mask, a selection and an edit change come between the view and the select).  Both calls
refuse while the depth test, the overlay lines or the gizmos are on: with `clear` those go off first, on both viewers, through the
ordinary state ops, and the View follows; without it the call is expected to be refused (where nothing is on, `feature` goes on first).
A refusal must leave what is resident as it was, so something always is: where the model holds no planes, or the viewer no depth map of
the viewport, the session puts an unrefused call of the same kind in front (`primed` in the call's record), with the features that are
on switched off for it and on again after.  Every fourth depth map is drawn without the ndc plane.  The calls that drop a model's
planes are steered to meet some: set_pod_kind and remove_add go to a model that holds planes, and where there is none the drawn model
gets a view first (`view_first`), as does every other transform.  An op that takes a view or changes state first (`view_first`, and a
select_visibility's `view` and `touch`) enqueues its frames in flight itself, after that and right in front of its own call, so that
"two frames enqueued and not waited for" is true of the call the record names; after a `touch` a frame of both viewers comes in
between, because a frame of `live` alone would persist a selection edit onto the selection just uploaded.
The shadow keeps per model `vis` — None, or the planes adopted from the device after they were verified (peak float32, the weight as
fixed-point int64, pixels uint32), `views`, where they were taken and which mask / selection / edit changes they survived — and sets
it to None exactly where the library calls drop_visibility: a fresh upload (a new ShadowModel), set_pod_kind, remove_add and a
gsx_model_apply_transform that is not the identity and keeps something; a model made by extract, convert, merge, decimate or a PLY
round trip starts without.  Mask, selection, edit, show-unedited, model-transform and camera changes keep it.  After a dropping call
on a model that held planes a select by them must be refused at once (`_planes_dropped`).  Per session `depth_map` is None or the size,
the ndc flag and the adopted planes; a `viewport` op of another size sets it to None.  Without a device there are no planes: `vis`
then records residency alone, which is all that conditions (i) to (m) of the fuzz (`unmet_views`) depend on.

`plan(seed)` is the schedule of a fuzz seed (every op kind once in a seeded order, then random ones, camera steps in between and a
run of them after each op that changes a model); `Session` draws each op's parameters from the shadow as it stands and applies it, to
the shadow alone (the CPU test) or in lock-step with a device (`dev`: tests/test_gpu_model_fuzz.py's adaptor)."""
from __future__ import annotations

import dataclasses
import hashlib

import numpy as np

import oracle
from tests import bounds_ref as B
from tests import clusters_ref as CL
from tests import common
from tests import decimate_ref as D
from tests import extract_ref as X
from tests import knn_ref as K
from tests import merge_ref as M
from tests import nearest_ref as R
from tests import neighbors_ref as N
from tests import property_ref as P
from tests import transform_ref as T
from wgpu_3dgs_viewer_app_amd.mask import MaskOp, MaskShape, MaskShapeKind, pack_program
from wgpu_3dgs_viewer_app_amd.query import default_edits

F = np.float32
W, H = 96, 64  # tests/model_ops.py's viewport
PLANES = ("pos", "color", "sh", "cov3d")
KINDS = [(sh, cov) for sh in range(4) for cov in range(2)]  # (ShKind, Cov3dKind) as integers
SINGLE, NORM8_HALF = (0, 0), (2, 1)
#: the pod kind a seed's viewer starts in (and creates models in): every kind over eight seeds, Single + Single and Norm8 + Half twice
START_KINDS = [SINGLE, NORM8_HALF, (1, 1), (1, 0), (2, 0), (3, 1), (0, 1), (3, 0)]
DEFAULT_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
MIN_N, MAX_N = 200, 5000  # no model shrinks below / grows above (the brute-force restatements stay well under a second)
MAX_MODELS = 4
#: camera steps after an op that changes a model.  gsx_model_set_pod_kind, a new model and a model whose planes moved start with an
#: unspeculated frame on every lane (three lanes at most), then speculate: the run must reach past them (condition (c))
POST_OP_RUN = 5
EXTRA_OPS = 2
SPATIAL_N = 2500

CAMERA = ("cam_step", "cam_jump", "viewport", "visibility", "display", "model_transform")
STATE = ("mask_eval", "sel_upload", "sel_edit", "edits_upload", "unedited", "rect_query")
SELECTS = ("select_range", "select_neighbors", "select_clusters", "select_knn", "select_nearest", "select_visibility")
READ_ONLY = ("bounds", "histogram", "property_values", "neighbors", "clusters", "knn", "export", "export_ply", "decimate_edge", "nearest", "align_step",
             "vis_view", "depth_map")
VIEW_CALLS = ("vis_view", "depth_map")  # they draw a model's own frame in the middle of the session (csrc/frame_isolation.h)
MODEL_CHANGING = ("xf_translate", "xf_scale", "xf_full", "set_pod_kind", "convert", "extract", "merge", "ply_roundtrip", "remove_add", "decimate")
FEATURES = ("depth_test", "hit_pairs", "gizmos")
SPATIAL = ("select_neighbors", "select_clusters", "select_knn", "neighbors", "clusters", "knn", "nearest", "select_nearest", "align_step")
NEAREST_FAMILY = ("nearest", "select_nearest", "align_step")  # two keys: the queries' model `key` and the targets' `dst`
OP_KINDS = CAMERA + STATE + SELECTS + READ_ONLY + MODEL_CHANGING + FEATURES
#: the variants condition (b) asks a non-trivial hit set of, each at least once over the seed set
SELECT_VARIANTS = ("select_range:model", "select_range:world", "select_neighbors", "select_clusters:0", "select_clusters:1", "select_clusters:2",
                   "select_knn:range", "select_knn:std_ratio", "select_nearest:range", "select_nearest:transfer",
                   "select_visibility:peak", "select_visibility:weight", "select_visibility:pixels")
#: the variants whose hit sets only the device run can show: the shadow holds no visibility planes without a device to adopt them from
DEVICE_ONLY_VARIANTS = ("select_visibility:peak", "select_visibility:weight", "select_visibility:pixels")
VIS_MEASURES = ("peak", "weight", "pixels")  # GSX_VIS_PEAK, _WEIGHT, _PIXELS
THRESHOLDS = (1e-4, 0.5, 1.0)  # of a depth map: t_epsilon (the crossing is the closing), the median surface, the front surface
VIS_QUANTILES = (0.25, 0.6)  # a select_visibility's range, as fractions of the positive values of its measure
SEEN_AT_ALL = (1e-45, float("inf"))  # the range of "every Gaussian that was seen": its hit count is n_seen
PARTIAL_OR_LARGE = ((83, 51), (320, 240))
DROPPERS = ("apply_transform", "set_pod_kind", "remove_add")  # the calls that drop a model's visibility planes (condition (j))
#: condition (f): src != dst under GSX_NEAREST_MODEL_TRANSFORMS; src != dst of different pod kinds; src == dst with different filters and
#: a query that is no target; a max_distance within which some but not all queries find a target
NEAREST_CASES = ("nearest:model_transforms", "nearest:kinds", "nearest:same_disjoint", "nearest:max_distance")
VIEWPORTS = [(W, H), (80, 64), (96, 80), (83, 51), (320, 240)]  # the last: 300 tiles, blocks of several tiles
MASK_EXPRS = [None, "0", "!1", "0 - 1", "0 | 1"]
FILTERS = [0, X.MASKED, X.SKIP_HIDDEN, X.MASKED | X.SKIP_HIDDEN, X.SELECTED, X.MASKED | X.SELECTED, X.SKIP_HIDDEN | X.SELECTED,
           X.MASKED | X.SKIP_HIDDEN | X.SELECTED]
ZERO3, ONE3, IDENT = np.zeros(3, F), np.ones(3, F), np.array([0, 0, 0, 1], F)
IDENTITY34 = np.eye(3, 4, dtype=F)
ALIGN_TOL_MAX = 1e-3  # an align draw whose tolerance formula exceeds this is drawn again (tests/test_gpu_nearest.py's bound on "the inverse motion")


def mask_shapes():
    return [MaskShape(MaskShapeKind.Box, pos=np.zeros(3, F), scale=np.array([1.2, 1.2, 1.2], F)),
            MaskShape(MaskShapeKind.Ellipsoid, pos=np.array([0.4, 0.0, 0.3], F), scale=np.array([1.0, 0.8, 1.0], F))]


def normalise_edits(edits):
    """the records as the library keeps them: a record without ENABLED reads as the default (gsx_model_download_edits)"""
    if edits is None:
        return None
    out = default_edits(edits.shape[0])
    on = (edits["flag"] & X.EDIT_ENABLED) != 0
    out[on] = edits[on]
    return out


def random_edits(n, rseed):
    rng = np.random.default_rng(rseed)
    e = default_edits(n)
    on = rng.random(n) < 0.3
    k = int(on.sum())
    e["flag"][on] = rng.choice([1, 3, 5], k)
    e["color"][on] = rng.uniform(0, 1, (k, 3))
    e["alpha"][on] = rng.uniform(0.3, 1.5, k)
    return e


def random_bits(n, rseed, density):
    return np.random.default_rng(rseed).random(n) < density


@dataclasses.dataclass
class ShadowModel:
    kind: tuple
    planes: list          # pos (n, 3) f32, color (n,) u32, sh (n, 45) f32, cov3d (n, 6) f32
    mt: tuple             # pos, quat (x, y, z, w), scale: float32
    mask: np.ndarray | None = None
    sel: np.ndarray | None = None
    edits: np.ndarray | None = None
    unedited: bool = False
    #: the resident visibility planes (Model::vis), or None: `views`, `at` (the (pose, viewport) of every view folded in), `survived`
    #: (the mask / sel / edit changes since the first of them) and the planes adopted from the device after they were verified: peak
    #: float32, weight as fixed-point int64 (units of 2^-24), pixels uint32.  Without a device the planes are None: residency alone.
    vis: dict | None = None
    vis_lost: str | None = None  # what dropped resident planes last (the library's drop_visibility), while none were taken since

    def drop_vis(self, by):
        if self.vis is not None:
            self.vis, self.vis_lost = None, by

    @property
    def n(self):
        return self.planes[0].shape[0]

    @property
    def pos(self):
        return self.planes[0]

    @property
    def color(self):
        return self.planes[1]

    def kept(self, flt=0, invert=False):
        return X.kept(self.n, flt, X.INVERT if invert else 0, self.mask, self.sel, None if self.edits is None else self.edits["flag"])

    def passes(self, flt=0):
        out = np.zeros(self.n, bool)
        out[self.kept(flt)] = True
        return out

    def part(self, flt=0):
        return N.participates(self.pos, self.passes(flt))

    def selection(self):
        return np.zeros(self.n, bool) if self.sel is None else self.sel

    def world(self):
        """property_ref's (R, s, t) of a WORLD position; None under the identity"""
        t, q, s = self.mt
        return None if M.is_identity(t, q, s) else (T.quat_rows(q).reshape(9), s, t)

    def values(self, prop, world=False):
        return P.values_pc(prop, self.pos, self.color, self.world() if world else None)


_MEMO: dict = {}


def memo(fn, *arrays_then_args):
    """fn(*arrays_then_args), remembered by the bytes of its arguments: a draw and the op it draws ask the same brute-force
    restatement of the same positions"""
    h = hashlib.blake2b((fn.__module__ + "." + fn.__qualname__).encode(), digest_size=16)
    for a in arrays_then_args:
        h.update(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else repr(a).encode())
    key = h.digest()
    if key not in _MEMO:
        if len(_MEMO) > 64:
            _MEMO.clear()
        _MEMO[key] = fn(*arrays_then_args)
    return _MEMO[key]


def _rows(planes, idx):
    return [np.ascontiguousarray(a[idx]) for a in planes]


def _all(n, value=True):
    return [np.full(n, value, bool) for _ in PLANES]


class Shadow:
    def __init__(self):
        self.models: dict[str, ShadowModel] = {}

    def add(self, key, kind, planes, mt=(ZERO3, IDENT, ONE3)):
        assert key not in self.models and len(self.models) < MAX_MODELS + 1
        n = np.asarray(planes[0]).shape[0]
        held = [np.array(a, t).reshape(shape) for a, t, shape in zip(planes, (F, np.uint32, F, F), ((n, 3), (n,), (n, 45), (n, 6)))]
        self.models[key] = ShadowModel(tuple(int(k) for k in kind), held, tuple(np.array(a, F) for a in mt))
        return self.models[key]

    def remove(self, key):
        del self.models[key]

    # ---- the device's planes against what the shadow knows ----
    def verify(self, key, got, exact, what=""):
        """count, order and every row the shadow knows: `exact[p]` marks the rows of plane p that must be the shadow's bytes"""
        m = self.models[key]
        for name, want, have, rows in zip(PLANES, m.planes, got, exact):
            assert have.shape == want.shape, (what, key, name, have.shape, want.shape)
            a, b = (np.ascontiguousarray(x).reshape(m.n, -1).view(np.uint32) for x in (have, want))  # (bits: a NaN equals itself)
            bad = np.nonzero(rows & (a != b).any(axis=1))[0]
            assert bad.size == 0, (what, key, name, f"{bad.size} rows differ, first {bad[:4].tolist()}")

    def adopt(self, key, got):
        self.models[key].planes = [np.array(a) for a in got]

    # ---- operations ----
    def extract(self, src, dst, flt=0, invert=False, drop_edits=False, kind=None):
        """gsx_model_extract, or gsx_model_convert into `kind`.  Returns (count, exact rows of dst's planes); 0 creates nothing."""
        s = self.models[src]
        idx = s.kept(flt, invert)
        if idx.size == 0:
            return 0, None
        kind = s.kind if kind is None else tuple(kind)
        d = self.add(dst, kind, _rows(s.planes, idx), s.mt)
        if s.edits is not None and not drop_edits:
            d.edits = s.edits[idx].copy()
        same = kind == s.kind
        return int(idx.size), [np.full(d.n, True), np.full(d.n, True), np.full(d.n, same), np.full(d.n, same)]

    def set_pod_kind(self, key, kind):
        m = self.models[key]
        same = tuple(kind) == m.kind
        m.kind = tuple(kind)
        m.drop_vis("set_pod_kind")  # (the library replaces the model)
        return [np.full(m.n, True), np.full(m.n, True), np.full(m.n, same), np.full(m.n, same)]

    def merge(self, dst, srcs, flt=0, invert=False, drop_edits=False):
        """gsx_model_merge.  Returns (total, counts, exact rows): an identity source's rows are its stored rows; a baked source's
        positions are transform_ref.position, its colour words are carried, its covariance and SH are the device's"""
        models = [self.models[k] for k in srcs]
        assert all(m.kind == models[0].kind for m in models)
        parts, exact, counts, edits = [], [], [], []
        for m in models:
            idx = m.kept(flt, invert)
            rows = _rows(m.planes, idx)
            ident = M.is_identity(*m.mt)
            if not ident:
                rows[0] = T.position(rows[0], *m.mt)
            parts.append(rows)
            exact.append([np.full(idx.size, True), np.full(idx.size, True), np.full(idx.size, ident), np.full(idx.size, ident)])
            counts.append(int(idx.size))
            edits.append(default_edits(idx.size) if m.edits is None else m.edits[idx])
        total = sum(counts)
        if total == 0:
            return 0, counts, None
        d = self.add(dst, models[0].kind, [np.concatenate([p[k] for p in parts]) for k in range(4)])
        if not drop_edits and any(m.edits is not None for m in models):
            d.edits = np.concatenate(edits)
        return total, counts, [np.concatenate([e[k] for e in exact]) for k in range(4)]

    def apply_transform(self, key, t, q, s, pivot=(0.0, 0.0, 0.0), flt=0, invert=False):
        """gsx_model_apply_transform.  Returns (count, exact rows): rows outside the kept set stay; inside, the positions are
        transform_ref.position, the colour is carried, the covariance is the device's unless the call only translates, the SH is the
        device's when the call rotates"""
        m = self.models[key]
        idx = m.kept(flt, invert)
        mode = T.mode(t, q, s)
        exact = _all(m.n)
        if mode != T.IDENTITY and idx.size:  # (gsx_api_transform.cpp returns before the drop for the identity and for an empty kept set)
            m.drop_vis("apply_transform")
            m.planes[0][idx] = T.position(m.planes[0][idx], t, q, s, pivot)
            if mode in (T.NO_ROTATION, T.FULL):
                exact[3][idx] = False
            if mode == T.FULL:
                exact[2][idx] = False
        return int(idx.size), exact

    def mask_evaluate(self, key, expr, shapes):
        m = self.models[key]
        if expr is None:
            m.mask = None
            return
        words = oracle.mask_evaluate(m.pos, *m.mt, *pack_program(MaskOp.parse(expr), shapes))
        m.mask = X.bits(words, m.n)

    def _select(self, m, hit, op):
        m.sel = P.apply_op(op, m.selection(), hit)
        return int(hit.sum()), int(m.sel.sum())

    def select_range(self, key, prop, lo, hi, op=0, flt=0, world=False):
        m = self.models[key]
        return self._select(m, P.hits(m.values(prop, world), m.passes(flt), lo, hi), op)

    def select_neighbors(self, key, r, lo, hi, op=0, flt=0):
        m = self.models[key]
        part = m.part(flt)
        return self._select(m, N.hits(N.brute(m.pos, part, r, cap=min(hi + 1, N.MAX_COUNT)), part, lo, hi), op)

    def select_clusters(self, key, r, mode, size_lo=0, size_hi=0, op=0, flt=0):
        m = self.models[key]
        c = CL.clusters(m.pos, m.part(flt), r)
        return self._select(m, CL.hits(c, mode, size_lo, size_hi, seeds=m.sel), op)

    def knn_scores(self, key, k, score, flt=0):
        m = self.models[key]
        part = m.part(flt)
        rows = memo(K.brute, m.pos, part, k)
        return part, rows, K.score(rows, score)

    def select_knn(self, key, k, score, lo=0.0, hi=0.0, std_ratio=None, op=0, flt=0, threshold=None):
        """threshold: the one the device returned (tests/test_gpu_knn.py: it may sit one unit in the last place from the
        restatement's, and a score is never compared with a threshold that differs); None: the restatement's"""
        m = self.models[key]
        part, _, s = self.knn_scores(key, k, score, flt)
        if std_ratio is None:
            hit = K.hit(s, part, K.SELECT_RANGE, lo, hi)
        elif threshold is None:
            hit = K.hit(s, part, K.SELECT_OUTLIERS, std_ratio=std_ratio)
        else:
            hit = part & (s > F(threshold)) if np.isfinite(s[part]).any() else np.zeros(m.n, bool)
        return self._select(m, hit, op)

    def vis_values(self, key, measure):
        """float64: the adopted planes as gsx_model_select_visibility compares them (the weight in units of 1, exact)"""
        v = self.models[key].vis
        return (v["peak"].astype(np.float64), v["weight"].astype(np.float64) / 2.0 ** 24, v["pixels"].astype(np.float64))[measure]

    def select_visibility(self, key, measure, lo, hi, op=0, flt=0):
        """gsx_model_select_visibility over the adopted planes: lo <= x <= hi among the Gaussians the filter passes"""
        m = self.models[key]
        x = self.vis_values(key, measure)
        return self._select(m, m.passes(flt) & (x >= lo) & (x <= hi), op)

    def decimate(self, src, dst, cell, flt=0, invert=False, driver=None):
        """gsx_model_decimate.  Returns (stats, map, exact rows of dst's planes): stats = (count, n_nonfinite, cells, singletons,
        largest_cell) and the map are decimate_ref.assign's over the kept set; dst holds one row per cell in ascending order of the
        cell's representative (its smallest index).  A one-member cell's row is src's stored row, exact in every plane.  A merged
        cell's row is `driver`'s float32 row (tests/decimate_driver.cpp played on src's planes), which the device quantises once in
        src's kind: known where the kind stores float32; without a driver it is the representative's row and unknown in every plane.
        0 cells create nothing."""
        s = self.models[src]
        kept = np.zeros(s.n, bool)
        kept[s.kept(flt, invert)] = True
        dmap, count, nonfinite, members = D.assign(s.pos, kept, cell)
        cells = int(members.size)
        stats = (count, nonfinite, cells, int((members == 1).sum()), int(members.max()) if cells else 0)
        if cells == 0:
            return stats, dmap, None
        idx = np.nonzero(dmap != D.NO_CELL)[0]
        rep = np.full(cells, s.n, np.int64)
        np.minimum.at(rep, dmap[idx].astype(np.int64), idx)
        rows, merged = _rows(s.planes, rep), members > 1
        if driver is not None:
            want = D.play(driver, s.planes, kept, cell)
            assert (want["count"], want["n_nonfinite"], want["cells"], want["singletons"], want["largest_cell"]) == stats and np.array_equal(want["map"], dmap)
            for mine, theirs in zip(rows, want["planes"]):
                assert mine[~merged].tobytes() == np.ascontiguousarray(theirs[~merged]).tobytes()  # (copied, not computed)
                mine[merged] = theirs[merged]
        d = self.add(dst, s.kind, rows, s.mt)
        known = [True, True, s.kind[0] == 0, s.kind[1] == 0] if driver is not None else [False] * 4
        return stats, dmap, [~merged | np.full(d.n, k) for k in known]

    def nearest(self, src, dst, src_filter=0, dst_filter=0, xform=None, model_transforms=False, max_distance=0.0):
        """gsx_model_nearest restated: nearest_ref's participants and `brute` (remembered: a draw and its op ask the same) over the
        two shadow models, under `xform` (the matrix a device returned, or None: nearest_ref.model_matrix of the two model
        transforms, or the identity).  Both selections are read as they are now."""
        s, t = self.models[src], self.models[dst]
        if xform is None:
            xform = R.model_matrix(s.mt, t.mt) if model_transforms else IDENTITY34
        xform = np.ascontiguousarray(xform, F).reshape(3, 4)
        q, q_part, q_bad = R.query_participates(xform, s.pos, s.passes(src_filter))
        t_pass = t.passes(dst_filter)
        t_part = N.participates(t.pos, t_pass)
        index, d2 = memo(R.brute, q, q_part, t.pos, t_part, float(max_distance))
        return dict(xform=xform, q=q, index=index, d2=d2, q_part=q_part, count=int(q_part.sum()), n_nonfinite=int(q_bad.sum()), t_part=t_part,
                    targets=int(t_part.sum()), targets_nonfinite=int((t_pass & ~t_part).sum()), **R.stats(index, d2))

    def select_nearest(self, src, dst, transfer=False, lo=0.0, hi=0.0, op=0, src_filter=0, dst_filter=0, xform=None, model_transforms=False,
                       max_distance=0.0):
        """gsx_model_select_nearest: writes the SOURCE's selection.  GSX_BOUNDS_SELECTED on either side and the transfer read the
        selections as they are before the call, also where src is dst"""
        s, t = self.models[src], self.models[dst]
        before = None if t.sel is None else t.sel.copy()
        ref = self.nearest(src, dst, src_filter, dst_filter, xform, model_transforms, max_distance)
        hit = R.hit(ref["index"], ref["d2"], ref["q_part"], R.SELECT_TRANSFER if transfer else R.SELECT_RANGE, lo, hi, before)
        return self._select(s, hit, op)

    def align(self, src, dst, xform, with_scale=False, src_filter=0, dst_filter=0, max_distance=0.0):
        """gsx_model_align_step restated: the pairs of `nearest`, nearest_ref.align_sums and align_solve.  `tol` is
        tests/test_gpu_nearest.py's bound on quaternion, scale and pos, from the reference's own Horn matrix; `degenerate` is spec
        §23's: fewer than 3 pairs, no spread among the queries, or an eigenvalue gap at or below 1e-9 of the matrix's norm"""
        ref = self.nearest(src, dst, src_filter, dst_filter, xform, False, max_distance)
        found = ref["index"] != R.NONE
        sums = R.align_sums(ref["q"][found], self.models[dst].pos[ref["index"][found]])
        n = sums["n"]
        Nm = R.horn_matrix(sums["H"])
        w = np.linalg.eigvalsh(Nm)
        norm, gap = float(np.linalg.norm(Nm)), float(w[-1] - w[-2])
        degenerate = n < 3 or sums["spread_q"] == 0 or gap <= 1e-9 * norm
        out = dict(nearest=ref, n_pairs=n, degenerate=degenerate, norm=norm, gap=gap, tol=np.inf, angle=0.0,
                   rms_before=float(np.sqrt(ref["d2"][found].astype(np.float64).sum() / n)) if n else 0.0)
        if not degenerate:
            want = R.align_solve(sums, with_scale)
            out.update(want, tol=10 * (2 * n * 2.0 ** -53) * norm / gap, angle=float(np.degrees(2 * np.arccos(min(1.0, want["quat"][3])))))
        return out


def unmet_views(views, selects, refusals, depth_maps):
    """conditions (i) to (m) of tests/test_gpu_model_fuzz.py over a seed set: the sessions' `vis_views`, `vis_selects`, `vis_refusals`
    and `depth_maps` records, which depend on the draws alone (what is resident, not what the planes hold)"""
    out = []
    ran = [r for r in views if not r["refused"]]
    if not any(r["views"] >= 2 and r["other_view"] for r in ran):
        out.append("(i) no vis_view accumulated onto planes taken at another pose or viewport")
    if not any(r["dressed"] for r in ran):
        out.append("(i) no vis_view of a model with a mask and stored edits")
    if not any(r["kind_differs"] for r in ran):
        out.append("(i) no vis_view of a model whose kind is not the seed's start kind")
    if set(DROPPERS) - set(refusals):
        out.append(f"(j) select_visibility was not refused for dropped planes after each of {DROPPERS}: {sorted(set(refusals))}")
    if not any(not r["refused"] and r["survived"] >= {"mask", "sel", "edit"} for r in selects):
        out.append("(j) no select_visibility on planes that survived a mask, a selection and an edit change")
    walked = [r for r in depth_maps if not r["refused"]]
    if not any(r["n_keys"] >= 3 for r in walked):
        out.append("(k) no depth_map walked three models or more")
    if not any(r["hidden_out"] for r in walked):
        out.append("(k) no depth_map with a hidden model left out")
    if not any(tuple(r["size"]) in PARTIAL_OR_LARGE for r in walked):
        out.append("(k) no depth_map at 83 x 51 or 320 x 240")
    out += [f"(k) no depth_map with the threshold {t}" for t in THRESHOLDS if not any(r["threshold"] == t for r in walked)]
    if not any(r["as_depth_buffer"] and r["lanes"] > 1 and r["frames"] >= 2 for r in walked):
        out.append("(k) no ndc plane was the depth buffer of two frames or more on a seed with several lanes")
    if not any(r["size_changed_after"] for r in walked):
        out.append("(k) no depth_map was followed by a viewport of another size (which drops it)")
    if not any(not r["ndc"] for r in walked):
        out.append("(k) no depth_map without the ndc plane")
    for name, recs in (("vis_view", views), ("depth_map", depth_maps)):
        if not any(r["refused"] for r in recs) or sum(not r["refused"] for r in recs) < 2:
            out.append(f"(l) {name} was not refused once and run twice: {[r['refused'] for r in recs]}")
        if not any(r["refused"] and r["resident"] for r in recs):
            out.append(f"(l) no {name} was refused with {'planes' if name == 'vis_view' else 'a map of the same viewport'} resident")
    for name, recs in (("vis_view", views), ("depth_map", depth_maps), ("select_visibility", selects)):
        if not any(r["inflight"] and not r["refused"] for r in recs):
            out.append(f"(m) {name} never ran with two frames enqueued and not waited for")
    return out


def unmet(cases, decimates, vis=None):
    """conditions (e), (f) and (h) of tests/test_gpu_model_fuzz.py over a seed set, stated once: `cases` is the union of the
    sessions' `cases`, `decimates` all their `decimates` records; with `vis` (dict(views, selects, refusals, depth_maps): the
    sessions' records of the visibility and depth map calls) also (i) to (m), unmet_views.  Returns what is not met."""
    out = [] if vis is None else unmet_views(vis["views"], vis["selects"], vis["refusals"], vis["depth_maps"])
    if not any(d["filtered"] for d in decimates):
        out.append("(e) no decimate of a source with a mask or selection filter in force")
    if not any(d["kind_differs"] for d in decimates):
        out.append("(e) no decimate of a source whose kind is not the seed's start kind")
    for d in decimates:
        if not (MIN_N <= d["cells"] < d["count"] and 0 < d["singletons"] < d["cells"]):
            out.append(f"(e) a decimate without both merged cells and singletons, or below MIN_N: {d}")
    if not any(d["largest_cell"] >= 3 for d in decimates):
        out.append("(e) no decimate with a cell of three or more members")
    out += [f"(f) no nearest-family call with {c}" for c in NEAREST_CASES if c not in cases]
    if "align:rotation" not in cases:
        out.append("(h) no align draw that is not degenerate with a reference rotation above 1 degree")
    return out


# ---- the schedule -------------------------------------------------------------------------------------------------------------------
def plan(seed):
    """the op kinds of a seed, in order: every kind but the plain camera step once in a seeded order, then EXTRA_OPS random ones; a run
    of POST_OP_RUN camera steps after every op that changes a model and none or one after the others: somewhat over half of all steps"""
    rng = np.random.default_rng(9000 + seed)
    walk = [k for k in OP_KINDS if k != "cam_step"]
    rng.shuffle(walk)
    walk += [walk[int(i)] for i in rng.integers(0, len(walk), EXTRA_OPS)]
    out = ["cam_step"]
    for k in walk:
        out.append(k)
        out += ["cam_step"] * (POST_OP_RUN if k in MODEL_CHANGING else int(rng.integers(0, 2)))
    return out


@dataclasses.dataclass
class View:
    pose: int = 0
    size: tuple = (W, H)
    mode: int = 0
    gsize: float = 1.0
    deg: int = 3
    depth: bool = False
    lines: bool = False
    gizmos: bool = False
    sel_edit_on: bool = False
    hidden: set = dataclasses.field(default_factory=set)
    rect: dict | None = None  # this step's rectangle query


def _plain(v):
    if isinstance(v, np.ndarray):
        return [_plain(x) for x in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, float):
        return float(np.format_float_positional(v, unique=True))
    return v


class Session:
    """One seed: the shadow, the view state both viewers are given, the random stream and the log of ops drawn so far."""

    def __init__(self, seed, driver=None):
        self.seed = seed
        self.driver = driver           # tests/decimate_driver.cpp, built (decimate_ref.build_driver): the merged rows of a decimate
        self.cases: set = set()        # NEAREST_CASES and "align:rotation" as the draws met them (conditions (f) and (h))
        self.decimates: list = []      # a record per decimate (condition (e))
        self.vis_views: list = []      # a record per vis_view, per select_visibility and per depth_map (conditions (i) to (m)); the
        self.vis_selects: list = []    # dropping calls after which a select_visibility was refused for planes that had been resident
        self.vis_refusals: list = []
        self.depth_maps: list = []
        self.depth_map = None          # gsx_viewer::depth_map: None, or dict(size, ndc, planes: the device's, adopted)
        self._ndc_buffer = None        # the depth_maps record whose ndc plane is the depth buffer now
        self.parent: dict = {}         # key -> the model it was extracted, converted or decimated from
        self.rng = np.random.default_rng(7000 + seed)
        self.lanes, self.host_verify = 1 + seed % 3, seed % 3
        self.kind = START_KINDS[seed % len(START_KINDS)]
        self.shadow, self.view, self.log, self.counter = Shadow(), View(), [], 0
        self.shapes = mask_shapes()
        self.nontrivial: set = set()   # SELECT_VARIANTS with a hit set neither empty nor full
        self.ran: dict = {}            # op kind -> times
        self.view.pose = int(self.rng.integers(0, 240))
        self.start = []                # (key, n, scene seed, transform)
        for i in range(2 + seed % 2):
            self.start.append((f"m{i}", int(self.rng.integers(1500, 4001)), 500 + 10 * seed + i, self._random_mt()))

    def scene(self, n, scene_seed):
        return common.small_scene(n, scene_seed)

    def load_start(self, dev=None):
        for key, n, scene_seed, mt in self.start:
            g = self.scene(n, scene_seed)
            self.shadow.add(key, self.kind, oracle.convert(g), mt)
            if dev is not None:
                dev.new_model(key, g, mt)
                self._take_upload(key, dev)

    def _take_upload(self, key, dev):
        """a fresh upload: position and colour are oracle.convert's; covariance and SH are the device's (quantised in its kind)"""
        m = self.shadow.models[key]
        got = dev.pod_live(key)
        single = [np.full(m.n, True), np.full(m.n, True), np.full(m.n, m.kind[0] == 0), np.full(m.n, m.kind[1] == 0)]
        self.shadow.verify(key, got, single, "upload")
        self.shadow.adopt(key, got)
        dev.rebuild([], [key])
        self.shadow.verify(key, dev.pod_rebuilt(key), _all(m.n), "rebuilt from the shadow")

    def _random_mt(self):
        rng = self.rng
        from wgpu_3dgs_viewer_app_amd import camera

        mt = camera.ModelTransform(pos=rng.uniform(-1.0, 1.0, 3).astype(F), rot=rng.uniform(-40, 40, 3).astype(F), scale=rng.uniform(0.7, 1.3, 3).astype(F))
        return (np.asarray(mt.pos, F), np.asarray(mt.quat(), F), np.asarray(mt.scale, F))

    # ---- drawing ----
    def keys(self):
        return sorted(self.shadow.models)

    def _new_key(self):
        self.counter += 1
        return f"k{self.counter}"

    def _evict(self, involved, room=1):
        """keys to remove first so that `room` more models fit under MAX_MODELS"""
        spare = [k for k in self.keys() if k not in involved]
        out = []
        while len(self.keys()) - len(out) + room > MAX_MODELS and spare:
            out.append(spare.pop(int(self.rng.integers(len(spare)))))
        return out

    def _filter(self, m, allow_selected=True, invertible=False):
        """a filter that keeps at least MIN_N Gaussians of the model as the shadow has it"""
        rng = self.rng
        flt, invert = int(FILTERS[int(rng.integers(len(FILTERS)))]), bool(rng.random() < 0.3) and invertible
        if not allow_selected:
            flt &= ~X.SELECTED
        if m.kept(flt, invert).size < MIN_N:
            flt, invert = 0, False
        return flt, invert

    def _radius(self, m, k, mul):
        """a multiple of knn_ref.kth_distance_median on the shadow; of the next k while it is 0 (a model merged with itself holds
        every position twice)"""
        r = 0.0
        while r <= 0.0:
            r, k = float(F(mul * memo(K.kth_distance_median, m.pos, m.part(0), k))), k + 1
        return r

    def _with_planes(self, kind, key):
        """a pod kind change and a new upload go to a model that holds visibility planes, where there is one; where there is none the
        op's `view_first` gives the drawn model some: the call must drop them (condition (j))"""
        have = [k for k in self.keys() if self.shadow.models[k].vis is not None]
        if have:
            key = have[0]
        return key, self.shadow.models[key]

    def _kept_bits(self, m, flt, invert):
        out = np.zeros(m.n, bool)
        out[m.kept(flt, invert)] = True
        return out

    def _target(self, m, flt, invert):
        """a cell count for gsx_model_decimate_edge: within [max(MIN_N, kept / 4), kept / 2], or the lower end where that is empty"""
        k = int(m.kept(flt, invert).size)
        lo = max(MIN_N, k // 4)
        return int(self.rng.integers(lo, max(lo, k // 2) + 1))

    def _decimate_cell(self, m, flt, invert):
        """(cell, flt, invert, the cells' member counts) of a decimate that leaves at least MIN_N cells: the edge
        decimate_ref.find_edge gives for a drawn target; where that leaves fewer (the count is not monotone in the edge) the median
        nearest-neighbour distance; where that does too, the same without a filter; None where no edge does"""
        for f, inv in ((flt, invert), (0, False)):
            kept = self._kept_bits(m, f, inv)
            edge, cells = memo(D.find_edge, m.pos, kept, self._target(m, f, inv))
            if cells < MIN_N:
                edge = F(self._radius(m, 1, 1.0))
            members = D.assign(m.pos, kept, float(edge))[3]
            if members.size >= MIN_N:
                return float(edge), f, inv, members
        return None

    def _descends(self, key, ancestor):
        while key in self.parent:
            key = self.parent[key]
            if key == ancestor:
                return True
        return False

    def _target_key(self, key, same=0.3, prefer_descendant=False):
        """the target model of a nearest-family call from `key`: another model of at most SPATIAL_N, or `key` itself with probability
        `same` and where there is no other"""
        sh = self.shadow
        others = [k for k in self.keys() if k != key and sh.models[k].n <= SPATIAL_N]
        if not others or self.rng.random() < same:
            return key
        if prefer_descendant and any(self._descends(k, key) for k in others):
            others = [k for k in others if self._descends(k, key)]
        return others[int(self.rng.integers(len(others)))]

    def _rigid(self, max_deg, max_shift, centre=ZERO3, scale=1.0, min_deg=0.0):
        """float32[3, 4]: a rotation by min_deg .. max_deg about a random axis through `centre`, scaled about it, then a shift of at
        most max_shift"""
        rng = self.rng
        axis, shift = rng.normal(size=3), rng.normal(size=3)
        half = np.radians(rng.uniform(min_deg, max_deg)) / 2
        A = scale * R.quat_rows(np.concatenate([axis / np.linalg.norm(axis) * np.sin(half), [np.cos(half)]]))
        c = np.asarray(centre, np.float64)
        b = c - A @ c + shift / np.linalg.norm(shift) * rng.uniform(0, max_shift)
        return np.concatenate([A, b[:, None]], axis=1).astype(F)

    def _nearest_args(self, key, dst, n_of):
        """the parameters the nearest-family calls share, alternated on `n_of` so that the seed set meets condition (f): the mapping
        (src != dst: the model transforms, a drawn similarity, the identity; src == dst: the identity), the two filters (src == dst
        with a mask and a selection: one against the other) and, every other time, a max_distance: the power-of-two multiple of the
        targets' median nearest-neighbour distance nearest to the queries' median distance within which some but not all find a target"""
        sh, rng = self.shadow, self.rng
        s, t = sh.models[key], sh.models[dst]
        a = dict(dst=dst, model_transforms=False, xform=None, src_filter=self._filter(s)[0], dst_filter=self._filter(t)[0], max_distance=0.0)
        if key != dst:
            how = n_of % 3
            if how == 0:
                a.update(model_transforms=True)
            elif how == 1:
                a.update(xform=self._rigid(40.0, 0.5, scale=float(rng.uniform(0.8, 1.25))))
        elif s.mask is not None and s.sel is not None:
            fs, fd = (X.SELECTED, X.MASKED) if n_of % 2 else (X.MASKED, X.SELECTED)
            if min(s.kept(fs).size, s.kept(fd).size) >= MIN_N:
                a.update(src_filter=fs, dst_filter=fd)
        ref = sh.nearest(key, dst, a["src_filter"], a["dst_filter"], a["xform"], a["model_transforms"])
        if (n_of // 3) % 2 == 0 and ref["n_found"]:
            d2 = ref["d2"][ref["index"] != R.NONE]
            r = self._radius(t, 1, 1.0)
            reach = [float(F(r * 2.0 ** k)) for k in range(-6, 9)]
            some = [md for md in reach if 0 < int((d2 <= R.cap2(md)).sum()) < ref["count"]]
            if some:
                mid = max(float(np.sqrt(np.median(d2))), min(some))
                a.update(max_distance=min(some, key=lambda md: abs(np.log(md / mid))))
                ref = sh.nearest(key, dst, a["src_filter"], a["dst_filter"], a["xform"], a["model_transforms"], a["max_distance"])
                self.cases.add("nearest:max_distance")
        if key != dst and a["model_transforms"]:
            self.cases.add("nearest:model_transforms")
        if key != dst and s.kind != t.kind:
            self.cases.add("nearest:kinds")
        if key == dst and a["src_filter"] != a["dst_filter"] and (ref["q_part"] & ~ref["t_part"]).any():
            self.cases.add("nearest:same_disjoint")
        return a, ref

    def _align_args(self, key):
        """dst, a small rigid `xform` about the targets' centre (at most 5 degrees, a shift of at most half their median
        nearest-neighbour distance), with_scale and the filters of an align step, drawn again (then from the model onto itself, without
        filters) while the reference's tolerance formula exceeds ALIGN_TOL_MAX"""
        sh, rng = self.shadow, self.rng
        for attempt in range(4):
            dst = self._target_key(key, prefer_descendant=True) if attempt < 2 else key
            s, t = sh.models[key], sh.models[dst]
            fs, fd = (self._filter(s)[0], self._filter(t)[0]) if attempt < 2 else (0, 0)
            centre = B.reference(t.pos, t.passes(fd))["center"]
            a = dict(dst=dst, xform=self._rigid(5.0, 0.5 * self._radius(t, 1, 1.0), centre, min_deg=0.5), with_scale=bool(rng.random() < 0.5),
                     src_filter=fs, dst_filter=fd, max_distance=0.0)
            ref = sh.align(key, a["dst"], a["xform"], a["with_scale"], fs, fd)
            if ref["degenerate"] or ref["tol"] <= ALIGN_TOL_MAX:
                break
        if not ref["degenerate"] and ref["angle"] > 1.0:
            self.cases.add("align:rotation")
        return a

    def draw(self, kind):
        rng, sh, v = self.rng, self.shadow, self.view
        keys = self.keys()
        key = keys[int(rng.integers(len(keys)))]
        if kind in SPATIAL:  # the n^2 restatements are most of a seed's time: a model of at most SPATIAL_N when there is one, or the smallest
            small = [k for k in keys if sh.models[k].n <= SPATIAL_N]
            key = small[int(rng.integers(len(small)))] if small else min(keys, key=lambda k: sh.models[k].n)
        m = sh.models[key]
        op = {"kind": kind}
        inflight = 2 if self.lanes > 1 else 0
        if kind == "cam_jump":
            op.update(pose=int(rng.integers(0, 240)))
        elif kind == "viewport":
            i = int(rng.integers(len(VIEWPORTS)))
            if self.depth_map is not None and tuple(VIEWPORTS[i]) == tuple(v.size):  # another size: the change drops the depth map
                i = (i + 1) % len(VIEWPORTS)
            op.update(size=VIEWPORTS[i])
        elif kind == "visibility":
            hidden = [k for k in keys if rng.random() < 0.3]
            op.update(hidden=hidden if len(hidden) < len(keys) else hidden[1:])
        elif kind == "display":
            op.update(mode=int(rng.integers(0, 3)), gsize=float(rng.choice([0.6, 1.0, 1.5])), deg=int(rng.integers(0, 4)))
        elif kind == "model_transform":
            op.update(key=key, mt=self._random_mt())
        elif kind == "mask_eval":
            op.update(key=key, expr=MASK_EXPRS[int(rng.integers(len(MASK_EXPRS)))])
        elif kind == "sel_upload":
            op.update(key=key, rseed=int(rng.integers(1 << 30)), density=None if rng.random() >= 0.8 else float(rng.choice([0.1, 0.5])))
        elif kind == "sel_edit":
            op.update(flag=int(rng.choice([0, 1, 3, 5])), color=rng.uniform(0, 1, 3), contrast=float(rng.uniform(-0.3, 0.3)), exposure=float(rng.uniform(-1, 1)),
                      gamma=float(rng.uniform(0.5, 2.0)), alpha=float(rng.uniform(0.3, 1.5)), highlight=float(rng.choice([0.0, 0.4])))
        elif kind == "edits_upload":
            op.update(key=key, rseed=int(rng.integers(1 << 30)) if rng.random() < 0.7 else None)
        elif kind == "unedited":
            op.update(key=key, on=not m.unedited)
        elif kind == "rect_query":
            x0, y0 = float(rng.uniform(0, v.size[0] * 0.5)), float(rng.uniform(0, v.size[1] * 0.5))
            op.update(p0=(x0, y0), p1=(x0 + float(rng.uniform(10, v.size[0] * 0.5)), y0 + float(rng.uniform(10, v.size[1] * 0.5))), op=int(rng.integers(0, 3)))
        elif kind in VIEW_CALLS or kind == "select_visibility":
            # Steered by n_of (the seed plus the times the kind ran) so that the seed set meets conditions (i) to (m) whatever the
            # walk's order; every random number is drawn whether or not it is used, so that the stream does not depend on the state.
            n_of = self.ran.get(kind, 0) + self.seed
            coin, coin2, pick, pose = float(rng.random()), float(rng.random()), int(rng.integers(1 << 30)), int(rng.integers(0, 240))
            flying = inflight if (n_of // 2) % 2 == 0 or coin2 < 0.5 else 0
            feature = FEATURES[int(rng.integers(len(FEATURES)))]
            touch = dict(expr=MASK_EXPRS[1 + int(rng.integers(len(MASK_EXPRS) - 1))], sel=int(rng.integers(1 << 30)), edits=int(rng.integers(1 << 30)))
            # the step's frame of a vis_view or depth_map carries a rectangle query, as fractions of the viewport the call runs at.  The
            # device adaptor hands it to `live` BEFORE the call and not again: the call switches the query off for its own frame and
            # must put it back
            rect = [float(x) for x in (rng.uniform(0, 0.5), rng.uniform(0, 0.5), rng.uniform(0.1, 0.5), rng.uniform(0.1, 0.5))] + [int(rng.integers(0, 3))]
            if kind == "vis_view":
                # every fourth is refused (no clear; where nothing is on, `feature` is switched on first).  Every other one accumulates:
                # onto the planes the model has, or onto a first view taken at `prime`, another pose.  The model: one with a mask
                # and stored edits, or one of another kind than the seed's first, where there is one
                dressed = [k for k in keys if sh.models[k].mask is not None and sh.models[k].edits is not None]
                other = [k for k in keys if sh.models[k].kind != self.kind]
                prefer = (dressed or other) if (n_of // 2) % 2 == 0 else (other or dressed)
                accumulate = n_of % 2 == 0
                op.update(key=prefer[pick % len(prefer)] if prefer else key, accumulate=accumulate, prime=(pose if pose != v.pose else (pose + 1) % 240) if accumulate else None,
                          clear=n_of % 4 != 1 and coin < 0.9, feature=feature, rect=rect, inflight=flying)
            elif kind == "depth_map":
                # every third is refused; the thresholds in turn; every other one hands its ndc plane to the depth test;
                # every fourth hides one more model first, every fourth moves to a viewport with partial tiles or of 300 tiles first
                ndc = n_of % 4 != 3  # (every fourth without the ndc plane)
                op.update(threshold=THRESHOLDS[(n_of // 3) % 3], ndc=ndc, as_depth_buffer=ndc and n_of % 2 == 0, clear=n_of % 3 != 0 and coin < 0.9, feature=feature,
                          hide=pick if n_of % 4 == 1 else None, size=PARTIAL_OR_LARGE[(n_of // 4) % 2] if n_of % 4 == 2 else None, rect=rect, inflight=flying)
            else:
                # every fourth as the session stands, on a model whose planes were dropped where there is one: refused without planes.
                # The others on a model with planes (those that survived most first); a model without gets a view first (`view`), and
                # every other one a mask, a selection and an edit change between the view and the select (`touch`).  The range:
                # two quantiles of the positive values, every fourth the Gaussians never seen
                as_is = n_of % 4 == 1
                have = sorted((k for k in keys if sh.models[k].vis is not None), key=lambda k: -len(sh.models[k].vis["survived"]))
                lost = [k for k in keys if sh.models[k].vis is None and sh.models[k].vis_lost]
                bare = [k for k in keys if sh.models[k].vis is None]
                if as_is:
                    pool = lost or bare or keys
                    key = pool[pick % len(pool)]
                elif have:
                    key = have[0]
                q = (None, None) if n_of % 4 == 3 else VIS_QUANTILES
                op.update(key=key, measure=n_of % 3, op=int(rng.integers(0, 3)), flt=self._filter(sh.models[key], False)[0], q_lo=q[0], q_hi=q[1], view=not as_is,
                          touch=touch if n_of % 2 == 0 else None, inflight=flying)
        elif kind in SELECTS:
            op.update(key=key, op=int(rng.integers(0, 3)), flt=self._filter(m, False)[0], inflight=inflight if rng.random() < 0.5 else 0)
            n_of = self.ran.get(kind, 0) + self.seed
            if kind == "select_range":
                world = bool(n_of % 2)
                prop = int([P.POS_X, P.POS_Y, P.POS_Z, P.RED, P.BLUE, P.HUE, P.VALUE][int(rng.integers(7))]) if not world else int(rng.integers(0, 3))
                vals = m.values(prop, world)
                lo, hi = np.quantile(vals[P.finite(vals)], [0.25, 0.6]).astype(F)
                op.update(prop=prop, world=world, lo=float(lo), hi=float(hi))
            elif kind == "select_neighbors":
                op.update(r=self._radius(m, 1, 1.0), lo=0, hi=0)
            elif kind == "select_clusters":
                mode = n_of % 3
                by_size = int(mode == CL.BY_SIZE)  # (the sizes [1, 1]: the Gaussians with no other within r; 0 in the other modes)
                op.update(mode=mode, r=self._radius(m, 1, 1.0 if mode != CL.LARGEST else 1.5), size_lo=by_size, size_hi=by_size)
                if mode == CL.SEEDED and not m.selection().any():
                    op.update(seeds=int(rng.integers(1 << 30)))  # a model without a selection gets a sparse one first
            elif kind == "select_nearest":
                transfer = bool(n_of % 2)
                a, ref = self._nearest_args(key, self._target_key(key), n_of // 2)
                op.update(a, flt=a["src_filter"], transfer=transfer, lo=0.0, hi=0.0)
                del op["src_filter"]
                if not transfer:
                    d = np.sqrt(ref["d2"][ref["index"] != R.NONE])
                    lo, hi = np.quantile(d, [0.25, 0.6]).astype(F) if d.size else (F(0), F(0))
                    op.update(lo=float(lo), hi=float(hi))
                elif not sh.models[op["dst"]].selection().any():
                    op.update(dst_seeds=int(rng.integers(1 << 30)))  # a target model without a selection gets one first
            else:
                part, _, s = sh.knn_scores(key, 3, K.SCORE_KTH, op["flt"])
                outliers = bool(n_of % 2)  # (score above mean + std_ratio * std; the range is then not looked at and must be 0)
                op.update(k=3, score=K.SCORE_KTH, lo=0.0, hi=0.0 if outliers else float(np.median(s[part & np.isfinite(s)])), std_ratio=1.0 if outliers else None)
        elif kind in READ_ONLY:
            flt, invert = self._filter(m, invertible=kind in ("export", "export_ply", "decimate_edge"))
            op.update(key=key, flt=flt, inflight=inflight if rng.random() < 0.5 else 0)
            if kind == "bounds":
                op.update(trim=int(rng.choice([0, 50])))
            elif kind == "histogram":
                world = bool(rng.random() < 0.5)  # (WORLD is for the positions)
                op.update(prop=int(rng.integers(0, 3 if world else 10)), bins=int(rng.choice([1, 64, 255])), world=world, auto=bool(rng.random() < 0.5))
            elif kind == "property_values":
                world = bool(rng.random() < 0.5)
                op.update(prop=int(rng.integers(0, 3 if world else 10)), world=world)
            elif kind in ("neighbors", "clusters"):
                op.update(r=self._radius(m, 2, 1.0))
            elif kind == "knn":
                op.update(k=int(rng.choice([1, 3, 8])), score=int(rng.integers(0, 2)))
            elif kind == "decimate_edge":
                op.update(invert=invert, target=self._target(m, flt, invert))
            elif kind == "nearest":
                a, _ = self._nearest_args(key, self._target_key(key), self.ran.get(kind, 0) + self.seed)
                op.update(a, flt=a["src_filter"])
                del op["src_filter"]
            elif kind == "align_step":
                a = self._align_args(key)
                op.update(a, flt=a["src_filter"])
                del op["src_filter"]
            else:
                op.update(invert=invert)
        elif kind in ("xf_translate", "xf_scale", "xf_full"):
            selected = bool(rng.random() < 0.5) and bool(m.selection().any())
            t = rng.uniform(-0.3, 0.3, 3).astype(F)
            q, s = IDENT, ONE3
            if kind == "xf_scale":
                t, s = ZERO3, rng.uniform(0.8, 1.25, 3).astype(F)
            elif kind == "xf_full":
                q = rng.normal(size=4)
                q = (q / np.linalg.norm(q)).astype(F)
                s = rng.uniform(0.8, 1.25, 3).astype(F)
                s[int(rng.integers(3))] *= F(-1)  # a reflection
            pivot = B.reference(m.pos, m.selection())["center"] if selected else ZERO3
            # every other one on a model that holds visibility planes (it gets a view first where it has none): the call drops them
            op.update(key=key, t=t, q=q, s=s, pivot=pivot, flt=X.SELECTED if selected else 0, view_first=(self.ran.get(kind, 0) + self.seed) % 2 == 0,
                      inflight=inflight)
        elif kind == "set_pod_kind":
            key, m = self._with_planes(kind, key)
            others = [k for k in KINDS if k != m.kind]
            op.update(key=key, to=others[int(rng.integers(len(others)))], view_first=True, inflight=inflight)
        elif kind in ("convert", "extract"):
            flt, invert = self._filter(m, invertible=True)
            op.update(key=key, dst=self._new_key(), flt=flt, invert=invert, drop_edits=bool(rng.random() < 0.3), evict=self._evict([key]),
                      remove_src=bool(rng.random() < 0.5), inflight=inflight)
            if kind == "convert":
                op.update(to=KINDS[int(rng.integers(len(KINDS)))])
            self.parent[op["dst"]] = key
        elif kind == "decimate":
            flt, invert = self._filter(m, invertible=True)
            if (self.ran.get(kind, 0) + self.seed) % 2 == 0:  # every other one: a model that has a mask or a selection, under that filter
                dressed = [(k, f) for k in keys for f, bits in ((X.MASKED, sh.models[k].mask), (X.SELECTED, sh.models[k].sel))
                           if bits is not None and sh.models[k].kept(f).size >= 2 * MIN_N]
                if dressed:
                    (key, flt), invert = dressed[int(rng.integers(len(dressed)))], False
                    m = sh.models[key]
            # condition (e) asks merged cells and singletons of EVERY decimate: a model that holds every position twice (merged with
            # itself) has no singleton under any edge, so another model is taken then, unfiltered
            first = None
            for k, f, inv in [(key, flt, invert)] + [(k, 0, False) for k in keys if k != key]:
                found = self._decimate_cell(sh.models[k], f, inv)
                if found is None:
                    continue
                first = first or (k,) + found[:3]
                if 0 < int((found[3] == 1).sum()) < found[3].size:
                    first = (k,) + found[:3]
                    break
            assert first is not None, "no cell edge leaves MIN_N cells"
            key, cell, flt, invert = first
            m = sh.models[key]
            op.update(key=key, dst=self._new_key(), cell=cell, flt=flt, invert=invert, evict=self._evict([key]), remove_src=bool(rng.random() < 0.5),
                      inflight=inflight)
            self.parent[op["dst"]] = key
        elif kind == "merge":
            other = [k for k in keys if k != key and sh.models[k].n + m.n <= MAX_N]
            srcs = [key, other[int(rng.integers(len(other)))]] if other else ([key, key] if 2 * m.n <= MAX_N else [key])
            op.update(srcs=srcs, dst=self._new_key(), evict=self._evict(srcs), remove_srcs=bool(rng.random() < 0.5), inflight=inflight)
            if sh.models[srcs[-1]].kind != m.kind:  # convert first when the kinds differ: the second source, into the first's kind
                op.update(via=self._new_key())
        elif kind == "ply_roundtrip":
            op.update(key=key, dst=self._new_key(), evict=self._evict([key]), inflight=inflight)
        elif kind == "remove_add":
            key, m = self._with_planes(kind, key)
            n = int(rng.integers(1500, 4001))
            op.update(key=key, n=n if n != m.n else n + 1, scene_seed=int(rng.integers(1000, 100000)), mt=self._random_mt(), view_first=True,
                      inflight=inflight)
        elif kind == "depth_test":
            op.update(on=not v.depth)
        elif kind == "hit_pairs":
            op.update(on=not v.lines)
        elif kind == "gizmos":
            op.update(on=not v.gizmos)
        self.log.append({k: _plain(x) for k, x in op.items()})
        self.ran[kind] = self.ran.get(kind, 0) + 1
        return op

    def replay(self):
        return f"seed {self.seed} step {len(self.log) - 1} ops {self.log}"

    # ---- applying ----
    def _touched(self, key, what):
        """a mask, selection ("sel") or edit change of a model: its visibility planes, where it has some, survive it"""
        m = self.shadow.models.get(key)
        if m is not None and m.vis is not None:
            m.vis["survived"].add(what)

    def apply(self, op, dev=None, sub=False):
        """apply a drawn op to the shadow and, with `dev`, to the device in lock-step.  Returns the keys whose model changed.  `sub`:
        a state op that another op switches first (a clear, a feature, a viewport, a touch): part of that op's step."""
        kind, sh, v = op["kind"], self.shadow, self.view
        dropped = False
        if not sub:
            v.rect = None
            if self._ndc_buffer is not None:  # the frame of the step before this one read the ndc plane as its depth buffer
                self._ndc_buffer["frames"] += 1
            # (an op that takes a view or changes state first enqueues its frames itself, right in front of its own call)
            if dev is not None and op.get("inflight") and kind != "select_visibility" and "view_first" not in op:
                dev.enqueue_frames(op["inflight"])
        if kind == "cam_step":
            v.pose = (v.pose + 1) % 240
        elif kind == "cam_jump":
            v.pose = op["pose"]
        elif kind == "viewport":
            if self.depth_map is not None and tuple(op["size"]) != self.depth_map["size"]:
                self.depth_map["rec"]["size_changed_after"] = dropped = True
                self.depth_map = None
            v.size = tuple(op["size"])
            if v.depth:
                self._ndc_buffer = None  # (the viewers get _depth(size))
        elif kind == "visibility":
            v.hidden = set(op["hidden"])
        elif kind == "display":
            v.mode, v.gsize, v.deg = op["mode"], op["gsize"], op["deg"]
        elif kind == "model_transform":
            sh.models[op["key"]].mt = tuple(np.array(a, F) for a in op["mt"])
        elif kind == "mask_eval":
            sh.mask_evaluate(op["key"], op["expr"], self.shapes)
            self._touched(op["key"], "mask")
        elif kind == "sel_upload":
            m = sh.models[op["key"]]
            m.sel = None if op["density"] is None else random_bits(m.n, op["rseed"], op["density"])
            self._touched(op["key"], "sel")
        elif kind == "sel_edit":
            v.sel_edit_on = bool(op["flag"] & 1)
        elif kind == "edits_upload":
            m = sh.models[op["key"]]
            m.edits = None if op["rseed"] is None else normalise_edits(random_edits(m.n, op["rseed"]))
            self._touched(op["key"], "edit")
        elif kind == "unedited":
            sh.models[op["key"]].unedited = op["on"]
        elif kind == "rect_query":
            v.rect = op
        elif kind == "depth_test":
            v.depth = op["on"]
            self._ndc_buffer = None  # (on: the viewers get _depth(size); off: nothing reads the plane)
        elif kind == "hit_pairs":
            v.lines = op["on"]
        elif kind == "gizmos":
            v.gizmos = op["on"]
        elif kind in SELECTS:
            self._apply_select(op, dev)
            return []
        elif kind in VIEW_CALLS:
            self._apply_view_call(op, dev)
            return []
        elif kind in READ_ONLY:
            if dev is not None:
                dev.read_only(op, sh)
            return []
        elif kind in MODEL_CHANGING:
            return self._apply_model_op(op, dev)
        if dev is not None:
            dev.state_op(op)
            if dropped:
                dev.depth_map_dropped()
        return []

    # ---- the calls that draw a model's own frame: gsx_model_visibility, gsx_render_depth_map ----
    def _features_off(self, dev):
        """the depth test, the lines and the gizmos that are on go off, on both viewers, through the ordinary state ops.  Returns
        their names."""
        v = self.view
        on = [name for name, flag in (("depth_test", v.depth), ("hit_pairs", v.lines), ("gizmos", v.gizmos)) if flag]
        for name in on:
            self.apply({"kind": name, "on": False}, dev, sub=True)
        return on

    def _features_on(self, dev, names):
        for name in names:
            self.apply({"kind": name, "on": True}, dev, sub=True)

    def _switch(self, dev, clear, feature):
        """`clear`: the features that are on go off.  Otherwise the call is to be refused: where nothing is on, `feature` goes on
        first.  Returns whether the call is refused."""
        v = self.view
        if clear:
            self._features_off(dev)
        elif not (v.depth or v.lines or v.gizmos):
            self._features_on(dev, [feature])
        return v.depth or v.lines or v.gizmos

    def _view_first(self, key, dev):
        """a model without visibility planes gets a view, with the features that are on switched off for it and on again after"""
        if self.shadow.models[key].vis is None:
            on = self._features_off(dev)
            self._view(key, self.view.pose, False, dev)
            self._features_on(dev, on)

    def _view(self, key, pose, accumulate, dev):
        """one gsx_model_visibility of `key` at `pose` that is not refused: the device's planes are verified by `dev` against the
        shadow's as they stand, then adopted.  Returns (views, whether it folded into planes taken at another pose or viewport)."""
        m = self.shadow.models[key]
        before, at = m.vis, (pose, tuple(self.view.size))
        folds = accumulate and before is not None
        planes = dict(peak=None, weight=None, pixels=None) if dev is None else dev.vis_view(key, pose, accumulate, m)
        m.vis = dict(planes, views=before["views"] + 1 if folds else 1, at=(before["at"] if folds else []) + [at], survived=before["survived"] if folds else set())
        m.vis_lost = None
        return m.vis["views"], bool(folds and any(a != at for a in before["at"]))

    def _apply_view_call(self, op, dev):
        kind, sh, v = op["kind"], self.shadow, self.view
        if kind == "depth_map":
            if op["size"] is not None and tuple(op["size"]) != tuple(v.size):
                self.apply({"kind": "viewport", "size": op["size"]}, dev, sub=True)
            shown = [k for k in self.keys() if k not in v.hidden]
            if op["hide"] is not None and len(shown) >= 2:
                v.hidden = v.hidden | {shown[op["hide"] % len(shown)]}
        flying = self.lanes > 1 and op["inflight"] >= 2
        (fx, fy, fw, fh, rop), (w, h) = op["rect"], v.size
        v.rect = dict(p0=(fx * w, fy * h), p1=((fx + fw) * w, (fy + fh) * h), op=rop)  # this step's query, in force across the call
        # A call that is to be refused must leave what is resident as it was, so something is: where the model holds no planes, or
        # the viewer no depth map of this viewport, an unrefused call of the same kind comes first (`primed`), with the features that
        # are on switched off for it and on again after.  (The frames in flight are then in front of that call.)
        resident = sh.models[op["key"]].vis is not None if kind == "vis_view" else self.depth_map is not None
        primed = not op["clear"] and not resident
        if primed:
            on = self._features_off(dev)
            if kind == "vis_view":
                self._view(op["key"], v.pose, False, dev)
            else:
                self._depth_map(dict(op, as_depth_buffer=False), dict(size_changed_after=False), dev)
            self._features_on(dev, on)
        refused = self._switch(dev, op["clear"], op["feature"])
        if kind == "vis_view":
            key = op["key"]
            m = sh.models[key]
            rec = dict(refused=refused, resident=m.vis is not None, primed=primed, views=0, other_view=False, dressed=m.mask is not None and m.edits is not None,
                       kind_differs=m.kind != self.kind, inflight=flying and not primed)
            if refused:
                if dev is not None:
                    dev.vis_refused(key, m)
            else:
                if op["accumulate"] and m.vis is None:  # nothing to accumulate onto: a first view from elsewhere
                    self._view(key, op["prime"], False, dev)
                rec["views"], rec["other_view"] = self._view(key, v.pose, op["accumulate"], dev)
            self.vis_views.append(rec)
            return
        alive = self.keys()
        shown = [k for k in alive if k not in v.hidden] or alive  # (Device._order: the step's painter's order is of these)
        rec = dict(refused=refused, resident=self.depth_map is not None, primed=primed, n_keys=len(shown), hidden_out=len(shown) < len(alive), size=tuple(v.size),
                   threshold=op["threshold"], ndc=op["ndc"], as_depth_buffer=False, lanes=self.lanes, frames=0, size_changed_after=False,
                   inflight=flying and not primed)
        if refused:
            if dev is not None:
                dev.depth_map_refused(self.depth_map)
        else:
            self._depth_map(op, rec, dev)
        self.depth_maps.append(rec)

    def _depth_map(self, op, rec, dev):
        """one gsx_render_depth_map that is not refused: the device's planes are verified by `dev`, then adopted"""
        v = self.view
        planes = None if dev is None else dev.depth_map(op, self.shadow)
        self.depth_map = dict(size=tuple(v.size), ndc=op["ndc"], planes=planes, rec=rec)
        if op["as_depth_buffer"]:  # (dev.depth_map switched the depth test on, against the ndc plane)
            v.depth, rec["as_depth_buffer"], self._ndc_buffer = True, True, rec

    def _apply_select(self, op, dev):
        kind, key, sh = op["kind"], op["key"], self.shadow
        m = sh.models[key]
        a = dict(op=op["op"], flt=op["flt"])
        if kind == "select_visibility":
            touched = False
            if op["view"] and m.vis is None:  # a model without planes gets a view first
                self._switch(dev, True, None)
                self._view(key, self.view.pose, False, dev)
            if op["touch"] is not None and m.vis is not None and not m.vis["survived"] >= {"mask", "sel", "edit"}:
                t, touched = op["touch"], True  # the planes survive a mask, a selection and an edit change, through the ordinary state ops
                self.apply({"kind": "mask_eval", "key": key, "expr": t["expr"]}, dev, sub=True)
                self.apply({"kind": "sel_upload", "key": key, "rseed": t["sel"], "density": 0.5}, dev, sub=True)
                self.apply({"kind": "edits_upload", "key": key, "rseed": t["edits"]}, dev, sub=True)
            if dev is not None and op["inflight"]:
                # The frames in flight come last, so that nothing but the select (or its refusal) follows them.  A frame of `live`
                # alone would persist a selection edit onto the selection just uploaded, which `rebuilt` has not drawn yet: a frame
                # of both viewers, compared as every other, comes first then
                if touched:
                    dev.frame()
                dev.enqueue_frames(op["inflight"])
            self.vis_selects.append(dict(refused=m.vis is None, survived=frozenset(m.vis["survived"]) if m.vis is not None else frozenset(),
                                         inflight=self.lanes > 1 and op["inflight"] >= 2))
            if m.vis is None:  # refused, and the selection stays
                if m.vis_lost:
                    self.vis_refusals.append(m.vis_lost)
                if dev is not None:
                    dev.select_refused(key)
                    dev.check_selection(key, m.selection(), upload=False)
                return
            self._touched(key, "sel")
            if m.vis["peak"] is None:  # without a device there are no planes to select by: residency alone
                return
            # the range the draw could not know: two quantiles of the positive values of the adopted plane, or "never seen"
            x = sh.vis_values(key, op["measure"])
            seen = x[x > 0]
            lo, hi = (0.0, 0.0) if op["q_lo"] is None or not seen.size else (float(q) for q in np.quantile(seen, [op["q_lo"], op["q_hi"]]))
            op.update(lo=lo, hi=hi)
            self.log[-1].update(lo=lo, hi=hi)
        if op.get("seeds") is not None:
            m.sel = random_bits(m.n, op["seeds"], 0.02)
            self._touched(key, "sel")
            if dev is not None:
                dev.upload_selection(key, m.sel)
        if op.get("dst_seeds") is not None:
            t = sh.models[op["dst"]]
            t.sel = random_bits(t.n, op["dst_seeds"], 0.3)
            self._touched(op["dst"], "sel")
            if dev is not None:
                dev.upload_selection(op["dst"], t.sel)
        got = dev.select(op) if dev is not None else None  # (hit, selected[, threshold or the matrix used])
        if kind == "select_nearest":
            target = None if sh.models[op["dst"]].sel is None else sh.models[op["dst"]].sel.copy()
            want = sh.select_nearest(key, op["dst"], op["transfer"], op["lo"], op["hi"], op["op"], op["flt"], op["dst_filter"],
                                     op["xform"] if got is None else got[2], op["model_transforms"], op["max_distance"])
            variant = "select_nearest:" + ("transfer" if op["transfer"] else "range")
            if dev is not None and op["dst"] != key:  # the target's selection is read, never written
                dev.check_selection(op["dst"], sh.models[op["dst"]].selection() if target is None else target, upload=False)
        elif kind == "select_visibility":
            want, variant = sh.select_visibility(key, op["measure"], op["lo"], op["hi"], **a), "select_visibility:" + VIS_MEASURES[op["measure"]]
        elif kind == "select_range":
            want, variant = sh.select_range(key, op["prop"], op["lo"], op["hi"], world=op["world"], **a), "select_range:" + ("world" if op["world"] else "model")
        elif kind == "select_neighbors":
            want, variant = sh.select_neighbors(key, op["r"], op["lo"], op["hi"], **a), kind
        elif kind == "select_clusters":
            want, variant = sh.select_clusters(key, op["r"], op["mode"], op["size_lo"], op["size_hi"], **a), f"select_clusters:{op['mode']}"
        else:
            threshold = got[2] if got is not None and op["std_ratio"] is not None else None
            want = sh.select_knn(key, op["k"], op["score"], op["lo"], op["hi"], op["std_ratio"], threshold=threshold, **a)
            variant = "select_knn:" + ("range" if op["std_ratio"] is None else "std_ratio")
        if 0 < want[0] < m.n:
            self.nontrivial.add(variant)
        self._touched(key, "sel")
        if dev is not None:
            assert tuple(got[:2]) == want, (kind, got, want)
            dev.check_selection(key, m.sel)

    def _apply_model_op(self, op, dev):
        kind, sh = op["kind"], self.shadow
        removed, changed, requantised = list(op.get("evict", [])), [], []
        if "view_first" in op:  # then the frames in flight, right in front of the call that drops the planes
            if op["view_first"]:
                self._view_first(op["key"], dev)
            if dev is not None and op["inflight"]:
                dev.enqueue_frames(op["inflight"])
        # did the model a transform, a pod kind change or a new upload goes to hold visibility planes?
        had = {op["key"]: sh.models[op["key"]].vis is not None} if kind in ("xf_translate", "xf_scale", "xf_full", "set_pod_kind", "remove_add") else {}
        for k in removed:
            sh.remove(k)
        if dev is not None and removed:
            dev.remove(removed)
        exact = {}
        if kind in ("xf_translate", "xf_scale", "xf_full"):
            key = op["key"]
            if dev is not None and op["flt"]:
                dev.check_pivot(key, op["pivot"])
            count, exact[key] = sh.apply_transform(key, op["t"], op["q"], op["s"], op["pivot"], op["flt"])
            if dev is not None:
                assert dev.live.models[key].apply_transform(op["t"], op["q"], op["s"], op["pivot"], op["flt"]) == count
            changed = [key]
        elif kind == "set_pod_kind":
            key = op["key"]
            exact[key] = sh.set_pod_kind(key, op["to"])
            if dev is not None:
                dev.live.models[key].set_pod_kind(*op["to"])
            changed, requantised = [key], [key]
        elif kind in ("convert", "extract"):
            changed, requantised = self._extract(op["key"], op["dst"], op["flt"], op["invert"], op["drop_edits"], op.get("to"), exact, dev)
            if changed and op["remove_src"]:
                sh.remove(op["key"])
                removed.append(op["key"])
                if dev is not None:
                    dev.remove([op["key"]])
        elif kind == "decimate":
            key, dst, src = op["key"], op["dst"], sh.models[op["key"]]
            assert self.driver is not None, "a session that decimates needs the built tests/decimate_driver.cpp"
            stats, dmap, exact[dst] = sh.decimate(key, dst, op["cell"], op["flt"], op["invert"], self.driver)
            in_force = bool(op["flt"] & X.MASKED and src.mask is not None) or bool(op["flt"] & X.SELECTED and src.sel is not None)
            self.decimates.append(dict(filtered=in_force, kind_differs=src.kind != self.kind, count=stats[0], cells=stats[2], singletons=stats[3],
                                       largest_cell=stats[4]))
            if dev is not None:
                got = dev.live.models[key].decimate(dst, op["cell"], op["flt"], op["invert"], want_map=True)
                assert (got.count, got.n_nonfinite, got.cells, got.singletons, got.largest_cell) == stats, (got, stats)
                assert np.array_equal(got.map, dmap), "the decimate's map"
            changed, requantised = [dst], [dst]  # (rebuilt from the driver's float32 rows, uploaded in src's kind: test_gpu_decimate's yardstick)
            if op["remove_src"]:
                sh.remove(key)
                removed.append(key)
                if dev is not None:
                    dev.remove([key])
        elif kind == "merge":
            srcs = list(op["srcs"])
            if op.get("via"):
                changed, requantised = self._extract(srcs[-1], op["via"], 0, False, False, sh.models[srcs[0]].kind, exact, dev)
                self._settle(changed, requantised, exact, dev, kind)  # the converted source is a model of its own until the merge
                sh.remove(srcs[-1])
                removed.append(srcs[-1])
                if dev is not None:
                    dev.remove([srcs[-1]])
                srcs[-1] = op["via"]
            total, counts, rows = sh.merge(op["dst"], srcs)
            if dev is not None:
                assert dev.live.merge(op["dst"], srcs) == (total, counts)
            exact[op["dst"]] = rows
            changed, requantised = [op["dst"]], []
            for k in dict.fromkeys(srcs):  # the sources removed or kept; the converted copy always goes
                if op["remove_srcs"] or k == op.get("via"):
                    sh.remove(k)
                    removed.append(k)
                    if dev is not None:
                        dev.remove([k])
        elif kind == "ply_roundtrip":
            key, dst = op["key"], op["dst"]
            m = sh.models[key]
            d = sh.add(dst, self.kind, _rows(m.planes, np.arange(m.n)))
            exact[dst] = [np.full(d.n, True), np.full(d.n, False), np.full(d.n, False), np.full(d.n, False)]
            if dev is not None:
                dev.ply_roundtrip(key, dst, m.n)
                dev.remove([key])
            sh.remove(key)
            removed.append(key)
            changed = [dst]
        elif kind == "remove_add":
            key = op["key"]
            sh.models[key].drop_vis("remove_add")
            lost = sh.models[key].vis_lost
            sh.remove(key)
            g = self.scene(op["n"], op["scene_seed"])
            sh.add(key, self.kind, oracle.convert(g), op["mt"]).vis_lost = lost
            if dev is not None:
                dev.remove([key])
                dev.new_model(key, g, op["mt"])
                self._take_upload(key, dev)
            self.view.hidden.discard(key)
            self._planes_dropped(key, had.get(key), dev)
            return [key]
        self._settle(changed, requantised, exact, dev, kind)
        for key in had:
            self._planes_dropped(key, had[key], dev)
        self.view.hidden -= set(changed) | set(removed)
        return changed

    def _planes_dropped(self, key, had, dev):
        """after a call that drops the visibility planes (an upload, a pod kind change, a transform that moves something) of a model
        that had some: a select by them is refused at once, and leaves the selection alone"""
        m = self.shadow.models.get(key)
        if not had or m is None or m.vis is not None:
            return
        self.vis_refusals.append(m.vis_lost)
        if dev is not None:
            dev.select_refused(key)
            dev.check_selection(key, m.selection(), upload=False)

    def _extract(self, src, dst, flt, invert, drop_edits, to, exact, dev):
        sh = self.shadow
        count, rows = sh.extract(src, dst, flt, invert, drop_edits, to)
        if dev is not None:
            model = dev.live.models[src]
            got = model.extract(dst, flt, invert, drop_edits) if to is None else model.convert(dst, to[0], to[1], flt, invert, drop_edits)
            assert got == count, (got, count)
        if not count:
            return [], []
        exact[dst] = rows
        return [dst], ([dst] if to is not None and tuple(to) != sh.models[src].kind else [])

    def _settle(self, changed, requantised, exact, dev, what):
        """after the device ran the op: check what the shadow knows of every changed model, rebuild the other viewer's copy from the
        shadow, and take what the shadow does not know.  A requantised model (convert, set_pod_kind) is rebuilt from the shadow's
        planes of BEFORE the conversion: the upload of those into the new kind is the yardstick (spec §16), so the two downloads
        must be the same bytes in every plane."""
        if dev is None:
            return
        sh = self.shadow
        for key in changed:
            got = dev.pod_live(key)
            sh.verify(key, got, exact[key], what)
            if key not in requantised:
                sh.adopt(key, got)
            dev.rebuild([], [key])
            sh.adopt(key, got)
            sh.verify(key, dev.pod_rebuilt(key), _all(sh.models[key].n), what + ": the model rebuilt from the shadow")
            dev.check_state(key, sh.models[key])
