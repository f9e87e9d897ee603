"""A host shadow of a viewer's models, for tests/test_model_shadow_cpu.py and tests/test_gpu_model_fuzz.py: what a long session of
model operations (gsx_model_extract, _merge, _convert, _set_pod_kind, _apply_transform, _import_ply, _decimate, the selects by
property, neighbour count, cluster, nearest neighbours and nearest in another model, gsx_mask_evaluate, the uploads) leaves in every
model, kept on the host, without a GPU and without libgsx.  Per model key: the pod kind, the dequantised planes as
gsx_model_download_pod returns them, the model transform, the mask bits, the selection bits, the stored edit records (each or none)
and show-unedited.

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
SELECTS = ("select_range", "select_neighbors", "select_clusters", "select_knn", "select_nearest")
READ_ONLY = ("bounds", "histogram", "property_values", "neighbors", "clusters", "knn", "export", "export_ply", "decimate_edge", "nearest", "align_step")
MODEL_CHANGING = ("xf_translate", "xf_scale", "xf_full", "set_pod_kind", "convert", "extract", "merge", "ply_roundtrip", "remove_add", "decimate")
FEATURES = ("depth_test", "hit_pairs", "gizmos")
SPATIAL = ("select_neighbors", "select_clusters", "select_knn", "neighbors", "clusters", "knn", "nearest", "select_nearest", "align_step")
NEAREST_FAMILY = ("nearest", "select_nearest", "align_step")  # two keys: the queries' model `key` and the targets' `dst`
OP_KINDS = CAMERA + STATE + SELECTS + READ_ONLY + MODEL_CHANGING + FEATURES
#: the variants condition (b) asks a non-trivial hit set of, each at least once over the seed set
SELECT_VARIANTS = ("select_range:model", "select_range:world", "select_neighbors", "select_clusters:0", "select_clusters:1", "select_clusters:2",
                   "select_knn:range", "select_knn:std_ratio", "select_nearest:range", "select_nearest:transfer")
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
        if mode != T.IDENTITY and idx.size:
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


def unmet(cases, decimates):
    """conditions (e), (f) and (h) of tests/test_gpu_model_fuzz.py over a seed set, stated once: `cases` is the union of the
    sessions' `cases`, `decimates` all their `decimates` records.  Returns what is not met."""
    out = []
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
        """(cell, flt, invert) of a decimate that leaves at least MIN_N cells: the edge decimate_ref.find_edge gives for a drawn
        target; where that leaves fewer (the count is not monotone in the edge) the median nearest-neighbour distance; where that
        does too, the same without a filter"""
        for f, inv in ((flt, invert), (0, False)):
            kept = self._kept_bits(m, f, inv)
            edge, cells = memo(D.find_edge, m.pos, kept, self._target(m, f, inv))
            if cells < MIN_N:
                edge = F(self._radius(m, 1, 1.0))
                cells = D.assign(m.pos, kept, edge)[3].size
            if cells >= MIN_N:
                return float(edge), f, inv
        raise AssertionError("no cell edge leaves MIN_N cells")

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
            op.update(size=VIEWPORTS[int(rng.integers(len(VIEWPORTS)))])
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
            op.update(key=key, t=t, q=q, s=s, pivot=pivot, flt=X.SELECTED if selected else 0, inflight=inflight)
        elif kind == "set_pod_kind":
            others = [k for k in KINDS if k != m.kind]
            op.update(key=key, to=others[int(rng.integers(len(others)))], inflight=inflight)
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
            cell, flt, invert = self._decimate_cell(m, flt, invert)
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
            n = int(rng.integers(1500, 4001))
            op.update(key=key, n=n if n != m.n else n + 1, scene_seed=int(rng.integers(1000, 100000)), mt=self._random_mt(), inflight=inflight)
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
    def apply(self, op, dev=None):
        """apply a drawn op to the shadow and, with `dev`, to the device in lock-step.  Returns the keys whose model changed."""
        kind, sh, v = op["kind"], self.shadow, self.view
        v.rect = None
        if dev is not None and op.get("inflight"):
            dev.enqueue_frames(op["inflight"])
        if kind == "cam_step":
            v.pose = (v.pose + 1) % 240
        elif kind == "cam_jump":
            v.pose = op["pose"]
        elif kind == "viewport":
            v.size = tuple(op["size"])
        elif kind == "visibility":
            v.hidden = set(op["hidden"])
        elif kind == "display":
            v.mode, v.gsize, v.deg = op["mode"], op["gsize"], op["deg"]
        elif kind == "model_transform":
            sh.models[op["key"]].mt = tuple(np.array(a, F) for a in op["mt"])
        elif kind == "mask_eval":
            sh.mask_evaluate(op["key"], op["expr"], self.shapes)
        elif kind == "sel_upload":
            m = sh.models[op["key"]]
            m.sel = None if op["density"] is None else random_bits(m.n, op["rseed"], op["density"])
        elif kind == "sel_edit":
            v.sel_edit_on = bool(op["flag"] & 1)
        elif kind == "edits_upload":
            m = sh.models[op["key"]]
            m.edits = None if op["rseed"] is None else normalise_edits(random_edits(m.n, op["rseed"]))
        elif kind == "unedited":
            sh.models[op["key"]].unedited = op["on"]
        elif kind == "rect_query":
            v.rect = op
        elif kind == "depth_test":
            v.depth = op["on"]
        elif kind == "hit_pairs":
            v.lines = op["on"]
        elif kind == "gizmos":
            v.gizmos = op["on"]
        elif kind in SELECTS:
            self._apply_select(op, dev)
            return []
        elif kind in READ_ONLY:
            if dev is not None:
                dev.read_only(op, sh)
            return []
        elif kind in MODEL_CHANGING:
            return self._apply_model_op(op, dev)
        if dev is not None:
            dev.state_op(op)
        return []

    def _apply_select(self, op, dev):
        kind, key, sh = op["kind"], op["key"], self.shadow
        m = sh.models[key]
        a = dict(op=op["op"], flt=op["flt"])
        if op.get("seeds") is not None:
            m.sel = random_bits(m.n, op["seeds"], 0.02)
            if dev is not None:
                dev.upload_selection(key, m.sel)
        if op.get("dst_seeds") is not None:
            t = sh.models[op["dst"]]
            t.sel = random_bits(t.n, op["dst_seeds"], 0.3)
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
        if dev is not None:
            assert tuple(got[:2]) == want, (kind, got, want)
            dev.check_selection(key, m.sel)

    def _apply_model_op(self, op, dev):
        kind, sh = op["kind"], self.shadow
        removed, changed, requantised = list(op.get("evict", [])), [], []
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
            sh.remove(key)
            g = self.scene(op["n"], op["scene_seed"])
            sh.add(key, self.kind, oracle.convert(g), op["mt"])
            if dev is not None:
                dev.remove([key])
                dev.new_model(key, g, op["mt"])
                self._take_upload(key, dev)
            self.view.hidden.discard(key)
            return [key]
        self._settle(changed, requantised, exact, dev, kind)
        self.view.hidden -= set(changed) | set(removed)
        return changed

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
