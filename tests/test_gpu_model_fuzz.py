"""GPU: the device-side model operations against one another and against the frame pipeline's cached state, over long sessions.

Two viewers per seed, in lock-step.  `live`: speculation on, several slabs, 1 to 3 frames in flight, slab shading and the edit cache
on; every operation goes to it through the Python mirror.  `rebuilt`: speculative = 0, progressive = 0, one lane, GSX_NO_EDIT_CACHE; it
never receives a model operation: after every step that changes a model the affected models are dropped and created again from the
host shadow (tests/model_shadow.py) with convert_ref.upload_pod in the shadow's kind, then given the mask, selection, edit records,
transform and show-unedited.  Every step renders one frame on both with the same camera, viewport, display state and painter's order:
the two framebuffers (and the RGBA8 resolves, which show the gizmos and lines) must be the same bytes.  After each operation the
counts, words, rows and positions the shadow knows are asserted; tests/model_shadow.py's docstring lists what it adopts from the
device instead.  A failure's message names the seed, the step and the ops so far with their drawn parameters.

Conditions that keep this from passing vacuously, asserted by test_conditions_over_the_seed_set: (a) every op kind ran; (b) every
select variant had a hit set neither empty nor full; (c) every op kind that changes a model was followed, before the next such op, by
a speculated frame of a model it changed (a decimated model among them); (d) model-changing ops ran with two frames enqueued and not
waited for.  The run of camera steps after a model-changing op is model_shadow.POST_OP_RUN = 5: a changed model's first frame on each
of up to three lanes is unspeculated, the fourth and fifth speculate.  For gsx_model_decimate and the nearest calls across two models,
stated once in model_shadow.unmet and proven for the default seeds without a GPU by tests/test_model_shadow_cpu.py: (e) some decimate
had a source under a mask or selection filter and some a source of another kind than the seed's first, every decimate left at least
MIN_N cells, merged ones and singletons both, and some cell had three members or more; (f) a nearest call ran between two models
under GSX_NEAREST_MODEL_TRANSFORMS, between two of different pod kinds, from a model to itself with different filters, and with a
max_distance that some but not all queries met; (g) a decimate and a select_nearest ran with two frames enqueued and not waited for;
(h) an align step was not degenerate with a reference rotation above 1 degree.

gsx_model_visibility, gsx_model_select_visibility and gsx_render_depth_map (the op kinds `vis_view`, `select_visibility`, `depth_map`
of tests/model_shadow.py) draw a model's own unspeculated frame in the middle of the session; csrc/frame_isolation.h saves and puts back
what that frame changes.  `rebuilt` never receives the three calls: a field that FrameIsolation failed to restore in the same way on
both viewers would cancel out of the frame comparison.  Their yardstick is a third viewer per seed, `probe`: GSX_NO_EDIT_CACHE,
speculative = 0, progressive = 0, one lane, no depth test, lines, gizmos or query.  It renders nothing but what a call asks of it:
before each call the models named are dropped and uploaded into it from the shadow (Device.rebuild, the code that rebuilds `rebuilt`)
and it is given the step's camera, viewport, Gaussian transform, selection edit and highlight.  A view's planes, transmittance and
statistics on `live` are probe's bytes; after an accumulate onto resident planes they are the maximum and the exact sums over the
planes the shadow adopted, and the statistics are the view's; probe's frame of the model has the call's transmittance as its alpha,
bit for bit (vis_view_call, which also holds every view to the host-side identities of tests/test_gpu_visibility.py).  A depth map's
six planes, statistics and ndc plane are probe's bytes, its layers index the keys, its transmittance is the alpha of probe's frame of
those keys (depth_map_call); with `as_depth_buffer` the ndc plane is `live`'s depth buffer as it lies on the device and `rebuilt`'s
as a download, and the frames that follow compare as ever, each lane behind its own depth snapshot.  A select is numpy over the
adopted planes; without planes it is refused and leaves the selection alone, and so it is at once after every call that drops the
planes of a model that held some.  A refused view or depth map (a feature on and no `clear`) answers GSX_ERR_INVALID_ARG, names its
entry point and leaves the resident planes as they were: EVERY refused call finds some (the session puts an unrefused call in front
where there are none), a refused view is followed by a select of every Gaussian seen at all, whose hit count is the shadow's, and a
refused depth map by a download through the unchanged pointers of the six planes and the ndc plane, which are the adopted bytes.  A
viewport of another size withdraws the depth map's pointers.  Conditions, stated once in model_shadow.unmet_views, proven for the
default seeds without a GPU and asserted here on the run: (i) a vis_view accumulated onto planes from another pose or viewport, one
ran on a model with a mask and stored edits, one on a model of another kind than the seed's first; (j) a select_visibility was
refused for dropped planes after each of the three dropping calls (gsx_model_apply_transform, gsx_model_set_pod_kind, a new upload
under the key), one ran on planes that survived a mask, a selection and an edit change, and each measure had a hit set neither empty
nor full (under (b)); (k) a depth map walked three models or more, one left a hidden model out, one ran at 83 x 51 or 320 x 240, each
of the three thresholds ran, an ndc plane was the depth buffer of two frames or more on a seed with several lanes, a depth map was
followed by a viewport of another size, and one ran without the ndc plane; (l) each of vis_view and depth_map was refused once, with
planes or a map of the same viewport resident, and ran twice; (m) each of the three ran with two frames enqueued and not waited for:
an op that takes a view or uploads state first enqueues them after that, right in front of the call itself.  The draws are steered
by the seed's parity so that this holds whatever the walk's order.

A decimated model is settled as a requantised one: the other viewer's copy is uploaded from the float32 rows of
tests/decimate_driver.cpp (built once per module, a host program) in the source's kind, and the two downloads are the same bytes in
every plane.  The matrix of GSX_NEAREST_MODEL_TRANSFORMS is nearest_ref.model_matrix bit for bit, except the entries that are nothing
but the float64 rounding noise of a sum that cancels (_matrix_noise: the off-diagonal 1e-17s between a model and its decimated copy,
which share a transform), where the device's entry must be noise too; index, d2 and the selection words are then `brute`'s under the
RETURNED matrix, bit for bit.  The align delta is bounded by tests/test_gpu_nearest.py's formula from the reference's own Horn matrix:
over the default seeds and the directed test the bound was 7.3e-13 to 8.3e-12 and the deviation 1.2e-16 to 8.9e-16 (359 to 2534 pairs).

Cost, measured on an MI355X in one session: a seed takes 0.49 to 1.10 s, of which 0.13 to 0.20 s are the hundred and more frames of
both viewers and 0.01 s the uploads into `probe` (so no model is kept in it between calls); the same seeds took 0.46 to 1.34 s
(frames 0.10 to 0.28 s) in that session before vis_view, depth_map and select_visibility joined the walk, and, in an earlier one,
0.39 to 0.91 s (frames 0.11 to 0.15 s) before decimate, decimate_edge, nearest, select_nearest and align_step did (a seed of
test_gpu_speculation.py::test_fuzz_operation_sequences, which has no host reference, takes 0.08 to 0.15 s); the rest is the host's
brute-force restatements, the driver's process and the downloads.  That is why a seed has only two ops beyond its walk through the
kinds, and why the spatial ops draw models of at most model_shadow.SPATIAL_N Gaussians when there are."""
import os
import time
import types

import numpy as np
import pytest

from tests import bounds_ref as B
from tests import clusters_ref as CL
from tests import common
from tests import convert_ref as CV
from tests import decimate_ref as D
from tests import extract_ref as X
from tests import knn_ref as K
from tests import model_shadow as S
from tests import nearest_ref as R
from tests import neighbors_ref as N
from tests import property_ref as P
from tests import test_gpu_depthmap as DM
from tests import test_gpu_visibility as VS
from tests.test_gpu_depth_test import ndc_of
from tests.test_gpu_nearest import SUM_RTOL
from wgpu_3dgs_viewer_app_amd import _lib, camera, mask as mask_mod, parallel, query
from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator, MaskOp
from wgpu_3dgs_viewer_app_amd.ply import Gaussians
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, DepthCompare, GaussianDisplayMode, GaussianShDegree, GsxError, HitPair, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
F = np.float32
SEEDS = [int(x) for x in os.environ.get("GSX_MODEL_FUZZ_SEEDS", ",".join(str(s) for s in S.DEFAULT_SEEDS)).split(",")]
MODES = [GaussianDisplayMode.Splat, GaussianDisplayMode.Ellipse, GaussianDisplayMode.Point]
LINES = np.concatenate([HitPair((-1.5, 0.0, 0.0), (1.5, 0.6, 0.0), (255, 40, 40, 255), 30.0), HitPair((0.0, -1.0, -1.0), (0.3, 1.0, 1.0), (40, 255, 40, 200), 20.0)])
#: what the seeds of this run saw, for the conditions over the seed set
SEEN = dict(seeds=[], ran={}, nontrivial=set(), speculated_after=set(), in_flight_ops={}, cases=set(), decimates=[],
            vis=dict(views=[], selects=[], refusals=[], depth_maps=[]))
#: tests/test_gpu_visibility.py's telescoping bound, per blended pair: every pair moves its weight from T into the sum
VIS_TELESCOPE = 3 * 2.0 ** -24 + 2.0 ** -25


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/decimate_driver.cpp, a stand-alone host program: the merged rows of every decimate"""
    return D.build_driver(tmp_path_factory.mktemp("decimate"))


def _kind(k):
    return ShKind(k[0]), Cov3dKind(k[1])


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same_f32(a, b, what):
    assert np.asarray(a).shape == np.asarray(b).shape and _bits(a).tobytes() == _bits(b).tobytes(), what


def _depth(size):
    """a cleared depth buffer with a rectangle at view depth 5.5 in its middle: in front of part of every scene here"""
    w, h = size
    d = np.ones((h, w), F)
    d[h // 4: (3 * h) // 4, w // 3: (2 * w) // 3] = ndc_of(camera.orbit_pose(0).projection(w / h), 5.5)
    return d


class Device:
    """the three viewers of a seed (`live`, `rebuilt` and `probe`, the yardstick of the visibility and depth map calls), and what
    model_shadow.Session asks of them"""

    def __init__(self, session, monkeypatch):
        self.s = session
        sh, cov = _kind(session.kind)
        self.live = MultiModelViewer(sh=sh, cov3d=cov)
        self.live.set_render_options(speculative=1, min_slab=512, frames_in_flight=session.lanes, host_verify=session.host_verify)
        monkeypatch.setenv("GSX_NO_EDIT_CACHE", "1")
        self.rebuilt = MultiModelViewer(sh=sh, cov3d=cov)
        self.probe = MultiModelViewer(sh=sh, cov3d=cov)
        monkeypatch.delenv("GSX_NO_EDIT_CACHE")
        for v in (self.rebuilt, self.probe):
            v.set_render_options(speculative=0, progressive=0, frames_in_flight=1)
        self.speculated, self.frame_s, self.probe_s = 0, 0.0, 0.0
        self.watch = None  # (op kind, the keys it changed) until a speculated frame of one of them, or the next model-changing op
        self.sel_edit = None  # the selection edit and highlight both viewers were given last: the probe gets them before a call
        self.dm_ptrs = None  # gsx_depth_map_device_ptrs of the live viewer's last depth map
        self.ndc_buffer = False  # the live viewer's depth buffer is its depth map's ndc plane
        self.has_depth_buffer = False  # the viewers were given a depth buffer at some time: it follows the viewport from then on
        self.query_preset = False  # `live` was given the step's query in front of a visibility or depth map call: the frame does not set it again

    def close(self):
        self.live.close()
        self.rebuilt.close()
        self.probe.close()

    def both(self, fn):
        for v in (self.live, self.rebuilt):
            fn(v)

    # ---- models ----
    def new_model(self, key, g, mt):
        self.live.add_model(key, g.shape[0])
        self.live.models[key].gaussian_buffers.gaussians_buffer.update_range(0, g)
        self.live.update_model_transform(key, *mt)

    def pod_live(self, key):
        assert CV.pod_kind(self.live, key) == _kind(self.s.shadow.models[key].kind), key
        return CV.pod(self.live, key)

    def pod_rebuilt(self, key):
        return CV.pod(self.rebuilt, key)

    def remove(self, keys):
        for k in keys:
            self.live.remove_model(k)
            if k in self.rebuilt.models:
                self.rebuilt.remove_model(k)

    def rebuild(self, removed, changed, v=None):
        """`changed` dropped and created again from the shadow in viewer `v` (default: `rebuilt`)"""
        v = self.rebuilt if v is None else v
        for k in removed:
            if k in v.models:
                v.remove_model(k)
        for k in changed:
            m = self.s.shadow.models[k]
            if k in v.models:
                v.remove_model(k)
            CV.upload_pod(v, k, m.planes, kind=_kind(m.kind))
            bufs = v.models[k].gaussian_buffers
            if m.mask is not None:
                bufs.mask_buffer.upload(X.words(m.mask))
            if m.sel is not None:
                bufs.selection_buffer.upload(X.words(m.sel))
            if m.edits is not None:
                bufs.gaussians_edit_buffer.upload(m.edits)
            v.update_model_transform(k, *m.mt)
            v.show_unedited(k, m.unedited)

    def check_state(self, key, m):
        """what an op carries or must leave alone, as the live viewer holds it"""
        bufs = self.live.models[key].gaussian_buffers
        assert CV.model_len(self.live, key) == m.n
        assert np.array_equal(X.bits(bufs.selection_buffer.download(), m.n), m.selection()), (key, "selection")
        want = query.default_edits(m.n) if m.edits is None else m.edits
        assert bufs.gaussians_edit_buffer.download().tobytes() == want.tobytes(), (key, "edit records")
        if m.mask is not None:
            assert np.array_equal(X.bits(bufs.mask_buffer.download(), m.n), m.mask), (key, "mask")

    def check_pivot(self, key, pivot):
        got = self.live.models[key].bounds(selected=True).center
        _same_f32(got, pivot, "bounds(selected).center")

    def ply_roundtrip(self, key, dst, n):
        data = self.live.models[key].export_ply()
        assert self.live.import_ply(dst, data) == n

    # ---- frames ----
    def _uniforms(self, v, pose):
        view = self.s.view
        v.update_camera(camera.orbit_pose(pose), view.size)
        v.update_gaussian_transform(view.gsize, MODES[view.mode], GaussianShDegree.new(view.deg), False)

    def _order(self, pose):
        alive = self.s.keys()
        shown = [k for k in alive if k not in self.s.view.hidden] or alive
        return parallel.model_render_keys(camera.orbit_pose(pose).pos, {k: types.SimpleNamespace(pos=self.s.shadow.models[k].mt[0]) for k in shown})

    def enqueue_frames(self, count):
        """frames of the live viewer alone, enqueued and not waited for, in front of the op that follows (a frame writes nothing but
        the selection edit it persists, which the step's own frame has written already)"""
        for j in range(1, count + 1):
            pose = (self.s.view.pose + j) % 240
            self._uniforms(self.live, pose)
            self.live.update_query(query.QueryPod.none())
            self.live.render_frame(self._order(pose))

    def _query(self):
        view = self.s.view
        return query.QueryPod.none() if view.rect is None else query.QueryPod.rect(view.rect["p0"], view.rect["p1"], query.QuerySelectionOp(view.rect["op"]))

    def _before_call(self, pose):
        """`live` in front of a visibility or depth map call: the camera the enqueued frames have moved on, and the step's query, which
        the step's frame then does NOT set again: the call switches it off for its own frame and must put it back"""
        self._uniforms(self.live, pose)
        self.live.update_query(self._query())
        self.query_preset = True

    def frame(self):
        t0 = time.perf_counter()
        try:
            return self._frame()
        finally:
            self.query_preset = False
            self.frame_s += time.perf_counter() - t0

    def _frame(self):
        s, view = self.s, self.s.view
        keys = self._order(view.pose)
        q = self._query()
        out = []
        for v in (self.live, self.rebuilt):
            self._uniforms(v, view.pose)
            if not (v is self.live and self.query_preset):  # (the query a visibility or depth map call had to put back)
                v.update_query(q)
            v.render_frame(keys)
            for k in keys:
                v.postprocessor.postprocess(k)
            v.poll()
            out.append((v.download_framebuffer(), v.download_rgba8()))
        assert np.array_equal(out[0][0], out[1][0]), f"framebuffers differ, L-inf {np.abs(out[0][0] - out[1][0]).max()}, keys {keys}"
        assert np.array_equal(out[0][1], out[1][1]), f"RGBA8 resolves differ, keys {keys}"
        if view.rect is not None and view.sel_edit_on:
            # The query's postprocess wrote the selection AFTER this frame's preprocess: a selection edit that persists reaches the
            # newly selected Gaussians in the NEXT frame's.  That frame is drawn here, on both, so that the stored edits the shadow
            # adopts below are those every later frame leaves alone (the frames enqueued in front of the next op among them).  This
            # extra frame is NOT compared: what it leaves in the stored edits is, below, and every later frame is
            for v in (self.live, self.rebuilt):
                v.update_query(query.QueryPod.none())
                v.render_frame(keys)
                v.poll()
        # what the frame itself wrote: the selection of a rectangle query, the stored edits of a selection edit that persists
        for k in keys:
            m = s.shadow.models[k]
            a, b = (v.models[k].gaussian_buffers for v in (self.live, self.rebuilt))
            if view.rect is not None:
                words = a.selection_buffer.download()
                assert np.array_equal(X.bits(words, m.n), X.bits(b.selection_buffer.download(), m.n)), (k, "selections differ")
                m.sel = X.bits(words, m.n)
            if view.sel_edit_on:
                edits = a.gaussians_edit_buffer.download()
                assert edits.tobytes() == b.gaussians_edit_buffer.download().tobytes(), (k, "stored edits differ")
                m.edits = edits if (edits["flag"] != 0).any() or m.edits is not None else None
        stats = {k: self.live.frame_stats(k)["speculated"] for k in keys}
        self.speculated += any(stats.values())
        if self.watch is not None and any(stats.get(k) for k in self.watch[1]):
            SEEN["speculated_after"].add(self.watch[0])
            self.watch = None
        return out[0][0]

    # ---- ops that both viewers get as they are ----
    def state_op(self, op):
        kind, view = op["kind"], self.s.view
        if kind == "viewport" and (view.depth or self.has_depth_buffer):
            # (with the test off as well, once there is a buffer: the overlay lines and gizmos read it, and it must be the viewport's)
            self.both(lambda v: v.update_depth_buffer(_depth(view.size)))
            self.ndc_buffer = False
        elif kind == "model_transform":
            self.both(lambda v: v.update_model_transform(op["key"], *op["mt"]))
        elif kind == "mask_eval":
            key, m = op["key"], self.s.shadow.models[op["key"]]
            MaskEvaluator(self.live).evaluate(MaskOp.parse(op["expr"]) if op["expr"] else None, key, self.s.shapes)
            if m.mask is not None:
                assert np.array_equal(X.bits(self.live.models[key].gaussian_buffers.mask_buffer.download(), m.n), m.mask), "mask bits"
            self.rebuilt.models[key].gaussian_buffers.mask_buffer.upload(None if m.mask is None else X.words(m.mask))
        elif kind == "sel_upload":
            m = self.s.shadow.models[op["key"]]
            self.both(lambda v: v.models[op["key"]].gaussian_buffers.selection_buffer.upload(None if m.sel is None else X.words(m.sel, True)))
        elif kind == "sel_edit":
            pod = query.GaussianEditPod(op["flag"], tuple(op["color"]), op["contrast"], op["exposure"], op["gamma"], op["alpha"])
            self.sel_edit = (pod, (1.0, 0.0, 1.0, op["highlight"]))
            self.both(lambda v: (v.update_selection_edit_with_pod(pod), v.update_selection_highlight(self.sel_edit[1])))
        elif kind == "edits_upload":
            m = self.s.shadow.models[op["key"]]
            raw = None if op["rseed"] is None else S.random_edits(m.n, op["rseed"])  # (as drawn: the library normalises them itself)
            self.both(lambda v: v.models[op["key"]].gaussian_buffers.gaussians_edit_buffer.upload(raw))
            self.check_state(op["key"], m)
        elif kind == "unedited":
            self.both(lambda v: v.show_unedited(op["key"], op["on"]))
        elif kind == "depth_test":
            # (off: the buffer stays, the overlay lines still read it.  An ndc plane does not stay: the next depth map overwrites it)
            fresh = op["on"] or self.ndc_buffer
            self.both(lambda v: (v.set_depth_test(DepthCompare.Less if op["on"] else DepthCompare.Always), v.update_depth_buffer(_depth(view.size)) if fresh else None))
            self.ndc_buffer, self.has_depth_buffer = False, self.has_depth_buffer or fresh
        elif kind == "hit_pairs":
            self.both(lambda v: v.update_hit_pairs(LINES if op["on"] else None))
        elif kind == "gizmos":
            self.both(lambda v: v.set_mask_gizmos(mask_mod.gizmo_records([self.s.shapes], 20.0) if op["on"] else None))

    # ---- selects ----
    def upload_selection(self, key, bits):
        self.both(lambda v: v.models[key].gaussian_buffers.selection_buffer.upload(X.words(bits)))

    def select(self, op):
        model, kind = self.live.models[op["key"]], op["kind"]
        a = dict(op=op["op"], filter=op["flt"])
        if kind == "select_visibility":
            return model.select_visibility(op["measure"], op["lo"], op["hi"], **a)
        if kind == "select_range":
            return model.select_range(op["prop"], op["lo"], op["hi"], world=op["world"], **a)
        if kind == "select_neighbors":
            return model.select_neighbors(op["r"], op["lo"], op["hi"], **a)
        if kind == "select_clusters":
            return model.select_clusters(op["r"], op["mode"], op["size_lo"], op["size_hi"], **a)
        if kind == "select_nearest":
            hit, selected, st = model.select_nearest(op["dst"], op["lo"], op["hi"], op["transfer"], op["op"], op["xform"], op["model_transforms"], op["flt"],
                                                     op["dst_filter"], op["max_distance"])
            _check_xform(st.xform, op, self.s.shadow.models[op["key"]], self.s.shadow.models[op["dst"]])
            return hit, selected, st.xform
        hit, selected, st = model.select_knn(op["k"], op["score"], op["lo"], op["hi"], op["std_ratio"], **a)
        if op["std_ratio"] is not None:  # the threshold within one unit in the last place of the restatement's (tests/test_gpu_knn.py)
            part, _, s = self.s.shadow.knn_scores(op["key"], op["k"], op["score"], op["flt"])
            ks = K.stats(np.where(part, s, K.INF))
            assert abs(int(_bits(st.threshold)[0]) - int(_bits(K.threshold(ks["mean"], ks["std"], op["std_ratio"]))[0])) <= 1
        return hit, selected, st.threshold

    def check_selection(self, key, bits, upload=True):
        assert np.array_equal(X.bits(self.live.models[key].gaussian_buffers.selection_buffer.download(), bits.size), bits), (key, "selection bits")
        if upload:
            self.rebuilt.models[key].gaussian_buffers.selection_buffer.upload(X.words(bits))

    # ---- read-only calls ----
    def read_only(self, op, shadow):
        read_only_call(self.live.models[op["key"]], shadow.models[op["key"]], op, shadow)

    # ---- the calls that draw a model's own frame; `rebuilt` never receives them ----
    def _probe(self, keys, pose):
        """the yardstick viewer holds `keys` as the shadow has them now, under the step's view state; no depth test, lines, gizmos, query"""
        t0 = time.perf_counter()
        p = self.probe
        self.rebuild([k for k in list(p.models) if k not in self.s.shadow.models], keys, p)
        self._uniforms(p, pose)
        if self.sel_edit is not None:
            p.update_selection_edit_with_pod(self.sel_edit[0])
            p.update_selection_highlight(self.sel_edit[1])
        self.probe_s += time.perf_counter() - t0

    def vis_view(self, key, pose, accumulate, m):
        self._probe([key], pose)
        self._before_call(pose)
        return vis_view_call(self.live, self.probe, key, accumulate, m.vis, m)

    def vis_kept(self, key, m):
        """the resident planes are the shadow's still: every Gaussian seen at all is hit.  The selection this writes is put back."""
        hit, _ = self.live.models[key].select_visibility(_lib.GSX_VIS_PEAK, *S.SEEN_AT_ALL)
        assert hit == int((m.vis["peak"] > 0).sum()), (key, "the resident visibility planes changed", hit)
        self.both(lambda v: v.models[key].gaussian_buffers.selection_buffer.upload(None if m.sel is None else X.words(m.sel, True)))

    def vis_refused(self, key, m):
        self._before_call(self.s.view.pose)
        with pytest.raises(GsxError) as e:
            self.live.models[key].visibility(accumulate=True)
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG and "gsx_model_visibility" in str(e.value), e.value
        assert m.vis is not None  # (the session sees to it that the model holds planes: the refusal must leave them as they were)
        self.vis_kept(key, m)

    def select_refused(self, key):
        with pytest.raises(GsxError, match="no visibility planes") as e:
            self.live.models[key].select_visibility(_lib.GSX_VIS_PEAK, *S.SEEN_AT_ALL)
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG

    def depth_map(self, op, shadow):
        view = self.s.view
        keys = self._order(view.pose)
        w, h = view.size
        self._probe(keys, view.pose)
        self._before_call(view.pose)
        got, ndc, self.dm_ptrs = depth_map_call(self.live, self.probe, keys, [shadow.models[k].n for k in keys], op["threshold"], op["ndc"])
        if op["as_depth_buffer"]:  # the plane as it lies on the device for `live`, downloaded and uploaded for `rebuilt`
            self.live.set_depth_test(DepthCompare.Less)
            self.live.set_depth_buffer_device(self.dm_ptrs["ndc"], w, h, 4 * w)
            self.rebuilt.set_depth_test(DepthCompare.Less)
            self.rebuilt.update_depth_buffer(ndc)
            self.ndc_buffer = self.has_depth_buffer = True
        return dict({p: getattr(got, p) for p in DM.PLANES}, **({"ndc": ndc} if op["ndc"] else {}))

    def depth_map_refused(self, resident):
        """`resident`: the session's depth map of this viewport (the session sees to it that there is one).  The refusal leaves its
        pointers and what they name as they were: the six planes and, where it has one, the ndc plane."""
        view = self.s.view
        self._before_call(view.pose)
        with pytest.raises(GsxError) as e:
            self.live.render_depth_map(self._order(view.pose))
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG and "gsx_render_depth_map" in str(e.value), e.value
        assert resident is not None and resident["size"] == tuple(view.size) and self.live.depth_map_device_ptrs() == self.dm_ptrs
        assert set(resident["planes"]) == set(DM.PLANES) | ({"ndc"} if resident["ndc"] else set())
        for p, want in resident["planes"].items():
            assert DM._device_plane(self.dm_ptrs[p], want.shape, want.dtype).tobytes() == want.tobytes(), ("a refused depth map changed the plane", p)

    def depth_map_dropped(self):
        """after a viewport op to another size: the pointers of the depth map are not handed out any more"""
        self._uniforms(self.live, self.s.view.pose)
        with pytest.raises(GsxError, match="viewport"):
            self.live.depth_map_device_ptrs()
        self.dm_ptrs = None


def _matrix_noise(s_mt, t_mt):
    """float64[3, 4]: 64 * 2^-53 times the sum of the absolute values of the terms of every entry of inv(M_dst) M_src: what two
    float64 evaluations of that product may differ by.  An entry of nearest_ref.model_matrix that is smaller than this is the
    rounding noise of a sum that cancels (a model and its extracted, converted or decimated copy share a transform: the product is
    the identity, and its off-diagonal entries are some 1e-17 of either sign): it has no bits to compare with."""
    (ps, qs, ss), (pd, qd, sd) = ([np.asarray(a, np.float64) for a in mt] for mt in (s_mt, t_mt))
    Rs, Rd = (np.abs(R.quat_rows(q / np.linalg.norm(q))) for q in (qs, qd))
    A = (Rd.T @ Rs) * ss[None, :] / sd[:, None]
    b = (Rd.T @ (np.abs(ps) + np.abs(pd))) / sd
    return 64 * 2.0 ** -53 * np.concatenate([A, b[:, None]], axis=1)


def _check_xform(got, op, s, t):
    """the matrix a nearest-family call used: nearest_ref.model_matrix of the two shadow transforms, the op's own, or the identity, bit
    for bit; where an entry of the reference is itself below its float64 rounding noise, the device's must be too"""
    if not op["model_transforms"]:
        _same_f32(got, S.IDENTITY34 if op["xform"] is None else op["xform"], "the matrix of the nearest search")
        return
    want, noise = R.model_matrix(s.mt, t.mt), _matrix_noise(s.mt, t.mt)
    cancels = np.abs(want.astype(np.float64)) <= noise
    assert (noise < 1e-13).all() and not cancels.all()
    assert np.array_equal(_bits(got)[~cancels], _bits(want)[~cancels]), ("the matrix of the model transforms", got, want)
    assert (np.abs(got.astype(np.float64))[cancels] <= noise[cancels]).all(), ("the entries that cancel", got, want)


def _check_nearest(got, ref, what):
    """the search's statistics against Shadow.nearest's: everything exact but the two float64 sums"""
    assert (got.count, got.n_nonfinite, got.targets, got.targets_nonfinite, got.n_found) == (
        ref["count"], ref["n_nonfinite"], ref["targets"], ref["targets_nonfinite"], ref["n_found"]), what
    _same_f32(got.d_min, ref["d_min"], (what, "d_min"))
    _same_f32(got.d_max, ref["d_max"], (what, "d_max"))
    assert got.mean == pytest.approx(ref["mean"], rel=SUM_RTOL, abs=0) and got.rms == pytest.approx(ref["rms"], rel=SUM_RTOL, abs=0), what


def _fixed(weight):
    """the weight plane as the device keeps it: int64 units of 2^-24 (gsx_model_visibility returns them times 2^-24, exactly)"""
    return np.round(np.asarray(weight, np.float64) * 2.0 ** 24).astype(np.int64)


def vis_view_call(live, probe, key, accumulate, resident, m):
    """gsx_model_visibility of `key` on `live` against `probe`, a plain viewer that holds the same model under the same view state and
    draws nothing else: the view's planes are probe's one view; after an accumulate onto `resident` (the shadow's adopted planes, or
    None) the planes are the maximum and the exact sums.  `m`: the shadow model (mask, stored edits, show-unedited).  Returns the
    planes to adopt."""
    want = probe.models[key].visibility(transmittance=True)
    got = live.models[key].visibility(accumulate=accumulate, transmittance=True)
    # the view by itself: what the host can say of any view
    assert want.views == 1 and want.n_pairs == int(want.pixels.sum(dtype=np.int64)) and want.weight_fixed == int(_fixed(want.weight).sum())
    assert want.n_seen == int((want.peak > 0).sum()) and want.peak_max == want.peak.max()
    lost = float((1.0 - want.transmittance.astype(np.float64)).sum())
    assert abs(want.weight_fixed / 2.0 ** 24 - lost) <= want.n_pairs * VIS_TELESCOPE, "the weights do not telescope into 1 - T"
    if m.mask is not None:
        assert not want.pixels[~m.mask].any(), "a Gaussian the mask excludes blended somewhere"
    if m.edits is not None and not m.unedited:
        assert not want.pixels[X.hidden(m.edits["flag"])].any(), "a Gaussian whose stored edit hides it blended somewhere"
    assert np.array_equal(_bits(got.transmittance), _bits(want.transmittance)), "the view's transmittance"
    if accumulate and resident is not None:
        assert np.array_equal(_bits(got.peak), _bits(np.maximum(resident["peak"], want.peak))), "accumulate: the peak is the maximum"
        assert np.array_equal(_fixed(got.weight), resident["weight"] + _fixed(want.weight)), "accumulate: the weight is the exact sum"
        assert np.array_equal(got.pixels, resident["pixels"] + want.pixels), "accumulate: the pixels are the sum"
        assert got.views == resident["views"] + 1
        assert (got.n_pairs, got.weight_fixed, got.n_visible) == (want.n_pairs, want.weight_fixed, want.n_visible), "the statistics are the view's"
        assert got.n_seen == int((got.peak > 0).sum()) and got.peak_max == got.peak.max()
    else:
        assert VS._same(got, want), "the planes and statistics of a first view"
    probe.render_frame([key])
    assert np.array_equal(_bits(probe.download_framebuffer()[..., 3]), _bits(want.transmittance)), "the transmittance is not the rendered frame's alpha"
    return dict(peak=got.peak, weight=_fixed(got.weight), pixels=got.pixels)


def depth_map_call(live, probe, keys, counts, threshold, ndc):
    """gsx_render_depth_map of `keys` (far to near; `counts`: their Gaussians) on `live` against `probe`, a plain viewer that holds the
    same models under the same view state.  Returns (the depth map, the ndc plane or None, gsx_depth_map_device_ptrs)."""
    size = tuple(probe.size)
    want = probe.render_depth_map(keys, threshold, ndc)
    want_ndc = DM._device_plane(probe.depth_map_device_ptrs()["ndc"], size[::-1]) if ndc else None
    got = live.render_depth_map(keys, threshold, ndc)
    assert DM._same(got, want), "the planes and statistics of the depth map"
    DM._consistent(got)
    ptrs = live.depth_map_device_ptrs()
    assert ptrs["size"] == size and (ptrs["ndc"] is not None) == bool(ndc)
    got_ndc = DM._device_plane(ptrs["ndc"], size[::-1]) if ndc else None
    assert not ndc or np.array_equal(_bits(got_ndc), _bits(want_ndc)), "the ndc plane"
    assert got.models == len(keys) and (got.layer[got.index != DM.NONE] < len(keys)).all(), "a layer names no key"
    for k, n in enumerate(counts):
        assert (got.index[got.layer == k] < n).all(), ("an index beyond its model", keys[k])
    probe.render_frame(keys)
    assert np.array_equal(_bits(probe.download_framebuffer()[..., 3]), _bits(got.transmittance)), "the transmittance is not the rendered frame's alpha"
    return got, got_ndc, ptrs


def read_only_call(model, m, op, shadow=None):
    """one read-only call of the model against the restatement over the shadow model `m` (`shadow`: the models, for the calls that
    name a second one)"""
    kind, flt = op["kind"], op["flt"]
    passes, part = m.passes(flt), m.part(flt)
    if kind == "decimate_edge":
        kept = np.zeros(m.n, bool)
        kept[m.kept(flt, op["invert"])] = True
        edge, cells = model.decimate_edge(op["target"], flt, op["invert"])
        want_edge, want_cells = S.memo(D.find_edge, m.pos, kept, op["target"])
        _same_f32(edge, want_edge, "decimate_edge")
        assert cells == want_cells
        got = model.decimate_count(edge, flt, op["invert"], want_map=True)
        dmap, count, nonfinite, members = D.assign(m.pos, kept, edge)
        assert (got.count, got.n_nonfinite, got.cells, got.singletons, got.largest_cell) == (
            count, nonfinite, members.size, int((members == 1).sum()), int(members.max()) if members.size else 0) and got.cells == cells
        assert np.array_equal(got.map, dmap)
    elif kind == "nearest":
        t = shadow.models[op["dst"]]
        got = model.nearest(op["dst"], op["xform"], op["model_transforms"], flt, op["dst_filter"], op["max_distance"])
        _check_xform(got.xform, op, m, t)
        ref = shadow.nearest(op["key"], op["dst"], flt, op["dst_filter"], got.xform, max_distance=op["max_distance"])
        assert np.array_equal(got.index, ref["index"]), "nearest index"
        _same_f32(got.d2, ref["d2"], "nearest d2")
        _check_nearest(got, ref, "nearest")
    elif kind == "align_step":
        st = model.align_step(op["dst"], op["xform"], False, op["with_scale"], flt, op["dst_filter"], op["max_distance"])
        ref = shadow.align(op["key"], op["dst"], op["xform"], op["with_scale"], flt, op["dst_filter"], op["max_distance"])
        _same_f32(st.nearest.xform, op["xform"], "the matrix of the align step")
        _check_nearest(st.nearest, ref["nearest"], "align_step")
        assert (st.n_pairs, st.degenerate) == (ref["n_pairs"], ref["degenerate"]), (st.n_pairs, st.degenerate, ref["n_pairs"], ref["degenerate"], ref["gap"], ref["norm"])
        assert st.rms_before == pytest.approx(ref["rms_before"], rel=SUM_RTOL, abs=0)
        if ref["degenerate"]:
            assert np.array_equal(st.quat, [0, 0, 0, 1]) and st.scale == 1 and not st.pos.any()
            _same_f32(st.xform_next, op["xform"], "a degenerate step's xform_next")
        else:
            dev = max(np.abs(st.quat - ref["quat"]).max(), abs(st.scale - ref["scale"]), np.abs(st.pos - ref["pos"]).max())
            print(f"align: {op['key']} -> {op['dst']}, {ref['n_pairs']} pairs, scale {op['with_scale']}, angle {ref['angle']:.3g} deg, |N| {ref['norm']:.6g} "
                  f"gap {ref['gap']:.6g} tol {ref['tol']:.3g} deviation {dev:.3g}")
            assert ref["tol"] <= S.ALIGN_TOL_MAX, "the draw promised a pair whose tolerance formula stays within the directed test's bound"
            assert st.quat[3] >= 0 and dev <= ref["tol"], (dev, ref["tol"])
            nxt = R.compose(dict(quat=st.quat, scale=st.scale, pos=st.pos), op["xform"])
            assert (np.abs(st.xform_next.astype(np.float64) - nxt.astype(np.float64)) <= np.spacing(np.abs(st.xform_next))).all(), "xform_next"
    elif kind == "bounds":
        got = model.bounds(masked=bool(flt & X.MASKED), skip_hidden=bool(flt & X.SKIP_HIDDEN), selected=bool(flt & X.SELECTED), trim_permille=op["trim"])
        want = B.reference(m.pos, passes)
        assert (got.count, got.n_nonfinite) == (want["count"], want["n_nonfinite"])
        for name in ("min", "max", "center"):
            _same_f32(getattr(got, name), want[name], ("bounds", name))
    elif kind == "histogram":
        vals = m.values(op["prop"], op["world"])
        lo, hi = (None, None) if op["auto"] else np.quantile(vals[passes & P.finite(vals)], [0.1, 0.9]).astype(F)
        got = model.histogram(op["prop"], op["bins"], lo, hi, filter=flt, world=op["world"])
        want = P.histogram(vals, passes, op["bins"], lo, hi)
        assert np.array_equal(got.bins, want["bins"])
        assert (got.count, got.below, got.above, got.n_nonfinite) == (want["count"], want["below"], want["above"], want["n_nonfinite"])
        for name in ("lo", "hi", "min", "max"):
            _same_f32(getattr(got, name), want[name], ("histogram", name))
    elif kind == "property_values":
        _same_f32(model.property_values(op["prop"], op["world"]), m.values(op["prop"], op["world"]), "property_values")
    elif kind == "neighbors":
        got = model.neighbors(op["r"], filter=flt)
        counts = N.brute(m.pos, part, op["r"])
        assert np.array_equal(got.counts, counts) and np.array_equal(got.hist, N.hist(counts, part)) and got.count == int(part.sum())
    elif kind == "clusters":
        got = model.clusters(op["r"], filter=flt)
        want = CL.clusters(m.pos, part, op["r"])
        assert np.array_equal(got.labels, want.labels) and np.array_equal(got.sizes, want.sizes)
        assert (got.count, got.n_clusters, got.largest_size, got.largest_label) == (want.count, want.n_clusters, want.largest_size, want.largest_label)
    elif kind == "knn":
        got = model.knn(op["k"], op["score"], filter=flt, rows=True)
        rows = S.memo(K.brute, m.pos, part, op["k"])
        score = K.score(rows, op["score"])
        st = K.stats(np.where(part, score, K.INF))
        _same_f32(got.d2, rows, "knn rows")
        _same_f32(got.score, score, "knn scores")
        assert (got.count, got.n_scored) == (int(part.sum()), st["n_scored"])
        _same_f32(got.score_min, st["score_min"], "score_min")
        _same_f32(got.score_max, st["score_max"], "score_max")
    else:
        idx = m.kept(flt, op["invert"])
        g = model.export(flt, op["invert"]).gaussians if kind == "export" else Gaussians.read_ply(model.export_ply(flt, op["invert"])).gaussians
        assert g.shape[0] == idx.size
        assert g["pos"].tobytes() == np.ascontiguousarray(m.pos[idx]).tobytes(), (kind, "pos")
        if kind == "export":
            assert np.array_equal(g["color"].view(np.uint32).reshape(-1), m.color[idx]), (kind, "color")
            assert g["sh"].reshape(-1, 45).tobytes() == np.ascontiguousarray(m.planes[2][idx]).tobytes(), (kind, "sh")


# ---- 1. the lock-step fuzz ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_model_operations(seed, monkeypatch, driver):
    t0 = time.perf_counter()
    s = S.Session(seed, driver)
    dev = Device(s, monkeypatch)
    step = -1
    try:
        s.load_start(dev)
        for step, kind in enumerate(S.plan(seed)):
            op = {"kind": "cam_step"} if kind == "cam_step" else s.draw(kind)
            changed = s.apply(op, dev)
            if kind in S.MODEL_CHANGING:
                dev.watch = (kind, changed)
            if s.lanes > 1 and op.get("inflight", 0) >= 2:
                SEEN["in_flight_ops"][kind] = SEEN["in_flight_ops"].get(kind, 0) + 1
            dev.frame()
    except (Exception, pytest.fail.Exception) as e:  # (pytest.raises' "DID NOT RAISE" is no Exception)
        raise AssertionError(f"{type(e).__name__}: {e}\n  at step {step} of {s.replay()}") from e
    finally:
        dev.close()
    SEEN["seeds"].append(seed)
    for k, c in s.ran.items():
        SEEN["ran"][k] = SEEN["ran"].get(k, 0) + c
    SEEN["nontrivial"] |= s.nontrivial
    SEEN["cases"] |= s.cases
    SEEN["decimates"] += s.decimates
    for name, recs in (("views", s.vis_views), ("selects", s.vis_selects), ("refusals", s.vis_refusals), ("depth_maps", s.depth_maps)):
        SEEN["vis"][name] += recs
    print(f"seed {seed}: lanes {s.lanes}, host_verify {s.host_verify}, kind {_kind(s.kind)}, {step + 1} frames, {dev.speculated} speculated, "
          f"{time.perf_counter() - t0:.2f} s of which {dev.frame_s:.2f} s in the frames of both viewers and {dev.probe_s:.2f} s in the uploads into the "
          f"probe, ops {dict(sorted(s.ran.items()))}\n  vis_view {s.vis_views}\n  select_visibility {s.vis_selects} after {s.vis_refusals}\n  depth_map {s.depth_maps}")
    assert dev.speculated > 0


def test_conditions_over_the_seed_set():
    """(a) to (m) of the module docstring, over the default seed set, which test_fuzz_model_operations ran before this.  A replay of
    other seeds through GSX_MODEL_FUZZ_SEEDS has no such set to answer for."""
    if set(SEEDS) != set(S.DEFAULT_SEEDS):
        pytest.skip("GSX_MODEL_FUZZ_SEEDS names other seeds than the default set the conditions are stated over")
    unfinished = sorted(set(S.DEFAULT_SEEDS) - set(SEEN["seeds"]))
    assert not unfinished, f"seeds that did not pass before this test (it is run with the whole file): {unfinished}"
    missing = [k for k in S.OP_KINDS if k != "cam_step" and not SEEN["ran"].get(k)]
    assert not missing, f"(a) op kinds that never ran: {missing}"
    trivial = [k for k in S.SELECT_VARIANTS if k not in SEEN["nontrivial"]]
    assert not trivial, f"(b) selects that never selected something and not everything: {trivial}"
    cold = [k for k in S.MODEL_CHANGING if k not in SEEN["speculated_after"]]
    assert not cold, f"(c) model-changing ops never followed by a speculated frame of the changed model: {cold}"
    assert sum(SEEN["in_flight_ops"].get(k, 0) for k in S.MODEL_CHANGING) > 0, "(d) no op ran with two frames enqueued and not waited for"
    unmet = S.unmet(SEEN["cases"], SEEN["decimates"], SEEN["vis"])
    assert not unmet, f"(e), (f), (h) to (m): {unmet}"
    cold = [k for k in ("decimate", "select_nearest") + S.VIEW_CALLS + ("select_visibility",) if not SEEN["in_flight_ops"].get(k)]
    assert not cold, f"(g), (m) never ran with two frames enqueued and not waited for: {cold}"


# ---- 2. directed ------------------------------------------------------------------------------------------------------------------------
def _two_lanes(**kw):
    v = MultiModelViewer(**kw)
    v.set_render_options(speculative=1, min_slab=512, frames_in_flight=2)
    return v


def _enqueue(v, pose, keys):
    v.update_camera(camera.orbit_pose(pose), (S.W, S.H))
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
    v.render_frame(keys)


def test_read_only_calls_between_frames_in_flight():
    """Two identical viewers with two lanes.  One enqueues two frames (one per lane), makes a read-only call, two frames, the next
    call ... through all of model_shadow.READ_ONLY, with no host wait but the call's own; its twin only renders.  A second model "t",
    the first 1200 Gaussians of "m" under a small rigid motion, is in every frame and is the target of the nearest search and the
    align step.  Every frame of both lanes is the twin's, and every answer is the restatement's."""
    n, n_t = 3000, 1200
    g = common.small_scene(n, 91)
    moved = g[:n_t].copy()
    half = np.radians(2.0) / 2
    motion = np.concatenate([R.quat_rows([0.0, 0.0, np.sin(half), np.cos(half)]), [[0.02], [-0.01], [0.015]]], axis=1).astype(F)
    moved["pos"] = R.map_points(motion, g["pos"][:n_t])
    rng = np.random.default_rng(91)
    shadow = S.Shadow()
    with _two_lanes() as v, _two_lanes() as twin, MultiModelViewer() as plain:
        for vv in (v, twin, plain):
            for key, rows in (("m", g), ("t", moved)):
                vv.add_model(key, rows.shape[0])
                vv.models[key].gaussian_buffers.gaussians_buffer.update_range(0, rows)
        m = shadow.add("m", S.SINGLE, CV.pod(v, "m"))
        t = shadow.add("t", S.SINGLE, CV.pod(v, "t"))
        m.mask, m.sel, m.edits = rng.random(n) < 0.8, rng.random(n) < 0.4, S.normalise_edits(S.random_edits(n, 91))
        for vv in (v, twin, plain):
            bufs = vv.models["m"].gaussian_buffers
            bufs.mask_buffer.upload(X.words(m.mask, True))
            bufs.selection_buffer.upload(X.words(m.sel, True))
            bufs.gaussians_edit_buffer.upload(m.edits)
        r = float(F(K.kth_distance_median(m.pos, m.part(0), 2)))
        flt = X.MASKED | X.SKIP_HIDDEN
        reach = float(F(K.kth_distance_median(t.pos, t.part(0), 1)))  # the targets' median nearest-neighbour distance
        calls = [dict(kind="bounds", flt=flt, trim=50), dict(kind="histogram", flt=flt, prop=P.HUE, bins=64, world=False, auto=True),
                 dict(kind="property_values", flt=0, prop=P.POS_Y, world=True), dict(kind="neighbors", flt=flt, r=r), dict(kind="clusters", flt=X.SELECTED, r=r),
                 dict(kind="knn", flt=flt, k=3, score=K.SCORE_MEAN), dict(kind="export", flt=X.SELECTED, invert=True), dict(kind="export_ply", flt=flt, invert=False),
                 dict(kind="decimate_edge", flt=flt, invert=False, target=600),
                 dict(kind="nearest", dst="t", flt=flt, dst_filter=0, xform=None, model_transforms=False, max_distance=reach),
                 dict(kind="align_step", key="t", dst="m", flt=0, dst_filter=X.MASKED, xform=S.IDENTITY34, with_scale=True, max_distance=0.0),
                 dict(kind="vis_view", accumulate=False), dict(kind="depth_map", threshold=0.5, ndc=True)]
        assert [c["kind"] for c in calls] == list(S.READ_ONLY)
        found = shadow.nearest("m", "t", flt, 0, max_distance=reach)
        assert 0 < found["n_found"] < found["count"]  # the max_distance rejects some queries and not all
        speculated = 0
        for k, call in enumerate(calls):
            poses = (10 + 2 * k, 11 + 2 * k)
            for pose in poses:
                _enqueue(v, pose, ["m", "t"])
            key = call.setdefault("key", "m")
            if call["kind"] in S.VIEW_CALLS:  # at the camera of the second frame in flight; the yardstick: the plain viewer, which draws nothing else
                plain.update_camera(camera.orbit_pose(poses[1]), (S.W, S.H))
                plain.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
                if call["kind"] == "vis_view":
                    vis_view_call(v, plain, key, call["accumulate"], None, m)
                else:
                    depth_map_call(v, plain, ["m", "t"], [n, n_t], call["threshold"], call["ndc"])
            else:
                read_only_call(v.models[key], shadow.models[key], call, shadow)
            got = [v.debug_download_lane_framebuffer(lane) for lane in (0, 1)]
            want = []
            for pose in poses:
                _enqueue(twin, pose, ["m", "t"])
                want.append(twin.download_framebuffer())
            assert want[0][..., :3].max() > 0 and not np.array_equal(want[0], want[1])
            assert any(all(np.array_equal(got[a], want[b]) for a, b in zip((0, 1), order)) for order in ((0, 1), (1, 0))), (k, call["kind"])
            v.poll()
            speculated += v.frame_stats("m")["speculated"]
        assert speculated >= 9  # (6 of 8 calls before decimate_edge, nearest and align_step joined: the same share of 11; not lowered for 13)


def test_a_key_removed_and_reused():
    """Frames in flight on two lanes, remove_model("m"), a model of another length under the same key, another pod kind: every frame
    that follows is a fresh viewer's (nothing derived from the first "m" survives: windows, shade records, a lane's shadow model)."""
    n, other_n = 3000, 1700
    to = (ShKind.Norm8, Cov3dKind.Half)
    with _two_lanes() as v, MultiModelViewer() as fresh:
        v.add_model("m", n)
        v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, common.small_scene(n, 92))
        for pose in (5, 6, 7, 8):  # enqueued, not waited for
            _enqueue(v, pose, ["m"])
        v.remove_model("m")
        v.add_model("m", other_n)
        v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, common.small_scene(other_n, 93))
        _enqueue(v, 9, ["m"])  # a frame of the new model in its first kind, in flight under the conversion
        v.models["m"].set_pod_kind(*to)
        held = CV.pod(v, "m")
        CV.upload_pod(fresh, "m", held, kind=to)
        CV.same_bytes(CV.pod(fresh, "m"), held)
        speculated = 0
        for k, pose in enumerate((10, 11, 12, 13, 14, 15)):
            _enqueue(v, pose, ["m"])
            a = v.download_framebuffer()
            _enqueue(fresh, pose, ["m"])
            b = fresh.download_framebuffer()
            assert b[..., :3].max() > 0 and np.array_equal(a, b), (k, float(np.abs(a - b).max()))
            speculated += v.frame_stats("m")["speculated"]
        assert speculated >= 3
