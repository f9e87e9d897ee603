"""GPU: gsx_model_apply_transform (spec/RENDER_SPEC.md §21; csrc/kernels_transform.hip) against gsx_model_merge of a copy under the
same model transform (byte for byte: the two kernels restate one arithmetic), against the float32 restatement
tests/transform_ref.py for positions (bit for bit, pivot included), and against itself for everything it must leave alone.  Device
bytes are read as tests/test_gpu_merge.py reads them: the resident planes through gsx_model_download_pod (the exact dequantisation of
the stored values: equal only if the stored bits are), the shade records through the later, speculated frames of a camera path,
which shade from them."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import common
from tests import extract_ref as X
from tests import merge_ref as R
from tests import transform_ref as T
from tests.model_ops import H, KIND_IDS, KINDS, W, frames as _frames, load as _load, model_len as _len, pod as _pod
from wgpu_3dgs_viewer_app_amd import _lib, camera, query
from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator, MaskOp, MaskShape, MaskShapeKind, pack_program
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as F
from wgpu_3dgs_viewer_app_amd.viewer import (BufferHandle, CommGroup, Cov3dKind, GaussianDisplayMode, GaussianShDegree, GsxError, MultiModelViewer,
                                             ShKind)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
FRAME_TOL = 1e-3  # spec §8
POSES = (5, 6, 7, 8)
ZERO3, ONE3, IDENT = np.zeros(3, np.float32), np.ones(3, np.float32), np.float32([0, 0, 0, 1])
FLT = X.MASKED | X.SKIP_HIDDEN | X.SELECTED
# one record-bearing kind of each record size: 16, 12 and 8 words
RECORD_KINDS = [(ShKind.Single, Cov3dKind.Single), (ShKind.Half, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)]
RECORD_IDS = [f"{s.name}-{c.name}" for s, c in RECORD_KINDS]
CARRIED_KINDS = [(ShKind.Norm8, Cov3dKind.Half), (ShKind.Half, Cov3dKind.Single), (ShKind.Single, Cov3dKind.Single)]
CARRIED_IDS = [f"{s.name}-{c.name}" for s, c in CARRIED_KINDS]


def fixture_transform(seed, pos=(0.3, -0.2, 0.5), scale=(1.3, -0.7, 0.9)):
    """a random rotation, a scale with a negative component (a reflection), a translation (tests/test_gpu_merge.py's)"""
    q = np.random.default_rng(seed).normal(size=4)
    return np.float32(pos), (q / np.linalg.norm(q)).astype(np.float32), np.float32(scale)


def _apply(v, key, mt, pivot=(0.0, 0.0, 0.0), flt=0, invert=False):
    return v.models[key].apply_transform(mt[0], mt[1], mt[2], pivot, flt, invert)


def _same_bytes(a, b, what=""):
    for name, x, y in zip(("pos", "color", "sh", "cov3d"), a, b):
        assert x.shape == y.shape and x.tobytes() == np.ascontiguousarray(y).tobytes(), (what, name)


def _edit_records(n, seed):
    rng = np.random.default_rng(seed)
    e = query.default_edits(n)
    e["flag"][0::3] = int(F.ENABLED | F.HIDDEN)
    e["flag"][1::3] = int(F.ENABLED)
    e["flag"][5::7] |= int(F.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    e["color"][:, 0] = rng.random(n).astype(np.float32)
    e["contrast"] = rng.random(n).astype(np.float32)
    return e


def _upload_pod(v, key, pod):
    """a fresh model from pod planes (gsx_model_upload_pod_device; the planes staged on the device with torch)"""
    import torch

    pos, color, sh, cov = pod
    v.add_model(key, pos.shape[0])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pos, color.view(np.int32), sh, cov)]
    torch.cuda.synchronize()
    v.models[key].gaussian_buffers.gaussians_buffer.update_range_pod_device(0, pos.shape[0], *(t.data_ptr() for t in dev))
    v.poll()


def _state(v, key):
    """what the call must not touch: the mask, selection and edit downloads and the retained raw edits buffer"""
    bufs = v.models[key].gaussian_buffers
    return [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(), bufs.gaussians_edit_buffer.download().tobytes(),
            BufferHandle(v, key, "edits").download().tobytes()]


# ---- 1. the whole model equals merge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_whole_model_equals_merge(sh, cov):
    n = 2500
    mt = fixture_transform(61)
    g = common.small_scene(n, 61)
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g, "m")
        _load(v, g, "copy", mt)
        assert v.merge("ref", ["copy"]) == (n, [n])
        assert _apply(v, "m", mt) == n
        _same_bytes(_pod(v, "m"), _pod(v, "ref"))
        # the later frames are speculated and shade from the records
        want = _frames(v, ["ref"], poses=POSES)
        assert want[0][..., :3].max() > 0 and not np.array_equal(want[0], want[2])
        for k, (a, b) in enumerate(zip(_frames(v, ["m"], poses=POSES), want)):
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


# ---- 2. subsets and edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33, 1023, 1025, 4097])
def test_subsets_and_edges(n):
    """Kept rows are the rows of the merge of a copy under the same filter, byte for byte; every other row is the download before."""
    mt = fixture_transform(62)
    g = common.small_scene(n, 62)
    rng = np.random.default_rng(62 + n)
    mask, sel = rng.random(n) < 0.6, rng.random(n) < 0.7
    last = np.arange(n) == n - 1
    edits = _edit_records(n, 62)
    # (filter, invert, selection): random sets with garbage above n, their complement, none, only the last index, all
    variants = [(FLT, False, sel), (FLT, True, sel), (X.SELECTED, False, np.zeros(n, bool)), (X.SELECTED, False, last), (X.SELECTED, True, last), (0, False, sel),
                (0, True, sel)]
    with MultiModelViewer() as v:
        _load(v, g, "m")
        _load(v, g, "copy", mt)
        for key in ("m", "copy"):
            bufs = v.models[key].gaussian_buffers
            bufs.mask_buffer.upload(X.words(mask, True))
            bufs.gaussians_edit_buffer.upload(edits)
        for k, (flt, invert, selection) in enumerate(variants):
            for key in ("m", "copy"):
                v.models[key].gaussian_buffers.selection_buffer.upload(X.words(selection, True))
            v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)  # the planes as uploaded, again
            kept = X.kept(n, flt, X.INVERT if invert else 0, mask, selection, edits["flag"])
            before = _pod(v, "m")
            count = _apply(v, "m", mt, flt=flt, invert=invert)
            assert count == kept.size, (k, count, kept.size)
            after = _pod(v, "m")
            want = [a.copy() for a in before]
            if kept.size:
                total, _ = v.merge("ref", ["copy"], flt, invert=invert)
                assert total == kept.size
                for w, r in zip(want, _pod(v, "ref")):
                    w[kept] = r
                v.remove_model("ref")
            _same_bytes(after, want, k)
            if kept.size:
                assert not np.array_equal(after[0][kept], before[0][kept])
        sizes = [X.kept(n, f, X.INVERT if i else 0, mask, s, edits["flag"]).size for f, i, s in variants]
        assert sizes[2:6] == [0, 1, n - 1, n]  # none, only the last index, all but the last, all


@pytest.mark.parametrize("sh,cov", RECORD_KINDS, ids=RECORD_IDS)
def test_records_of_a_subset(sh, cov):
    """Unkept records untouched, kept records rewritten: the speculated frames of the model equal those of a model uploaded from its
    own downloaded pod (the upload writes planes and records from one value).  2300 Gaussians: three workgroups, ragged rounds, and
    one round in which every Gaussian is kept."""
    n = 2300
    sel = np.random.default_rng(63).random(n) < 0.6
    sel[1024:1280] = True
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, common.small_scene(n, 63), "m")
        v.models["m"].gaussian_buffers.selection_buffer.upload(X.words(sel, True))
        for mt in (fixture_transform(63, pos=(0.1, 0.05, -0.1), scale=(1.1, -0.9, 1.05)), (np.float32([0.05, 0.0, -0.05]), IDENT, np.float32([0.9, 1.1, 1.0])),
                   (np.float32([-0.1, 0.1, 0.0]), IDENT, ONE3)):  # full, no rotation, translate
            before = _pod(v, "m")
            assert _apply(v, "m", mt, flt=X.SELECTED) == int(sel.sum())
            pod = _pod(v, "m")
            assert all(np.array_equal(a[~sel], b[~sel]) for a, b in zip(pod, before)) and not np.array_equal(pod[0][sel], before[0][sel])
            _upload_pod(v, "fresh", pod)
            _same_bytes(_pod(v, "fresh"), pod)  # (quantising the decoded values again is the identity)
            got, want = _frames(v, ["m"], poses=POSES), _frames(v, ["fresh"], poses=POSES)
            assert want[0][..., :3].max() > 0 and not np.array_equal(want[0], want[2])
            for k, (a, b) in enumerate(zip(got, want)):
                assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))
            v.remove_model("fresh")


# ---- 3. carried planes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", CARRIED_KINDS, ids=CARRIED_IDS)
def test_carried_planes(sh, cov):
    n = 1500
    g = common.small_scene(n, 64)
    sel = np.random.default_rng(64).random(n) < 0.7
    with MultiModelViewer(sh=sh, cov3d=cov) as v, MultiModelViewer(sh=sh, cov3d=cov) as twin:
        for vv in (v, twin):
            _load(vv, g, "m")
            vv.models["m"].gaussian_buffers.selection_buffer.upload(X.words(sel, True))
        # translate only: colour, SH and covariance keep their stored bits; positions are the float32 formula's, bit for bit
        t = np.float32([0.25, -1.5, 3.0])
        before = _pod(v, "m")
        for quat in (IDENT, np.float32([-0.0, 0.0, 0.0, -1.0])):
            start = _pod(v, "m")
            assert _apply(v, "m", (t, quat, ONE3), flt=X.SELECTED) == int(sel.sum())
            after = _pod(v, "m")
            _same_bytes(after[1:], before[1:], "translate")
            want = start[0].copy()
            want[sel] = T.position(start[0][sel], t, quat, ONE3)
            assert after[0].tobytes() == want.tobytes() and not np.array_equal(after[0][sel], start[0][sel])
        # scale only: the SH planes keep their stored bits; the covariance is merge's
        scale = np.float32([1.25, -0.5, 2.0])
        start = _pod(v, "m")
        _upload_pod(v, "copy", start)
        v.update_model_transform("copy", ZERO3, IDENT, scale)
        assert v.merge("ref", ["copy"])[0] == n
        assert _apply(v, "m", (ZERO3, IDENT, scale)) == n
        after, ref = _pod(v, "m"), _pod(v, "ref")
        assert after[2].tobytes() == start[2].tobytes() and after[1].tobytes() == start[1].tobytes()
        assert after[3].tobytes() == ref[3].tobytes() and after[0].tobytes() == ref[0].tobytes()
        assert after[0].tobytes() == T.position(start[0], ZERO3, IDENT, scale).tobytes() and not np.array_equal(after[3], start[3])
        # the full identity with a pivot: nothing is written, the count is returned, and the camera path goes on as if nothing had
        # been called (the twin is never called): frames identical, the next frame still a speculated one
        for vv in (v, twin):
            vv.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
            frames = _frames(vv, ["m"], poses=POSES[:3])
        before = _pod(v, "m")
        for quat in (IDENT, np.float32([0, 0, 0, -1])):
            assert _apply(v, "m", (np.float32([0.0, -0.0, 0.0]), quat, ONE3), pivot=(1.5, -2.0, 0.5)) == n
            assert _apply(v, "m", (ZERO3, quat, ONE3), pivot=(1.5, -2.0, 0.5), flt=X.SELECTED) == int(sel.sum())
        _same_bytes(_pod(v, "m"), before, "identity")
        a, b = _frames(v, ["m"], poses=POSES[3:])[0], _frames(twin, ["m"], poses=POSES[3:])[0]
        assert np.array_equal(a, b) and frames[0][..., :3].max() > 0
        assert v.frame_stats("m")["speculated"] and twin.frame_stats("m")["speculated"]


# ---- 4. the pivot -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", [(ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)], ids=["Single-Single", "Norm8-Half"])
def test_pivot(sh, cov):
    n = 1500
    g = common.small_scene(n, 65)
    mt = fixture_transform(65)
    pivot = np.float32([0.7, -1.9, 0.3])
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g, "a")
        _load(v, g, "b")
        start = _pod(v, "a")
        assert _apply(v, "a", mt, pivot=pivot) == n and _apply(v, "b", mt) == n
        a, b = _pod(v, "a"), _pod(v, "b")
        assert a[0].tobytes() == T.position(start[0], *mt, pivot).tobytes()
        assert b[0].tobytes() == T.position(start[0], *mt).tobytes() and not np.array_equal(a[0], b[0])
        _same_bytes(a[1:], b[1:], "the covariance and the SH do not depend on the pivot")
        # a quaternion that is not of unit length: the matrix of the quaternion as given moves the positions
        q = np.float32([0.0, 0.0, 1.0, 1.0])
        assert _apply(v, "b", (ZERO3, q, ONE3), pivot=pivot) == n
        assert _pod(v, "b")[0].tobytes() == T.position(b[0], ZERO3, q, ONE3, pivot).tobytes()


def test_rotating_a_selection_about_its_centre_keeps_the_centre():
    """A half turn about z (the quaternion (0, 0, 1, 0): R = diag(-1, -1, 1) exactly) about the centre c of the selection's box maps the
    box onto itself: the new centre is c but for the rounding of the positions.  A position's error is at most the float32 bound of
    its own products, 16 u sum |a_i b_i| over merge_ref.bake's magnitudes for q = p - c, plus u |q| for the subtraction and u (|q| +
    |c|) for the final addition; the centre of the new box moves by no more than the largest of them, plus u |c| for its own
    rounding."""
    n = 3000
    sel = np.random.default_rng(66).random(n) < 0.5
    half_turn = np.float32([0, 0, 1, 0])
    with MultiModelViewer() as v:
        _load(v, common.small_scene(n, 66), "m")
        v.models["m"].gaussian_buffers.selection_buffer.upload(X.words(sel))
        c = v.models["m"].bounds(selected=True).center
        start = _pod(v, "m")[0]
        assert _apply(v, "m", (ZERO3, half_turn, ONE3), pivot=c, flt=X.SELECTED) == int(sel.sum())
        after = v.models["m"].bounds(selected=True)
        moved = _pod(v, "m")[0]
    assert moved[sel].tobytes() == T.position(start[sel], ZERO3, half_turn, ONE3, c).tobytes() and np.array_equal(moved[~sel], start[~sel])
    q = start[sel].astype(np.float64) - c.astype(np.float64)
    (_, _, _), (mag, _, _) = R.bake(q, np.zeros((q.shape[0], 0)), np.zeros((q.shape[0], 6)), ZERO3, half_turn, ONE3)
    bound = (16 * U * mag + U * np.abs(q) + U * (np.abs(q) + np.abs(c)[None, :])).max(axis=0) + U * np.abs(c)
    err = np.abs(after.center.astype(np.float64) - c)
    print(f"centre moved by {err} of a bound {bound}")
    assert (err <= bound).all() and np.abs(q).max() > 1.0


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------
def _stateful_model(v, g, mask, sel, edits):
    _load(v, g, "m")
    bufs = v.models["m"].gaussian_buffers
    bufs.mask_buffer.upload(X.words(mask, True))
    bufs.selection_buffer.upload(X.words(sel, True))
    bufs.gaussians_edit_buffer.upload(edits)


def _fresh_frame(pod, mask, sel, edits, pose):
    with MultiModelViewer() as fresh:
        _upload_pod(fresh, "m", pod)
        bufs = fresh.models["m"].gaussian_buffers
        bufs.mask_buffer.upload(X.words(mask, True))
        bufs.selection_buffer.upload(X.words(sel, True))
        bufs.gaussians_edit_buffer.upload(edits)
        return _frames(fresh, ["m"], poses=(pose,))[0]


@pytest.mark.parametrize("lanes", [1, 2])
def test_state_is_kept_and_the_next_frame_is_the_moved_model(lanes):
    n = 3000
    g = common.small_scene(n, 67)
    rng = np.random.default_rng(67)
    mask, sel, edits = rng.random(n) < 0.8, np.arange(n) < n // 2, _edit_records(n, 67)
    with MultiModelViewer() as v:
        if lanes > 1:  # frames in flight on two lanes, as tests/test_gpu_inflight.py sets them up
            v.set_render_options(speculative=1, min_slab=2048, frames_in_flight=lanes)
        _stateful_model(v, g, mask, sel, edits)
        before = _state(v, "m")
        box = v.models["m"].bounds()
        for pose in POSES[:3]:  # (with lanes: enqueued, not waited for)
            v.update_camera(camera.orbit_pose(pose), (W, H))
            v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
            v.render_frame(["m"])
        t = np.float32([10.0 * float(box.max[0] - box.min[0]), 0.0, 0.0])  # ten box sizes
        assert _apply(v, "m", (t, IDENT, ONE3), flt=X.SELECTED) == n // 2
        got = _frames(v, ["m"], poses=POSES[3:])[0]
        assert _state(v, "m") == before
        pod = _pod(v, "m")
        assert np.array_equal(pod[0][n // 2:], oracle.convert(g)[0][n // 2:]) and (pod[0][:n // 2, 0] > box.max[0]).all()
    want = _fresh_frame(pod, mask, sel, edits, POSES[3])
    assert want[..., :3].max() > 0 and np.array_equal(got, want), float(np.abs(got - want).max())


def test_a_mask_program_is_evaluated_over_the_moved_positions():
    """The same box program before and after the call: gsx_mask_evaluate must not take the second evaluation for a repetition of the
    first (the positions moved under it).  The call itself re-evaluates nothing: the bits stay."""
    n = 3000
    g = common.small_scene(n, 68)
    sel = np.arange(n) % 2 == 0
    box = [MaskShape(MaskShapeKind.Box, pos=np.float32([0.2, 0.0, 0.1]), scale=np.float32([1.2, 1.5, 1.0]))]
    op = MaskOp.parse("0")
    t = (np.float32([0.9, -0.4, 0.3]), IDENT, ONE3)
    with MultiModelViewer() as v, MultiModelViewer() as fresh:
        _load(v, g, "m")
        v.models["m"].gaussian_buffers.selection_buffer.upload(X.words(sel))
        MaskEvaluator(v).evaluate(op, "m", box)
        first = v.models["m"].gaussian_buffers.mask_buffer.download()
        start = _pod(v, "m")[0]
        assert np.array_equal(X.bits(first, n), X.bits(oracle.mask_evaluate(start, ZERO3, IDENT, ONE3, *pack_program(op, box)), n))
        _frames(v, ["m"], poses=POSES[:3])
        assert _apply(v, "m", t, flt=X.SELECTED) == int(sel.sum())
        assert v.models["m"].gaussian_buffers.mask_buffer.download().tobytes() == first.tobytes()  # not re-evaluated by the call
        MaskEvaluator(v).evaluate(op, "m", box)
        pod = _pod(v, "m")
        want_mask = X.bits(oracle.mask_evaluate(pod[0], ZERO3, IDENT, ONE3, *pack_program(op, box)), n)
        got_mask = X.bits(v.models["m"].gaussian_buffers.mask_buffer.download(), n)
        assert np.array_equal(got_mask, want_mask) and not np.array_equal(got_mask, X.bits(first, n)) and 0 < got_mask.sum() < n
        got = _frames(v, ["m"], poses=POSES[3:])[0]
        _upload_pod(fresh, "m", pod)
        MaskEvaluator(fresh).evaluate(op, "m", box)
        want = _frames(fresh, ["m"], poses=POSES[3:])[0]
        assert want[..., :3].max() > 0 and np.array_equal(got, want)


# ---- 6. the frame against the transformed source -------------------------------------------------------------------------------------
def test_frame_of_the_transformed_model_is_the_frame_of_the_source_under_the_model_transform():
    """Single + Single, tests/test_gpu_merge.py's fixture (400 Gaussians, 80 x 48, SH degree 3): the model transformed in place under
    the identity against a copy under the model transform, within the framebuffer tolerance of spec §8 (gsx_model_merge: 4.0e-6)."""
    seed, n, pose, size = 129, 400, 5, (80, 48)
    mt = fixture_transform(seed)
    g = common.small_scene(n, seed)
    with MultiModelViewer() as v:
        _load(v, g, "src", mt)
        _load(v, g, "m")
        assert _apply(v, "m", mt) == n
        transformed = _frames(v, ["src"], poses=(pose,), size=size)[0]
        in_place = _frames(v, ["m"], poses=(pose,), size=size)[0]
    diff = float(np.abs(in_place.astype(np.float64) - transformed).max())
    print(f"in-place frame against the transformed source's: {diff:.3e}")
    assert transformed[..., :3].max() > 0.5 and diff <= FRAME_TOL


# ---- 7. determinism -------------------------------------------------------------------------------------------------------------------
def test_two_copies_get_identical_bytes():
    n = 5000
    g = common.small_scene(n, 69)
    sel = np.random.default_rng(69).random(n) < 0.4
    mt = fixture_transform(69)
    with MultiModelViewer(sh=ShKind.Half, cov3d=Cov3dKind.Half) as v:
        for key in ("a", "b"):
            _load(v, g, key)
            v.models[key].gaussian_buffers.selection_buffer.upload(X.words(sel))
        for key in ("a", "b"):
            assert _apply(v, key, mt, pivot=(0.3, 0.2, -0.1), flt=X.SELECTED) == int(sel.sum())
        _same_bytes(_pod(v, "a"), _pod(v, "b"))
        for a, b in zip(_frames(v, ["a"], poses=POSES), _frames(v, ["b"], poses=POSES)):
            assert np.array_equal(a, b)


# ---- 8. errors and empties ----------------------------------------------------------------------------------------------------------
def _desc(mt=(ZERO3, IDENT, ONE3), pivot=(0.0, 0.0, 0.0), flt=0, flags=0, reserved=0):
    f = lambda a, k: (C.c_float * k)(*(float(x) for x in a))  # noqa: E731
    return _lib.TransformDesc(flt, flags, f(mt[0], 3), f(mt[1], 4), f(mt[2], 3), f(pivot, 3), reserved)


def test_errors_and_empties():
    """Every row of the error list but the allocation failure, which a test cannot ask of a shared device; the model's bytes are the
    same after every refusal."""
    n = 700
    g = common.small_scene(n, 70)
    good = fixture_transform(70)
    nan, inf = np.nan, np.inf
    with MultiModelViewer() as v, MultiModelViewer(sh=ShKind.Norm8, cov3d=Cov3dKind.Half) as other:
        _load(v, g, "m")
        L, before, count = v._L, _pod(v, "m"), C.c_uint64(12345)
        call = lambda desc, key=b"m": L.gsx_model_apply_transform(v._h, key, C.byref(desc), C.byref(count))  # noqa: E731
        bad = [_desc(good, flt=8), _desc(good, flags=X.DROP_EDITS), _desc(good, flags=4), _desc(good, flags=X.INVERT | 8), _desc(good, reserved=1),
               _desc((np.float32([nan, 0, 0]), good[1], good[2])), _desc((np.float32([0, inf, 0]), good[1], good[2])),
               _desc((good[0], np.float32([0, nan, 0, 1]), good[2])), _desc((good[0], np.float32([0, 0, -inf, 1]), good[2])),
               _desc((good[0], good[1], np.float32([1, nan, 1]))), _desc((good[0], good[1], np.float32([inf, 1, 1]))),
               _desc(good, pivot=(nan, 0, 0)), _desc(good, pivot=(0, 0, -inf)), _desc((good[0], np.zeros(4, np.float32), good[2])),
               _desc((good[0], np.float32([-0.0, 0, 0, -0.0]), good[2]))]
        for k, desc in enumerate(bad):
            assert call(desc) == _lib.GSX_ERR_INVALID_ARG and b"gsx_model_apply_transform" in L.gsx_last_error_string(), k
            _same_bytes(_pod(v, "m"), before, k)
        # null viewer, key, desc
        assert L.gsx_model_apply_transform(None, b"m", C.byref(_desc(good)), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_apply_transform(v._h, None, C.byref(_desc(good)), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_apply_transform(v._h, b"m", None, C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        # an unknown key
        assert call(_desc(good), b"nope") == _lib.GSX_ERR_NOT_FOUND and b"'nope'" in L.gsx_last_error_string()
        with pytest.raises(GsxError) as e:
            _apply(v, "m", (np.float32([nan, 0, 0]), good[1], good[2]))  # (the facade raises)
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG
        _same_bytes(_pod(v, "m"), before, "refusals")
        # an empty kept set (no selection: none passes), a model of 0 Gaussians: GSX_OK, count 0, nothing written
        assert call(_desc(good, flt=X.SELECTED)) == _lib.GSX_OK and count.value == 0
        _same_bytes(_pod(v, "m"), before, "empty kept set")
        _lib.check(L.gsx_model_create(v._h, b"zero", 0, int(ShKind.Single), int(Cov3dKind.Single)))
        count.value = 12345
        assert call(_desc(good), b"zero") == _lib.GSX_OK and count.value == 0
        # out_count is nullable; without a selection SELECTED inverted keeps all
        assert L.gsx_model_apply_transform(v._h, b"m", C.byref(_desc(good, flt=X.SELECTED, flags=X.INVERT)), None) == _lib.GSX_OK
        _load(v, g, "copy", good)
        assert v.merge("ref", ["copy"])[0] == n
        _same_bytes(_pod(v, "m"), _pod(v, "ref"), "SELECTED inverted, no selection")
        # a sharded model
        moved = _pod(v, "m")
        v.shard_set_limits("m", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        assert call(_desc(good)) == _lib.GSX_ERR_UNSUPPORTED
        _same_bytes(_pod(v, "m"), moved, "sharded")
        # a viewer with a communicator
        _load(other, g[:50], "m")
        held = _pod(other, "m")
        group = CommGroup(1)
        other.comm_init_group(group, 0)
        with pytest.raises(GsxError) as e:
            _apply(other, "m", good)
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED
        _same_bytes(_pod(other, "m"), held, "communicator")
        assert _len(v, "m") == (_lib.GSX_OK, n)
