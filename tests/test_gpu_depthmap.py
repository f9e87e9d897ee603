"""GPU: gsx_render_depth_map and gsx_depth_map_device_ptrs (spec/RENDER_SPEC.md §25; csrc/kernels_depthmap.hip).  What is compared
bit for bit — the transmittance against a rendered frame with one and with two models, two calls against each other, the next frame
against the run without the call, the round trip of the ndc plane through the depth test — uses scenes that close pixels
(visibility_scenes.SOLID).  The planes are compared with tests/depthmap_ref.py walking the DEVICE's own projection and tile lists
(calls from before this section), on the scenes whose share of uncertain crossings stays under the cap (visibility_scenes.REF;
tests/test_depthmap_cpu.py proves the cap with the oracle's projection, the tests here assert it on the run)."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import depthmap_ref as D
from tests import visibility_scenes as S
from tests.model_ops import load as _load
from tests.test_gpu_visibility import _look_rot
from wgpu_3dgs_viewer_app_amd import _lib, camera
from wgpu_3dgs_viewer_app_amd.viewer import (Cov3dKind, DepthCompare, GaussianDisplayMode, GaussianShDegree, GsxError, HitPair, MultiModelViewer,
                                             ShKind, device_bytes)

pytestmark = pytest.mark.gpu
KEY = "m"
KINDS = [(ShKind(sh), Cov3dKind(cov)) for sh, cov in S.KINDS.values()]
KIND_IDS = list(S.KINDS)
INRIA = dict(alpha_max=0.99, alpha_min=1.0 / 255.0)
MODES = {"splat": GaussianDisplayMode.Splat, "ellipse": GaussianDisplayMode.Ellipse, "point": GaussianDisplayMode.Point}
U32 = np.uint32
NONE = _lib.GSX_DEPTH_MAP_NONE
PLANES = ("surface", "sum", "alpha", "transmittance", "index", "layer")
# two model transforms (pos, quat x y z w, scale) that keep the halves of a scene in view
MT = {"a": ((0.3, -0.2, 0.1), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0)),
      "b": ((-0.4, 0.1, -0.3), (0.0, float(np.sin(0.2)), 0.0, float(np.cos(0.2))), (1.1, 1.1, 1.1))}


def _open(spec, kind=KINDS[0], mode=GaussianDisplayMode.Splat, **options):
    """a viewer holding the scene under KEY, the camera and the Gaussian transform set"""
    g, cam, size = S.scene(spec)
    v = MultiModelViewer(sh=kind[0], cov3d=kind[1])
    _load(v, g, KEY)
    v.update_camera(cam, size)
    v.update_gaussian_transform(1.0, mode, GaussianShDegree.new(3), False)
    if options:
        v.set_render_options(**options)
    return v, g


def _open_two(spec, kind=KINDS[0], **options):
    """one scene's Gaussians split by index into the keys "a" and "b", with different model transforms"""
    g, cam, size = S.scene(spec)
    v = MultiModelViewer(sh=kind[0], cov3d=kind[1])
    half = g.shape[0] // 2
    _load(v, g[:half], "a", MT["a"])
    _load(v, g[half:], "b", MT["b"])
    v.update_camera(cam, size)
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
    if options:
        v.set_render_options(**options)
    return v


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


def _same(a, b):
    """two results: the same bytes in every plane and every statistic"""
    return (all(np.array_equal(_bits(getattr(a, p)), _bits(getattr(b, p))) for p in PLANES)
            and (a.n_covered, a.n_crossed, _bits(a.surface_min).item(), _bits(a.surface_max).item(), a.models)
            == (b.n_covered, b.n_crossed, _bits(b.surface_min).item(), _bits(b.surface_max).item(), b.models))


def _consistent(dm):
    """the statistics are the planes', and index, layer and surface go together"""
    crossed = dm.index != NONE
    assert np.array_equal(crossed, dm.layer != NONE) and np.array_equal(crossed, np.isfinite(dm.surface)) and not np.isnan(dm.surface).any()
    assert dm.n_covered == int((dm.alpha > 0).sum()) and dm.n_crossed == int(crossed.sum())
    if dm.n_crossed:
        assert dm.surface_min == dm.surface[crossed].min() and dm.surface_max == dm.surface[crossed].max() and dm.surface_min > 0
    else:
        assert np.isinf(dm.surface_min) and dm.surface_max == 0


def _words(bits):
    n = bits.shape[0]
    w = np.zeros((n + 31) // 32, U32)
    np.bitwise_or.at(w, np.arange(n)[bits] >> 5, (U32(1) << (np.arange(n)[bits] & 31).astype(U32)))
    return w


_hip = None


def _device_plane(ptr, shape, dtype=np.float32):
    """a plane of gsx_depth_map_device_ptrs, copied to the host"""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    out = np.empty(shape, dtype)
    assert _hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


# ---- 1. transmittance against a rendered frame ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,params", [
    ("5x3", "splat", None), ("partial", "splat", INRIA), ("partial", "ellipse", None), ("one-tile", "ellipse", INRIA), ("one-tile", "point", INRIA),
    ("7x5", "splat", None), ("long-list", "splat", INRIA), ("long-list", "point", None)])
def test_transmittance_is_the_rendered_frames_one_model(name, mode, params):
    v, g = _open(S.SOLID[name], KINDS[0], MODES[mode])
    with v:
        if params:
            v.set_spec_params(**params)
        v.render_frame([KEY])
        fb = v.download_framebuffer()
        dm = v.render_depth_map([KEY])
        assert np.array_equal(_bits(dm.transmittance), _bits(fb[..., 3])), "the new kernel's per-pixel sequence is not the compositor's"
        if mode == "splat":
            assert (fb[..., 3] < 1e-4).any(), "the scene closes pixels"
        assert dm.models == 1 and dm.n_crossed > 0
        _consistent(dm)
        closed = dm.transmittance < 1e-4
        assert (dm.index[closed] != NONE).all(), "threshold >= t_epsilon: a closed pixel has crossed"
        assert (dm.layer[dm.index != NONE] == 0).all()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", ["5x3", "partial", "long-list"])
@pytest.mark.parametrize("order", [("a", "b"), ("b", "a")], ids=["ab", "ba"])
def test_transmittance_is_the_rendered_frames_two_models(name, order, kind):
    v = _open_two(S.SOLID[name], kind)
    with v:
        v.render_frame(list(order))
        fb = v.download_framebuffer()
        assert (fb[..., 3] < 1e-4).any(), "the scene closes pixels"
        dm = v.render_depth_map(list(order))
        assert np.array_equal(_bits(dm.transmittance), _bits(fb[..., 3])), "T is not carried from model to model as the frame carries it"
        assert dm.models == 2
        _consistent(dm)
        layers = dm.layer[dm.index != NONE]
        assert (layers == 0).any() and (layers == 1).any(), "both models hold surfaces"
        total = S.SOLID[name][0]
        n = {"a": total // 2, "b": total - total // 2}
        for k, key in enumerate(order):
            assert (dm.index[dm.layer == k] < n[key]).all()
        # the nearest model alone is the walk's first launch: where it crosses, the second model changes nothing
        front = v.render_depth_map([order[1]])
        on = front.index != NONE
        assert np.array_equal(dm.index[on], front.index[on]) and (dm.layer[on] == 1).all() and np.array_equal(_bits(dm.surface[on]), _bits(front.surface[on]))


# ---- 2. the planes against the reference ------------------------------------------------------------------------------------------------
def _device_lists(v, key, size):
    v.render_frame([key])
    return v.download_projection(key), v.download_tile_lists(key)


@pytest.mark.parametrize("threshold", [0.5, 1.0])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(S.REF))
def test_planes_against_the_reference_on_the_devices_own_lists(name, kind, threshold):
    """The largest deviations seen on the MI355X (A, S and T as shares of their bounds) are in DESIGN.md, "Depth map"."""
    v, g = _open(S.REF[name], kind, progressive=0)
    w, h = S.REF[name][1:3]
    with v:
        pr, (off, lst) = _device_lists(v, KEY, (w, h))
        dm = v.render_depth_map([KEY], threshold=threshold)
        f = common.oracle_frame(S.scene(S.REF[name])[1], w, h)
        ref = D.walk(pr["mean2d"], pr["conic_opacity"], pr["key"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 1e-4, 0, threshold)
        unc, crossed, dev_a, dev_s, dev_t = D.check(ref, dm.surface, dm.sum, dm.alpha, dm.transmittance, dm.index, dm.layer, cap=S.UNCERTAIN_CAP, floor=0.25)
        print(f"depth map {name} {KIND_IDS[KINDS.index(kind)]} threshold {threshold}: L_max {ref.l_max}, most blends {int(ref.steps.max())}, uncertain "
              f"{int(ref.uncertain.sum())} of {ref.uncertain.size}, crossed {crossed:.1%}, A off by {dev_a:.3e} of its bound, S by {dev_s:.3e}, T by {dev_t:.3e}")
        _consistent(dm)
        if name == "long-list":
            assert ref.l_max > 256
        if threshold == 1.0:
            assert np.array_equal(np.isinf(dm.surface), dm.alpha == 0), "the front surface: +inf exactly where nothing was blended"
        depth = pr["key"].view(np.float32)
        on = dm.index != NONE
        assert np.array_equal(_bits(dm.surface[on]), _bits(depth[dm.index[on]])), "the surface is the stored depth key of its Gaussian"


@pytest.mark.parametrize("order", [("a", "b"), ("b", "a")], ids=["ab", "ba"])
def test_two_models_against_the_reference(order):
    spec = S.REF["partial"]
    w, h = spec[1:3]
    v = _open_two(spec, progressive=0)
    with v:
        lists = {k: _device_lists(v, k, (w, h)) for k in order}
        dm = v.render_depth_map(list(order))
        f = common.oracle_frame(S.scene(spec)[1], w, h)
        ref = None
        for layer in (1, 0):  # the last key first
            pr, (off, lst) = lists[order[layer]]
            ref = D.walk(pr["mean2d"], pr["conic_opacity"], pr["key"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 1e-4, 0, 0.5, layer=layer, state=ref)
        D.check(ref, dm.surface, dm.sum, dm.alpha, dm.transmittance, dm.index, dm.layer, cap=S.UNCERTAIN_CAP, floor=0.25)
        assert (ref.layer == 0).any() and (ref.layer == 1).any()
        _consistent(dm)


def test_three_models_against_the_reference():
    """visibility_scenes.THREE at 83 x 51: "mid" has no entry in the right three tile columns, so its launch (not the first) returns
    early there and must leave the planes of the first launch alone; "near" has none in the left three, so the first launch writes
    those tiles with an empty list.  The reference is chained through `state=` on the device's own lists."""
    models, cam, (w, h) = S.three_models()
    order = list(models)  # far to near
    v = MultiModelViewer(sh=KINDS[0][0], cov3d=KINDS[0][1])
    with v:
        for key, g in models.items():
            _load(v, g, key)
        v.update_camera(cam, (w, h))
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
        v.set_render_options(progressive=0)
        lists = {k: _device_lists(v, k, (w, h)) for k in order}
        dm = v.render_depth_map(order)
        f = common.oracle_frame(cam, w, h)
        ref = None
        for layer in (2, 1, 0):  # the last key first
            pr, (off, lst) = lists[order[layer]]
            ref = D.walk(pr["mean2d"], pr["conic_opacity"], pr["key"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 1e-4, 0, 0.5, layer=layer, state=ref)
        unc, crossed, dev_a, dev_s, dev_t = D.check(ref, dm.surface, dm.sum, dm.alpha, dm.transmittance, dm.index, dm.layer, cap=S.UNCERTAIN_CAP, floor=0.25)
        print(f"depth map of three models: uncertain {int(ref.uncertain.sum())} of {ref.uncertain.size}, crossed {crossed:.1%}, A off by {dev_a:.3e} of its "
              f"bound, S by {dev_s:.3e}, T by {dev_t:.3e}, layers {[int((ref.layer == k).sum()) for k in range(3)]}")
        assert all((ref.layer == k).any() for k in range(3)), "all three models hold surfaces"
        assert dm.models == 3
        _consistent(dm)
        # the device's own lists: whole tiles of a launch that is not the first are empty, and so are tiles of the first launch
        entries = {k: np.diff(np.asarray(lists[k][1][0], np.int64)).reshape(4, 6) for k in order}
        assert not entries["mid"][:, 3:].any() and entries["mid"][:, :3].any(), "the launch of 'mid' returns early in the right three tile columns"
        assert not entries["near"][:, :3].any() and entries["near"][:, 3:].any(), "the first launch writes the left three tile columns with an empty list"
        # there: a pixel the first launch crossed, in a tile where a later launch returned early, keeps its crossing ...
        kept = dm.layer == 2
        assert (ref.layer[:, 48:] == 2).any() and kept[:, 48:].any() and not kept[:, :48].any()
        assert (dm.index[kept] < models["near"].shape[0]).all()
        # ... and the walk without the model that is absent from a half is, in that half, the same bytes: the early return changed
        # nothing on the right, the first launch's write of an empty tile is the walk's neutral start on the left
        for keys, cols, layers in ((["far", "near"], slice(48, None), (0, 2)), (["far", "mid"], slice(0, 48), (0, 1))):
            two = v.render_depth_map(keys)
            for p in ("surface", "sum", "alpha", "transmittance", "index"):
                assert np.array_equal(_bits(getattr(two, p)[:, cols]), _bits(getattr(dm, p)[:, cols])), (keys, p)
            on = two.layer[:, cols] != NONE
            assert np.array_equal(np.asarray(layers, U32)[two.layer[:, cols][on]], dm.layer[:, cols][on]), (keys, "layer")


# ---- 3. determinism and isolation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [1, 2])
def test_two_calls_return_the_same_bytes_whatever_ran_before(in_flight):
    spec = S.SOLID["partial"]
    g, cam, size = S.scene(spec)
    v = _open_two(spec, frames_in_flight=in_flight)
    with v:
        first = v.render_depth_map(["a", "b"], ndc=True)
        ndc = _device_plane(v.depth_map_device_ptrs()["ndc"], size[::-1])
        assert _same(first, v.render_depth_map(["a", "b"], ndc=True))
        for pose in (4, 5, 6, 7, 6):  # a camera path: the later frames are speculated, and dealt to the lanes
            v.update_camera(camera.orbit_pose(pose), size)
            v.render_frame(["a", "b"])
        last = v.download_framebuffer()
        v.models["a"].visibility()
        v.update_camera(cam, size)
        again = v.render_depth_map(["a", "b"], ndc=True)
        assert _same(first, again)
        assert np.array_equal(_bits(_device_plane(v.depth_map_device_ptrs()["ndc"], size[::-1])), _bits(ndc))
        # the framebuffer downloaded after the call is the frame from before it (the camera's viewport is the same)
        assert np.array_equal(_bits(v.download_framebuffer()), _bits(last))
        # the planes the pointers name are the planes the call returned
        ptrs = v.depth_map_device_ptrs()
        assert ptrs["size"] == tuple(size)
        for p in PLANES:
            assert np.array_equal(_bits(_device_plane(ptrs[p], size[::-1], getattr(again, p).dtype)), _bits(getattr(again, p))), p
        # the ndc plane is the depth test's relation read backwards, 1 without a crossing
        P = np.ascontiguousarray(cam.projection(size[0] / size[1]), np.float32).reshape(16)
        with np.errstate(divide="ignore"):
            want = np.clip(P[14] / again.surface - P[10], np.float32(0), np.float32(1)).astype(np.float32)
        assert np.array_equal(_bits(ndc), _bits(want)) and (ndc[again.index == NONE] == 1).all() and (ndc[again.index != NONE] < 1).all()
        # without the flag the plane is not handed out
        v.render_depth_map(["a", "b"], planes=False)
        assert v.depth_map_device_ptrs()["ndc"] is None


def test_the_next_frame_is_the_frame_without_the_call():
    spec = S.SOLID["5x3"]
    size = S.scene(spec)[2]
    frames = []
    for call in (False, True):
        v = _open_two(spec)
        with v:
            out = []
            for k, pose in enumerate((5, 6, 7, 8)):
                v.update_camera(camera.orbit_pose(pose), size)
                if call and k in (1, 3):
                    v.render_depth_map(["a", "b"], planes=False)
                v.render_frame(["a", "b"])
                out.append(v.download_framebuffer())
            frames.append(out)
    for a, b in zip(*frames):
        assert np.array_equal(_bits(a), _bits(b))


def test_render_needs_a_new_preprocess_and_sort_and_the_planes_are_counted():
    v, g = _open(S.SOLID["5x3"])
    w, h = S.SOLID["5x3"][1:3]
    with v:
        v.preprocessor.preprocess(KEY)
        v.radix_sorter.sort(KEY)
        v.renderer.render([KEY])
        fb = v.download_framebuffer()
        v.models[KEY].visibility()  # (the scratch framebuffer the two calls share is allocated here)
        base = device_bytes()
        with pytest.raises(GsxError, match="no depth map"):
            v.depth_map_device_ptrs()
        v.render_depth_map([KEY], planes=False)
        assert device_bytes() >= base + 7 * 4 * w * h, "the planes are viewer-owned device memory"
        grown = device_bytes()
        v.render_depth_map([KEY], ndc=True)
        assert device_bytes() == grown, "the second call reuses them"
        assert np.array_equal(_bits(v.download_framebuffer()), _bits(fb))
        with pytest.raises(GsxError, match="not preprocessed"):
            v.renderer.render([KEY])
        v.preprocessor.preprocess(KEY)
        v.radix_sorter.sort(KEY)
        v.renderer.render([KEY])
        assert np.array_equal(_bits(v.download_framebuffer()), _bits(fb))
        # a viewport change drops the depth map
        v.update_camera(S.scene(S.SOLID["5x3"])[1], (w + 1, h))
        with pytest.raises(GsxError, match="viewport"):
            v.depth_map_device_ptrs()
        assert v.render_depth_map([KEY]).surface.shape == (h, w + 1) and v.depth_map_device_ptrs()["size"] == (w + 1, h)


# ---- 4. the round trip: a wall's ndc plane as the depth buffer of a second model ----------------------------------------------------------
def test_ndc_plane_of_a_wall_occludes_a_second_model():
    cam = camera.orbit_pose(0)
    w, h = 80, 48
    V = np.asarray(cam.view(), np.float64).reshape(4, 4).T
    R_, t = V[:3, :3], V[:3, 3]
    eye, fwd = -R_.T @ t, -R_[2]
    wall = common.small_scene(1, 91, 3, 2.0)
    wall["pos"][0] = (eye + 3.0 * fwd).astype(np.float32)
    wall["scale"][0] = (3000.0, 3000.0, 0.01)
    wall["rot"][0] = _look_rot(R_)
    wall["color"][0, 3] = 255
    # 200 Gaussians well behind the wall (view depth 6 to 8) and 20 well in front of it (1.5 to 2)
    rng = np.random.default_rng(5)
    pts = common.small_scene(220, 92, 3, 2.0)
    local = np.stack([rng.uniform(-1.0, 1.0, 220), rng.uniform(-0.6, 0.6, 220), np.concatenate([rng.uniform(6.0, 8.0, 200), rng.uniform(1.5, 2.0, 20)])], 1)
    pts["pos"] = (eye + local[:, :1] * R_[0] + local[:, 1:2] * R_[1] + local[:, 2:3] * fwd).astype(np.float32)
    pts["scale"] = 0.05
    pts["color"][:, 3] = 200
    behind = np.arange(220) < 200
    v = MultiModelViewer()
    with v:
        _load(v, wall, "wall")
        _load(v, pts, "pts")
        v.update_camera(cam, (w, h))
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
        v.render_frame(["pts"])
        plain = v.download_framebuffer()
        dm = v.render_depth_map(["wall"], ndc=True)
        assert dm.n_crossed == w * h and (dm.index == 0).all() and abs(float(dm.surface_min) - 3.0) < 1e-3 and dm.surface_max == dm.surface_min
        ptrs = v.depth_map_device_ptrs()
        ndc = _device_plane(ptrs["ndc"], (h, w))
        assert (ndc > 0).all() and (ndc < 1).all()
        # 1. the device plane handed over as it is
        v.set_depth_test(DepthCompare.Less)
        v.set_depth_buffer_device(ptrs["ndc"], w, h, 4 * w)
        v.render_frame(["pts"])
        on_device = v.download_framebuffer()
        # 2. the same plane downloaded and uploaded
        v.set_depth_buffer_device(None, 0, 0, 0)
        v.update_depth_buffer(ndc)
        v.render_frame(["pts"])
        uploaded = v.download_framebuffer()
        assert np.array_equal(_bits(on_device), _bits(uploaded))
        assert not np.array_equal(_bits(on_device), _bits(plain)), "the wall hides something"
        # 3. what stands well behind the wall contributes nothing, what stands well in front does
        v.models["pts"].gaussian_buffers.mask_buffer.upload(_words(behind))
        v.render_frame(["pts"])
        hidden = v.download_framebuffer()
        assert (hidden[..., 3] == 1).all() and not hidden[..., :3].any(), "a Gaussian well behind the wall contributes nothing"
        v.models["pts"].gaussian_buffers.mask_buffer.upload(_words(~behind))
        v.render_frame(["pts"])
        front = v.download_framebuffer()
        assert (front[..., 3] < 1).any(), "a Gaussian well in front of the wall contributes"
        assert np.array_equal(_bits(front), _bits(on_device)), "the depth-tested frame of all of them is the frame of those in front"
        # the call itself refuses while the test is on, and the planes stay
        with pytest.raises(GsxError, match="depth test"):
            v.render_depth_map(["wall"])
        assert np.array_equal(_bits(_device_plane(v.depth_map_device_ptrs()["ndc"], (h, w))), _bits(ndc))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_message_and_the_planes_as_they_were():
    import torch

    v = _open_two(S.SOLID["5x3"])
    w, h = S.SOLID["5x3"][1:3]
    cam = S.scene(S.SOLID["5x3"])[1]
    with v:
        L, hnd = v._L, v._h
        before = v.render_depth_map(["a", "b"], ndc=True)
        ptrs = v.depth_map_device_ptrs()

        def refused(what, call=None, status=_lib.GSX_ERR_INVALID_ARG):
            call = call or (lambda: v.render_depth_map(["a", "b"]))
            with pytest.raises(GsxError) as e:
                call()
            assert e.value.status == status, what
            msg = L.gsx_last_error_string().decode()
            assert "gsx_render_depth_map" in msg, what
            return msg

        v.set_depth_test(DepthCompare.Less)
        assert "depth test" in refused("depth")
        v.set_depth_test(DepthCompare.Always)
        v.update_hit_pairs([HitPair((0, 0, 0), (1, 1, 1))])
        assert "overlay lines" in refused("lines")
        v.update_hit_pairs(None)
        _lib.check(L.gsx_viewer_set_band(hnd, 0, 1))
        assert "band" in refused("band")
        _lib.check(L.gsx_viewer_set_band(hnd, 0, 0xFFFFFFFF))
        ext = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
        _lib.check(L.gsx_viewer_set_external_framebuffer(hnd, ext.data_ptr(), ext.numel() * 4))
        assert "external framebuffer" in refused("external framebuffer")
        _lib.check(L.gsx_viewer_set_external_framebuffer(hnd, None, 0))
        win = torch.zeros(2 * ((w + 15) // 16) * ((h + 15) // 16), dtype=torch.int32, device="cuda")
        _lib.check(L.gsx_shard_set_windows(hnd, b"b", win.data_ptr()))
        assert "shard" in refused("sharded model")
        _lib.check(L.gsx_shard_set_windows(hnd, b"b", None))
        # the arguments
        assert "no keys" in refused("n_keys == 0", lambda: v.render_depth_map([]))
        assert "twice" in refused("a repeated key", lambda: v.render_depth_map(["a", "b", "a"]))
        assert "no model 'nobody'" in refused("unknown key", lambda: v.render_depth_map(["a", "nobody"]), _lib.GSX_ERR_NOT_FOUND)
        for bad in (float("nan"), float("inf"), 0.0, 0.5e-4, 1.0 + 2.0 ** -20, -0.5):
            assert "threshold" in refused(f"threshold {bad}", lambda bad=bad: v.render_depth_map(["a", "b"], threshold=bad))
        keys = (C.c_char_p * 2)(b"a", b"b")

        def raw(desc):
            return L.gsx_render_depth_map(hnd, keys, 2, C.byref(desc), None, None, None, None, None, None, None)

        assert raw(_lib.DepthMapDesc(2, 0.5)) == _lib.GSX_ERR_INVALID_ARG and b"flag" in L.gsx_last_error_string()
        assert raw(_lib.DepthMapDesc(0, 0.5, (C.c_uint32 * 2)(0, 1))) == _lib.GSX_ERR_INVALID_ARG and b"reserved" in L.gsx_last_error_string()
        assert L.gsx_render_depth_map(hnd, keys, 2, None, None, None, None, None, None, None, None) == _lib.GSX_ERR_INVALID_ARG
        # GSX_DEPTH_MAP_NDC needs the depth test's projection: an orthographic one is refused, without the flag it is walked
        ortho = np.diag([0.2, 0.3, -0.02, 1.0]).astype(np.float32)
        ortho[2, 3] = -1.0
        view = np.ascontiguousarray(cam.view(), np.float32)
        v.update_camera_with_matrices(view, ortho.T.reshape(16), (w, h))
        assert "projection" in refused("ndc with an orthographic projection", lambda: v.render_depth_map(["a", "b"], ndc=True))
        v.update_camera(cam, (w, h))
        # nothing of all that touched the planes or what the pointers name
        assert v.depth_map_device_ptrs() == ptrs
        for p in PLANES:
            assert np.array_equal(_bits(_device_plane(ptrs[p], (h, w), getattr(before, p).dtype)), _bits(getattr(before, p))), p
        assert _same(before, v.render_depth_map(["a", "b"], ndc=True))
        # the smallest and the largest threshold are taken
        low = v.render_depth_map(["a", "b"], threshold=1e-4)
        assert low.n_crossed == int((low.transmittance < 1e-4).sum()) > 0, "at t_epsilon the crossing is the closing"
        assert v.render_depth_map(["a", "b"], threshold=1.0).n_crossed == before.n_covered
