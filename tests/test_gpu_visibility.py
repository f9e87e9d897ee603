"""GPU: gsx_model_visibility, gsx_model_select_visibility and gsx_model_visibility_reset (spec/RENDER_SPEC.md §24;
csrc/kernels_visibility.hip).  What is compared bit for bit — the transmittance against a rendered frame, two calls against each
other, accumulation against single calls, the select against numpy over the downloaded planes — uses scenes that close pixels
(visibility_scenes.SOLID).  Peak, weight and pixels are compared with tests/visibility_ref.py walking the DEVICE's own projection and
tile lists (calls from before this section), on scenes whose share of uncertain pairs stays under the cap (visibility_scenes.REF;
tests/test_visibility_cpu.py proves the cap for the seeds with the oracle's projection, the test asserts it on the run)."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import visibility_ref as R
from tests import visibility_scenes as S
from tests.model_ops import load as _load
from wgpu_3dgs_viewer_app_amd import _lib, camera, query
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as EF
from wgpu_3dgs_viewer_app_amd.viewer import (Cov3dKind, DepthCompare, GaussianDisplayMode, GaussianShDegree, GsxError, HitPair,
                                             MultiModelViewer, ShKind, device_bytes)

pytestmark = pytest.mark.gpu
KEY = "m"
KINDS = [(ShKind(sh), Cov3dKind(cov)) for sh, cov in S.KINDS.values()]
KIND_IDS = list(S.KINDS)
INRIA = dict(alpha_max=0.99, alpha_min=1.0 / 255.0)
MODES = {"splat": GaussianDisplayMode.Splat, "ellipse": GaussianDisplayMode.Ellipse, "point": GaussianDisplayMode.Point}
U32 = np.uint32


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


def _bits(a):
    return np.ascontiguousarray(a).view(U32)


def _same(a, b):
    """two results: the same bytes in every plane and every statistic"""
    return (np.array_equal(_bits(a.peak), _bits(b.peak)) and np.array_equal(a.weight, b.weight) and np.array_equal(a.pixels, b.pixels)
            and (a.transmittance is None or np.array_equal(_bits(a.transmittance), _bits(b.transmittance)))
            and (a.n_visible, a.n_seen, a.n_pairs, a.weight_fixed, _bits(a.peak_max).item(), a.views)
            == (b.n_visible, b.n_seen, b.n_pairs, b.weight_fixed, _bits(b.peak_max).item(), b.views))


def _selected(v, n):
    w = v.models[KEY].gaussian_buffers.selection_buffer.download()
    return ((w[np.arange(n) >> 5] >> (np.arange(n) & 31)) & 1).astype(bool)


def _words(bits):
    n = bits.shape[0]
    w = np.zeros((n + 31) // 32, U32)
    np.bitwise_or.at(w, np.arange(n)[bits] >> 5, (U32(1) << (np.arange(n)[bits] & 31).astype(U32)))
    return w


# ---- 1. transmittance against a rendered frame ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name,mode,params,progressive", [
    ("5x3", "splat", None, 1), ("5x3", "splat", None, 0), ("partial", "splat", INRIA, 1), ("partial", "ellipse", None, 0),
    ("one-tile", "point", INRIA, 1), ("7x5", "splat", None, 1), ("long-list", "splat", None, 0), ("long-list", "ellipse", INRIA, 1),
    ("long-list", "point", None, 1)])
def test_transmittance_is_the_rendered_frames(name, mode, params, progressive, kind):
    v, g = _open(S.SOLID[name], kind, MODES[mode], progressive=progressive)
    with v:
        if params:
            v.set_spec_params(**params)
        v.render_frame([KEY])
        fb = v.download_framebuffer()
        vis = v.models[KEY].visibility(transmittance=True)
        assert np.array_equal(_bits(vis.transmittance), _bits(fb[..., 3])), "the new kernel's per-pixel sequence is not the compositor's"
        if mode == "splat":
            assert (fb[..., 3] < 1e-4).any(), "the scene closes pixels"
        assert vis.views == 1 and vis.n_pairs > 0 and vis.n_seen == int((vis.peak > 0).sum()) and vis.peak_max == vis.peak.max()
        assert vis.n_pairs == int(vis.pixels.sum()) and vis.weight_fixed == int(np.round(vis.weight * 2.0 ** 24).sum())


def test_transmittance_with_mask_hidden_and_opacity_edits_and_show_unedited():
    v, g = _open(S.SOLID["5x3"])
    n = g.shape[0]
    rng = np.random.default_rng(3)
    with v:
        m = v.models[KEY]
        bufs = m.gaussian_buffers
        bufs.mask_buffer.upload(_words(rng.random(n) < 0.8))
        edits = query.default_edits(n)
        hidden, faded = rng.random(n) < 0.15, rng.random(n) < 0.3
        edits["flag"][hidden] = int(EF.ENABLED | EF.HIDDEN)
        edits["flag"][faded & ~hidden] = int(EF.ENABLED)
        edits["alpha"][faded & ~hidden] = 0.4
        bufs.gaussians_edit_buffer.upload(edits)
        for unedited in (False, True):
            v.show_unedited(KEY, unedited)
            v.render_frame([KEY])
            fb = v.download_framebuffer()
            vis = m.visibility(transmittance=True)
            assert np.array_equal(_bits(vis.transmittance), _bits(fb[..., 3]))
            if not unedited:
                assert not vis.pixels[hidden].any() and vis.pixels[~hidden].any(), "a hidden Gaussian blends nowhere"
                t_edited = fb[..., 3].copy()
            else:
                assert not np.array_equal(t_edited, fb[..., 3]), "show_unedited draws another frame"


# ---- 2. peak, weight and pixels against the reference; 3. telescoping --------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", list(S.REF))
def test_planes_against_the_reference_on_the_devices_own_lists(name, kind):
    """Largest deviations seen on the MI355X (peak; weight as a share of its bound) are in DESIGN.md, "Visibility"."""
    v, g = _open(S.REF[name], kind, progressive=0)
    w, h = S.REF[name][1:3]
    with v:
        v.render_frame([KEY])
        pr = v.download_projection(KEY)
        off, lst = v.download_tile_lists(KEY)
        vis = v.models[KEY].visibility(transmittance=True)
        f = common.oracle_frame(S.scene(S.REF[name])[1], w, h)
        ref = R.walk(pr["mean2d"], pr["conic_opacity"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 1e-4, 0)
        dev_peak, dev_weight = R.check(ref, vis.peak, vis.weight, vis.pixels)
        print(f"visibility {name} {KIND_IDS[KINDS.index(kind)]}: L_max {ref.l_max}, uncertain {ref.uncertain.mean():.2%}, peak off by {dev_peak:.3e} "
              f"(bound {R.tol(ref.l_max):.3e}), weight off by {dev_weight:.3e} of its bound, pairs {vis.n_pairs}")
        assert vis.n_visible == pr_visible(pr) and vis.n_seen > 0
        if name == "long-list":
            assert ref.l_max > 256
        # 3. telescoping: every blended pair moves its weight from T into the sum
        assert vis.weight_fixed == int(np.round(vis.weight * 2.0 ** 24).sum()) and vis.n_pairs == int(vis.pixels.sum())
        lost = float((1.0 - vis.transmittance.astype(np.float64)).sum())
        assert abs(vis.weight_fixed / 2.0 ** 24 - lost) <= vis.n_pairs * (3 * 2.0 ** -24 + 2.0 ** -25)


def pr_visible(pr):
    return int((pr["key"] != 0xFFFFFFFF).sum())


# ---- 4. occlusion ------------------------------------------------------------------------------------------------------------------------
def test_an_opaque_wall_hides_what_stands_behind_it():
    cam = camera.orbit_pose(0)
    w, h = 80, 48
    g = common.small_scene(201, 91, 3, 2.0)
    V = np.asarray(cam.view(), np.float64).reshape(4, 4).T
    R_, t = V[:3, :3], V[:3, 3]
    eye, fwd = -R_.T @ t, -R_[2]
    # 200 Gaussians in a slab well behind the wall, the wall (index 200) between them and the camera
    rng = np.random.default_rng(5)
    local = np.stack([rng.uniform(-1.5, 1.5, 200), rng.uniform(-1.0, 1.0, 200), rng.uniform(6.0, 8.0, 200)], 1)
    g["pos"][:200] = (eye + local[:, :1] * R_[0] + local[:, 1:2] * R_[1] + local[:, 2:3] * fwd).astype(np.float32)
    g["scale"][:200] = 0.05
    g["pos"][200] = (eye + 3.0 * fwd).astype(np.float32)
    g["scale"][200] = (3000.0, 3000.0, 0.01)
    g["rot"][200] = _look_rot(R_)
    g["color"][200, 3] = 255
    behind = np.arange(201) < 200
    v = MultiModelViewer()
    with v:
        _load(v, g, KEY)
        v.update_camera(cam, (w, h))
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
        m = v.models[KEY]
        vis = m.visibility(transmittance=True)
        assert vis.peak[200] > 0.99 and vis.pixels[200] == w * h and (vis.transmittance < 1e-4).all(), "the wall covers the frame"
        assert not vis.peak[behind].any() and not vis.pixels[behind].any() and not vis.weight[behind].any()
        assert vis.n_seen == 1
        # with the wall masked out, every one of the 200 whose centre is on screen is seen
        m.gaussian_buffers.mask_buffer.upload(_words(behind))
        v.render_frame([KEY])
        pr = v.download_projection(KEY)
        vis = m.visibility()
        on_screen = behind & (pr["key"] != 0xFFFFFFFF) & (pr["mean2d"][:, 0] >= 0) & (pr["mean2d"][:, 0] < w) & (pr["mean2d"][:, 1] >= 0) & (pr["mean2d"][:, 1] < h)
        assert on_screen.sum() > 100 and (vis.peak[on_screen] > 0).all() and vis.peak[200] == 0 and vis.pixels[200] == 0


def _look_rot(R_):
    """the quaternion (x, y, z, w) of the rotation whose columns are the camera's right, up and backward axes: a Gaussian with it is
    flat towards the camera when its third scale is small"""
    m = R_.T  # columns: the view axes in world space
    w = np.sqrt(max(0.0, 1.0 + m[0, 0] + m[1, 1] + m[2, 2])) / 2.0
    if w > 1e-6:
        q = np.array([(m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w), w])
    else:  # a half turn: take the axis from the diagonal
        x = np.sqrt(max(0.0, (1 + m[0, 0]) / 2))
        y = np.sqrt(max(0.0, (1 + m[1, 1]) / 2)) * (1 if m[0, 1] >= 0 else -1)
        z = np.sqrt(max(0.0, (1 + m[2, 2]) / 2)) * (1 if m[0, 2] >= 0 else -1)
        q = np.array([x, y, z, 0.0])
    return (q / np.linalg.norm(q)).astype(np.float32)


# ---- 5. determinism and isolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [1, 2])
def test_two_calls_return_the_same_bytes_whatever_ran_before(in_flight):
    g, cam, size = S.scene(S.SOLID["partial"])
    v, _ = _open(S.SOLID["partial"], frames_in_flight=in_flight)
    with v:
        m = v.models[KEY]
        first = m.visibility(transmittance=True)
        assert _same(first, m.visibility(transmittance=True))
        for pose in (4, 5, 6, 7, 6):  # a camera path: the later frames are speculated, and dealt to the lanes
            v.update_camera(camera.orbit_pose(pose), size)
            v.render_frame([KEY])
        last = v.download_framebuffer()
        v.update_camera(cam, size)
        again = m.visibility(transmittance=True)
        assert _same(first, again)
        # the framebuffer downloaded after the call is the frame from before it (the camera's viewport is the same)
        assert np.array_equal(_bits(v.download_framebuffer()), _bits(last))


def test_the_next_frame_is_the_frame_without_the_call():
    g, cam, size = S.scene(S.SOLID["5x3"])
    frames = []
    for call in (False, True):
        v, _ = _open(S.SOLID["5x3"])
        with v:
            out = []
            for k, pose in enumerate((5, 6, 7, 8)):
                v.update_camera(camera.orbit_pose(pose), size)
                if call and k in (1, 3):
                    v.models[KEY].visibility()
                v.render_frame([KEY])
                out.append(v.download_framebuffer())
            frames.append(out)
    for a, b in zip(*frames):
        assert np.array_equal(_bits(a), _bits(b))


def test_render_needs_a_new_preprocess_and_sort_and_queries_keep_their_hits():
    v, g = _open(S.SOLID["5x3"])
    with v:
        v.update_query(query.QueryPod.hit((40.0, 24.0)))
        v.preprocessor.preprocess(KEY)
        v.radix_sorter.sort(KEY)
        v.renderer.render([KEY])
        v.postprocessor.postprocess(KEY)
        v.poll()
        hits = v.download_query_hits(KEY)
        fb = v.download_framebuffer()
        assert hits.shape[0] > 0
        v.models[KEY].visibility()
        assert np.array_equal(v.download_query_hits(KEY).tobytes(), hits.tobytes()) and np.array_equal(_bits(v.download_framebuffer()), _bits(fb))
        with pytest.raises(GsxError, match="not preprocessed"):
            v.renderer.render([KEY])
        with pytest.raises(GsxError):
            v.radix_sorter.sort(KEY)
        v.preprocessor.preprocess(KEY)
        v.radix_sorter.sort(KEY)
        v.renderer.render([KEY])
        assert np.array_equal(_bits(v.download_framebuffer()), _bits(fb))


# ---- 6. accumulate -------------------------------------------------------------------------------------------------------------------------
def test_accumulate_is_the_maximum_and_the_exact_sums():
    g, cam, size = S.scene(S.SOLID["partial"])
    views = [(cam, size), (camera.orbit_pose(17), (64, 40))]
    v, _ = _open(S.SOLID["partial"])
    with v:
        m = v.models[KEY]
        m.visibility()
        m.visibility_reset()
        base = device_bytes()
        single = []
        for c, s in views:
            v.update_camera(c, s)
            single.append(m.visibility())
            assert single[-1].views == 1, "without the flag a view replaces the planes"
        assert not _same(single[0], single[1])
        m.visibility_reset()
        assert device_bytes() == base
        v.update_camera(*views[0])
        a = m.visibility(accumulate=True)  # no planes yet: the first view
        assert _same(a, single[0])
        assert device_bytes() >= base + 16 * g.shape[0]
        v.update_camera(*views[1])
        b = m.visibility(accumulate=True)
        assert b.views == 2
        assert np.array_equal(_bits(b.peak), _bits(np.maximum(single[0].peak, single[1].peak)))
        assert np.array_equal(b.weight, single[0].weight + single[1].weight) and np.array_equal(b.pixels, single[0].pixels + single[1].pixels)
        assert (b.n_pairs, b.weight_fixed, b.n_visible) == (single[1].n_pairs, single[1].weight_fixed, single[1].n_visible), "the statistics are the view's"
        assert b.n_seen == int((b.peak > 0).sum()) and b.peak_max == b.peak.max()
        # the orbit helper: reset, then accumulate
        orbit = m.visibility_orbit([views[0][0], camera.orbit_pose(17)], size)
        assert orbit.views == 2 and v.size == tuple(size)
        v.update_camera(*views[1])
        assert m.visibility().views == 1
        m.visibility_reset()
        assert device_bytes() == base
        m.visibility_reset()  # nothing to free: fine


# ---- 7. select -----------------------------------------------------------------------------------------------------------------------------
def test_select_against_numpy_over_the_downloaded_planes():
    v, g = _open(S.SOLID["5x3"])
    n = g.shape[0]
    rng = np.random.default_rng(11)
    with v:
        m = v.models[KEY]
        vis = m.visibility()
        measures = {_lib.GSX_VIS_PEAK: vis.peak.astype(np.float64), _lib.GSX_VIS_WEIGHT: vis.weight, _lib.GSX_VIS_PIXELS: vis.pixels.astype(np.float64)}
        ranges = {_lib.GSX_VIS_PEAK: (0.05, 0.6), _lib.GSX_VIS_WEIGHT: (0.5, np.inf), _lib.GSX_VIS_PIXELS: (1.0, 40.0)}
        mask = rng.random(n) < 0.7
        m.gaussian_buffers.mask_buffer.upload(_words(mask))
        sel = np.zeros(n, bool)
        for measure, x in measures.items():
            lo, hi = ranges[measure]
            for op in (query.QuerySelectionOp.Set, query.QuerySelectionOp.Add, query.QuerySelectionOp.Remove):
                for flt in (0, _lib.GSX_BOUNDS_MASKED, _lib.GSX_BOUNDS_SELECTED):
                    passes = {0: np.ones(n, bool), _lib.GSX_BOUNDS_MASKED: mask, _lib.GSX_BOUNDS_SELECTED: sel}[flt]  # (the selection as it is now)
                    hit = passes & (x >= lo) & (x <= hi)
                    want = hit if op == query.QuerySelectionOp.Set else (sel | hit if op == query.QuerySelectionOp.Add else sel & ~hit)
                    got_hit, got_selected = m.select_visibility(measure, lo, hi, int(op), flt)
                    assert (got_hit, got_selected) == (int(hit.sum()), int(want.sum())), (measure, op, flt)
                    sel = want
                    assert np.array_equal(_selected(v, n), sel)
                    # an exact boundary is inside: [x_k, x_k]
                xs = np.sort(x[x > 0])
                assert m.select_visibility(measure, xs[0], xs[0], 0, 0)[0] == int((x == xs[0]).sum())
                sel = x == xs[0]
        # "never seen", then extract(SELECTED | INVERT): exactly the peak > 0 set
        m.gaussian_buffers.mask_buffer.upload(None)
        hit, selected = m.select_visibility(_lib.GSX_VIS_PEAK, 0.0, 0.0)
        assert hit == selected == int((vis.peak == 0).sum()) and 0 < hit < n
        kept = m.extract("seen", _lib.GSX_BOUNDS_SELECTED, invert=True)
        assert kept == int((vis.peak > 0).sum())
        pos = v.models["seen"].gaussian_buffers.gaussians_buffer.download_pod()[0]
        assert np.array_equal(pos, m.gaussian_buffers.gaussians_buffer.download_pod()[0][vis.peak > 0])


def test_select_over_257_partials():
    n = 262145  # 257 workgroups of the select, 257 partials of its finish
    g = common.small_scene(n, 13, 0, 3.0)
    v = MultiModelViewer(sh=ShKind.Norm8, cov3d=Cov3dKind.Half)
    with v:
        _load(v, g, KEY)
        v.update_camera(camera.orbit_pose(5), (16, 16))
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(0), False)
        m = v.models[KEY]
        vis = m.visibility()
        assert 0 < vis.n_seen < n
        for measure, x, lo, hi in ((_lib.GSX_VIS_PEAK, vis.peak.astype(np.float64), 1e-45, np.inf), (_lib.GSX_VIS_PIXELS, vis.pixels.astype(np.float64), 0.0, 0.0),
                                   (_lib.GSX_VIS_WEIGHT, vis.weight, float(np.median(vis.weight[vis.weight > 0])), np.inf)):
            want = (x >= lo) & (x <= hi)
            assert m.select_visibility(measure, lo, hi) == (int(want.sum()), int(want.sum()))
            assert np.array_equal(_selected(v, n), want)
        assert _selected(v, n)[-1] == bool(vis.weight[-1] >= float(np.median(vis.weight[vis.weight > 0]))), "the last Gaussian is the 257th group's only one"


# ---- 8. planes dropped ---------------------------------------------------------------------------------------------------------------------
def test_calls_that_rewrite_the_pod_planes_drop_the_planes():
    v, g = _open(S.SOLID["5x3"])
    n = g.shape[0]
    with v:
        m = v.models[KEY]
        base = None
        for drop in ("upload_range", "apply_transform", "set_pod_kind"):
            vis = m.visibility()
            if base is None:
                m.visibility_reset()
                base = device_bytes()
                vis = m.visibility()
            # a mask, a selection or an edit change keeps them
            m.gaussian_buffers.mask_buffer.upload(_words(np.arange(n) % 3 != 0))
            m.gaussian_buffers.selection_buffer.upload(_words(np.arange(n) % 2 == 0))
            m.gaussian_buffers.gaussians_edit_buffer.upload(query.default_edits(n))
            assert m.select_visibility(_lib.GSX_VIS_PEAK, 1e-45, np.inf)[0] == vis.n_seen
            assert m.apply_transform() == n, "the identity writes nothing"
            assert m.select_visibility(_lib.GSX_VIS_PEAK, 1e-45, np.inf)[0] == vis.n_seen
            m.gaussian_buffers.mask_buffer.upload(None)
            m.gaussian_buffers.gaussians_edit_buffer.upload(None)
            if drop == "upload_range":
                m.gaussian_buffers.gaussians_buffer.update_range(5, g[5:9])
            elif drop == "apply_transform":
                assert m.apply_transform(pos=(0.1, 0.0, 0.0)) == n
            else:
                m.set_pod_kind(ShKind.Half, Cov3dKind.Half)
                m = v.models[KEY]
            with pytest.raises(GsxError, match="no visibility planes") as e:
                m.select_visibility(_lib.GSX_VIS_PEAK, 0.0, 0.0)
            assert e.value.status == _lib.GSX_ERR_INVALID_ARG
        v.remove_model(KEY)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_message_and_the_planes_untouched():
    import torch

    v, g = _open(S.SOLID["5x3"])
    w, h = S.SOLID["5x3"][1:3]
    with v:
        m = v.models[KEY]
        L, hnd = v._L, v._h
        before = m.visibility()

        def refused(what, call=None):
            call = call or (lambda: m.visibility(accumulate=True))
            with pytest.raises(GsxError) as e:
                call()
            assert e.value.status == _lib.GSX_ERR_INVALID_ARG, what
            assert L.gsx_last_error_string(), what
            return L.gsx_last_error_string().decode()

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
        _lib.check(L.gsx_shard_set_windows(hnd, KEY.encode(), win.data_ptr()))
        assert "shard" in refused("sharded model")
        _lib.check(L.gsx_shard_set_windows(hnd, KEY.encode(), None))
        # the arguments
        d = _lib.VisibilityDesc(2)
        assert L.gsx_model_visibility(hnd, KEY.encode(), C.byref(d), None, None, None, None, None) == _lib.GSX_ERR_INVALID_ARG
        assert b"flag" in L.gsx_last_error_string()
        d = _lib.VisibilityDesc(0, (C.c_uint32 * 3)(0, 1, 0))
        assert L.gsx_model_visibility(hnd, KEY.encode(), C.byref(d), None, None, None, None, None) == _lib.GSX_ERR_INVALID_ARG
        d = _lib.VisibilityDesc(0)
        assert L.gsx_model_visibility(hnd, b"nobody", C.byref(d), None, None, None, None, None) == _lib.GSX_ERR_NOT_FOUND
        assert "measure" in refused("measure", lambda: m.select_visibility(3, 0.0, 1.0))
        assert "selection op" in refused("op", lambda: m.select_visibility(0, 0.0, 1.0, op=3))
        assert "range" in refused("reversed", lambda: m.select_visibility(0, 1.0, 0.5))
        assert "range" in refused("nan", lambda: m.select_visibility(0, float("nan"), 1.0))
        assert "filter" in refused("filter", lambda: m.select_visibility(0, 0.0, 1.0, filter=0x80))
        # a wrap of the pixel plane: (views + 1) * width * height >= 2^32
        v.update_camera(S.scene(S.SOLID["5x3"])[1], (65536, 32768))
        assert "wrap" in refused("wrap")
        v.update_camera(S.scene(S.SOLID["5x3"])[1], (w, h))
        # nothing of all that touched the planes
        assert m.select_visibility(_lib.GSX_VIS_PEAK, 1e-45, np.inf)[0] == before.n_seen
        after = m.visibility(accumulate=True)
        assert after.views == 2 and np.array_equal(after.pixels, 2 * before.pixels) and np.array_equal(_bits(after.peak), _bits(before.peak))
