"""Mask gizmos (gsx_viewer_set_mask_gizmos, spec §10) on the GPU.

The overlay is compared with the float64 restatement of the spec section (tests/gizmo_ref.py) away from the pixels that restatement
marks ambiguous: equal coverage, colour within 2e-6, depth within 5e-6 — §9's tolerances (measured on an MI355X over these scenes:
colour 6.1e-8, depth 1.2e-7 at the most, the near-clipped scenes included).  The splat frame needs none: under `Less` it is the frame of
a viewer without gizmos that was handed the effective depth E as the caller's depth buffer."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import common, gizmo_ref as G, overlay_ref as R
from wgpu_3dgs_viewer_app_amd import _lib, camera, query
from wgpu_3dgs_viewer_app_amd.query import QuerySelectionOp as Op
from wgpu_3dgs_viewer_app_amd.query import QueryToolsetTool as Tool
from wgpu_3dgs_viewer_app_amd.viewer import (DepthCompare, GaussianDisplayMode, GaussianShDegree, GsxError, MASK_GIZMO_DTYPE,
                                             MultiModelViewer)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_NAMES = tuple(G.scenes(*G.VIEWPORTS[0]))
COLOUR_TOL, DEPTH_TOL = 2e-6, 5e-6
BG = np.array([0.2, 0.5, 0.9], np.float32)
STROKE_RGBA = (1.0, 0.25, 0.0, 0.6)

_gaussians = {}


def _scene(seed, n=6000):
    if (seed, n) not in _gaussians:
        _gaussians[(seed, n)] = common.small_scene(n, seed, scale_mul=10.0)
    return _gaussians[(seed, n)]


def _viewer(**opts):
    v = MultiModelViewer()
    v.set_render_options(min_slab=2048, **opts)
    g = _scene(900)
    v.add_model("m", g.shape[0])
    v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
    return v


def _frame(v, cam, size):
    v.update_camera(cam, size)
    v.render_frame(["m"])
    v.poll()
    return v.download_framebuffer()


def _orbit(i):
    a = 0.12 * i
    return camera.CameraOrbitControl(target=np.zeros(3, np.float32), pos=np.array([5.0 * math.sin(a), 1.0, -5.0 * math.cos(a)], np.float32),
                                     z=(0.1, 20.0))


def _set(v, size, name, less=True):
    """the scene's gizmos, lines and depth buffer on a viewer -> its camera"""
    gizmos, lines, depth, cam, _ = G.reference(size, name)
    v.set_mask_gizmos(gizmos)
    v.update_hit_pairs(lines)
    if less and (len(gizmos) or len(lines) or depth is not None):
        v.set_depth_test(DepthCompare.Less)  # (legal without a caller buffer while gizmos or lines are set: D = 1)
    if depth is not None:
        v.update_depth_buffer(depth)
    return cam


def _launches(v, cam, size):
    L = _lib.load()
    before = L.gsx_debug_launch_count()
    fb = _frame(v, cam, size)
    return fb, L.gsx_debug_launch_count() - before


@pytest.mark.parametrize("name", SCENE_NAMES)
@pytest.mark.parametrize("size", G.VIEWPORTS)
def test_overlay_equals_the_restatement(size, name):
    w, h = size
    gizmos, lines, depth, _, ref = G.reference(size, name)
    with _viewer() as v:
        if name == "cleared":  # n = 0 after a set
            v.set_mask_gizmos(G.scenes(w, h)["box_trs"][0])
        cam = _set(v, size, name)
        _frame(v, cam, size)
        rgba, eff = v.download_overlay()
    d0 = np.ones((h, w), np.float32) if depth is None else depth
    cover = eff < d0
    clear = ~ref["ambiguous"]
    assert (ref["ambiguous"] & ref["cover"]).sum() <= G.AMBIGUOUS_CAP * max(int(ref["cover"].sum()), 1)
    wrong = (cover != ref["cover"]) & clear
    dc = np.abs(rgba.astype(np.float64) - ref["rgba"])[clear & ~wrong]
    dz = np.abs(eff.astype(np.float64) - ref["depth"])[clear & ~wrong]
    print(f"{name} {w}x{h}: covered {int(cover.sum())}, ambiguous {int(ref['ambiguous'].sum())}, coverage differs at {int(wrong.sum())}, "
          f"colour {dc.max():.2e}, depth {dz.max():.2e}")
    assert not wrong.any(), f"coverage differs at {int(wrong.sum())} unambiguous pixels, first (y, x) {np.argwhere(wrong)[:4].tolist()}"
    assert dc.max() <= COLOUR_TOL and dz.max() <= DEPTH_TOL
    # nothing drawn, nothing there: zero colour and E = D, bit for bit (tiles no record touches among them)
    assert not rgba[~cover].any() and np.array_equal(eff[~cover], d0[~cover])
    if name == "cleared":
        assert not cover.any()
    else:
        assert cover.sum() > 100


def test_shape_order_and_clipped_edges_show():
    size = G.VIEWPORTS[0]
    be, eb = G.reference(size, "box_ellipsoid_line_order")[4], G.reference(size, "ellipsoid_box_line_order")[4]
    assert np.abs(be["rgba"] - eb["rgba"]).max() > 0.05  # the two frames differ; each matched its own reference above
    with _viewer() as a, _viewer() as b:
        ca, cb = _set(a, size, "box_ellipsoid_line_order"), _set(b, size, "ellipsoid_box_line_order")
        _frame(a, ca, size)
        _frame(b, cb, size)
        assert np.abs(a.download_overlay()[0] - b.download_overlay()[0]).max() > 0.05
    segs = G.reference(size, "camera_inside_box")[4]["segments"]
    assert sum(1 for s in segs if s[3] > 0) >= 8 and sum(1 for s in segs if s[3] > 0 and s[2] == G.WHOLE) < 8


@pytest.mark.parametrize("name,size", [("box_ellipsoid_line_order", G.VIEWPORTS[0]), ("caller_plane", G.VIEWPORTS[1]),
                                       ("camera_inside_box", G.VIEWPORTS[1])])
def test_splat_frame_equals_the_frame_against_uploaded_E(name, size):
    _, _, depth, _, ref = G.reference(size, name)
    with _viewer() as a, _viewer() as b, _viewer() as c, _viewer() as plain:
        cam = _set(a, size, name)
        fa = _frame(a, cam, size)
        _, eff = a.download_overlay()
        for v, e in ((b, eff), (c, ref["depth"].astype(np.float32))):  # the library's own E: exact.  The restatement's: away from ambiguous pixels
            v.set_depth_test(DepthCompare.Less)
            v.update_depth_buffer(e)
        fb, fc = _frame(b, cam, size), _frame(c, cam, size)
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), f"L-inf {np.abs(fa - fb).max()}"
        clear = ~ref["ambiguous"]
        assert np.array_equal(fa[clear].view(np.uint32), fc[clear].view(np.uint32)), f"L-inf {np.abs(fa - fc)[clear].max()}"
        # GSX_DEPTH_ALWAYS: the gizmos are drawn all the same and the splat framebuffer is the untested one, bit for bit
        a.set_depth_test(DepthCompare.Always)
        f_always, f_plain = _frame(a, cam, size), _frame(plain, cam, size)
        assert np.array_equal(f_always.view(np.uint32), f_plain.view(np.uint32))
        if depth is None:
            assert np.array_equal(a.download_overlay()[1], eff)
        assert not np.array_equal(fa, f_plain)  # ... and under `Less` the gizmos hide splats


def test_batch_boxes_change_no_bit():
    """GSX_OVERLAY_BATCH_BOXES=0 (the flat walk) against the default, in child processes: colour, E, the `Less` frame and its sort count."""
    size = G.VIEWPORTS[0]
    names = ["ellipsoid_trs", "past_batch_64_tail", "past_batch_64_head", "random200"]
    got = []
    for value in (None, "0"):
        env = dict(os.environ)
        env.pop("GSX_OVERLAY_BATCH_BOXES", None)
        if value is not None:
            env["GSX_OVERLAY_BATCH_BOXES"] = value
        r = subprocess.run([sys.executable, "-m", "tests.gizmo_child", str(size[0]), str(size[1])] + names, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert got[0] == got[1], (got[0], got[1])
    assert all(got[0][n][4] > 100 for n in names)  # (something was drawn)


def test_launch_counts():
    size = G.VIEWPORTS[0]
    gizmos, lines = G.scenes(*size)["box_ellipsoid_line_order"][:2]
    with _viewer(speculative=0) as only, _viewer(speculative=0) as both, _viewer(speculative=0) as without, _viewer(speculative=0) as never:
        for v in (only, both, without, never):
            v.set_depth_test(DepthCompare.Less)
            v.update_depth_buffer(np.ones(size[::-1], np.float32))
        only.set_mask_gizmos(gizmos)
        both.set_mask_gizmos(gizmos)
        both.update_hit_pairs(lines)
        for i in range(2):
            for v, extra in ((only, 1), (both, 2)):
                _, n = _launches(v, _orbit(i), size)
                without.update_depth_buffer(v.download_overlay()[1])  # the same limits: the same frame behind them
                _, n0 = _launches(without, _orbit(i), size)
                assert n == n0 + extra, (i, extra, n, n0)  # the raster launch subsumes k_depth_limits: the set-up launches are the ones added
        both.set_mask_gizmos(None)
        both.update_hit_pairs(None)
        for i in range(3):  # cleared: the launches and the bits of a viewer that never set any
            (fa, na), (fb, nb) = _launches(both, _orbit(i), size), _launches(never, _orbit(i), size)
            assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and na == nb, (i, na, nb)
        rgba, eff = both.download_overlay()
        assert not rgba.any() and np.all(eff == 1.0)


def test_refusals():
    size = G.VIEWPORTS[0]
    gizmos = G.scenes(*size)["box_trs"][0]
    with _viewer(frames_in_flight=2) as v:
        with pytest.raises(GsxError, match="mask gizmos"):
            v.set_mask_gizmos(np.tile(gizmos, 257))  # n = 257
        v.set_mask_gizmos(np.tile(gizmos, 256))      # 256 are taken
        for field, value, what in (("kind", 2, "kind"), ("scale", np.float32([1.0, np.nan, 1.0]), "finite"), ("line_width", np.inf, "finite")):
            bad = np.tile(gizmos, 3)
            bad[field][1] = value
            with pytest.raises(GsxError, match=what):
                v.set_mask_gizmos(bad)
        L = v._L
        assert L.gsx_viewer_set_mask_gizmos(v._h, None, 1) == _lib.GSX_ERR_INVALID_ARG  # null with n > 0
        v.set_mask_gizmos(gizmos)
        v.update_camera(R.scene_camera(), size)
        # changed between preprocess and render: refused, as the lines and the depth calls are
        v.preprocessor.preprocess("m")
        v.radix_sorter.sort("m")
        v.set_mask_gizmos(gizmos[:1])
        with pytest.raises(GsxError, match="mask gizmos"):
            v.renderer.render(["m"])
        _frame(v, R.scene_camera(), size)  # (a whole frame is fine again)
        v.preprocessor.preprocess("m")
        v.radix_sorter.sort("m")
        v.set_mask_gizmos(None)  # cleared in between: refused as well
        with pytest.raises(GsxError, match="mask gizmos"):
            v.renderer.render(["m"])
        v.set_mask_gizmos(gizmos)
        # sharded frames, gsx_render_more, band frames and an external framebuffer; the message names both setters
        keys = (C.c_char_p * 1)(b"m")
        for status in (L.gsx_shard_set_windows(v._h, b"m", None), L.gsx_render_more(v._h, keys, 1), L.gsx_shard_frame_begin(v._h, b"m", 2, 0, 0, None)):
            msg = L.gsx_last_error_string()
            assert status == _lib.GSX_ERR_INVALID_ARG and b"gsx_viewer_set_mask_gizmos" in msg and b"gsx_viewer_set_overlay_lines" in msg
        _lib.check(L.gsx_viewer_set_band(v._h, 0, 2))
        with pytest.raises(GsxError, match="mask gizmos"):
            v.render_frame(["m"])
        _lib.check(L.gsx_viewer_set_band(v._h, 0, 0xFFFFFFFF))
        import torch

        ext = torch.empty(size[0] * size[1] * 4, dtype=torch.float32, device="cuda")
        _lib.check(L.gsx_viewer_set_external_framebuffer(v._h, ext.data_ptr(), ext.numel() * 4))
        with pytest.raises(GsxError, match="mask gizmos"):
            v.render_frame(["m"])
        _lib.check(L.gsx_viewer_set_external_framebuffer(v._h, None, 0))
        _frame(v, R.scene_camera(), size)
        assert all(v.overlay_device_ptrs())
    # (the refusal on a lane has no test: no public call hands out a lane's handle)


def test_two_frames_in_flight_match_the_one_lane_frame():
    size = G.VIEWPORTS[1]
    with _viewer(frames_in_flight=2) as two, _viewer(frames_in_flight=1) as one:
        cams = [_set(v, size, "box_ellipsoid_line_order") for v in (two, one)]
        for i in range(4):
            fa, fb = _frame(two, _orbit(i), size), _frame(one, _orbit(i), size)
            assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), i
            oa, ob = two.download_overlay(), one.download_overlay()
            assert np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1]) and (oa[1] < 1.0).sum() > 100
        assert cams[0] is not None


def _resolved(fb, overlay):
    """the float colour the resolve rounds, float64 [h, w, 4]: rgb + T (C + (1 - A) background), alpha 1 - T (1 - A)"""
    fb, o = fb.astype(np.float64), overlay.astype(np.float64)
    t = fb[..., 3:4]
    rgb, alpha = fb[..., :3] + t * (o[..., :3] + (1.0 - o[..., 3:4]) * BG.astype(np.float64)), 1.0 - t * (1.0 - o[..., 3:4])
    return np.clip(np.concatenate([rgb, alpha], axis=2), 0.0, 1.0)


def test_resolve_goes_over_the_gizmos_with_and_without_a_stroke():
    size = G.VIEWPORTS[1]
    w, h = size
    with _viewer() as v:
        cam = _set(v, size, "box_ellipsoid_line_order")
        fb = _frame(v, cam, size)
        rgba, _ = v.download_overlay()
        col = _resolved(fb, rgba)
        base = v.download_rgba8(BG)
        assert np.abs(base.astype(np.float64) - np.floor(col * 255.0 + 0.5)).max() <= 1  # k_resolve_rgba8's rounding
        assert (rgba[..., 3] > 0).sum() > 300 and (fb[..., 3] > 0.05).sum() > 100  # (gizmos there, and seen through the splats somewhere)
        t = query.DeviceQueryToolset(v)
        v.set_toolset_overlay(STROKE_RGBA, (0.1, 1.0, 0.3, 0.75), 2.5)
        t.update_brush_radius(6.3)
        t.start(Tool.Brush, Op.Set, (12.2, 14.1))
        for p in ((30.4, 22.7), (55.3, 20.2), (w - 4.4, h - 6.6)):
            t.update_pos(p)
        t.render()
        tex = v.download_query_texture() != 0
        got = v.download_rgba8(BG)
        s = np.array(STROKE_RGBA, np.float32).astype(np.float64)
        over = col * (1.0 - s[3])
        over[..., :3] += s[:3] * s[3]
        over[..., 3] += s[3]
        want = np.where(tex[..., None], np.floor(over * 255.0 + 0.5), base.astype(np.float64))
        assert tex.sum() > 200 and (tex & (rgba[..., 3] > 0)).sum() > 20  # the stroke crosses the gizmos
        assert np.abs(got.astype(np.float64) - want).max() <= 1
        assert np.array_equal(got[~tex], base[~tex])
