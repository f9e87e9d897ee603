"""Overlay lines (gsx_viewer_set_overlay_lines, spec §9: the app's measurement pass) on the GPU.

The overlay itself is compared with the float64 restatement of the spec section (tests/overlay_ref.py) away from the pixels that
restatement marks ambiguous: equal coverage, colour within 2e-6, depth within 5e-6 (ten times the float32-against-float64 deviation
of the restatement on the CPU; the room is for another FMA contraction).  The splat frame needs no tolerance: a frame rendered with
lines under `Less` is, bit for bit, the frame of a viewer without lines that was handed the downloaded effective depth E as the
caller's depth buffer."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from tests import common, overlay_ref as R
from wgpu_3dgs_viewer_app_amd import _lib, camera
from wgpu_3dgs_viewer_app_amd.viewer import (DepthCompare, GaussianDisplayMode, GaussianShDegree, GsxError, HIT_PAIR_DTYPE, HitPair,
                                             MultiModelViewer)

pytestmark = pytest.mark.gpu
SCENE_NAMES = tuple(R.scenes(*R.VIEWPORTS[0]))
COLOUR_TOL, DEPTH_TOL = 2e-6, 5e-6

_gaussians = {}


def _scene(seed, n=6000):
    if (seed, n) not in _gaussians:
        _gaussians[(seed, n)] = common.small_scene(n, seed, scale_mul=10.0)
    return _gaussians[(seed, n)]


def _viewer(keys=("m",), **opts):
    v = MultiModelViewer()
    v.set_render_options(min_slab=2048, **opts)
    for i, k in enumerate(keys):
        g = _scene(900 + i)
        v.add_model(k, g.shape[0])
        v.models[k].gaussian_buffers.gaussians_buffer.update_range(0, g)
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
    return v


def _frame(v, cam, size, keys=("m",), staged=False):
    v.update_camera(cam, size)
    if staged:
        for k in keys:
            v.preprocessor.preprocess(k)
            v.radix_sorter.sort(k)
        v.poll()
        v.renderer.render(list(keys))
    else:
        v.render_frame(list(keys))
    v.poll()
    return v.download_framebuffer()


def _orbit(i):
    """the scenes' camera, swung about the origin"""
    a = 0.12 * i
    return camera.CameraOrbitControl(target=np.zeros(3, np.float32), pos=np.array([5.0 * math.sin(a), 1.0, -5.0 * math.cos(a)], np.float32),
                                     z=(0.1, 20.0))


_reference = {}


def _ref(size, name):
    """the restatement of one scene, computed once and shared (read-only)"""
    if (size, name) not in _reference:
        w, h = size
        lines, depth = R.scenes(w, h)[name]
        view, proj = R.matrices(w, h)
        r = R.draw(lines, view, proj, w, h, depth)
        for a in r.values():
            a.setflags(write=False)
        _reference[(size, name)] = (lines, depth, r)
    return _reference[(size, name)]


@pytest.mark.parametrize("name", SCENE_NAMES)
@pytest.mark.parametrize("size", R.VIEWPORTS)
def test_overlay_equals_the_restatement(size, name):
    w, h = size
    lines, depth, ref = _ref(size, name)
    with _viewer() as v:
        v.update_hit_pairs(lines)
        if len(lines):
            v.set_depth_test(DepthCompare.Less)  # (legal without a caller buffer while lines are set: D = 1)
        if depth is not None:
            v.update_depth_buffer(depth)
        _frame(v, R.scene_camera(), size)
        rgba, eff = v.download_overlay()
    d0 = np.ones((h, w), np.float32) if depth is None else depth
    cover = eff < d0
    clear = ~ref["ambiguous"]
    assert ref["ambiguous"].sum() <= R.AMBIGUOUS_CAP * max(int(ref["cover"].sum()), 1)
    wrong = (cover != ref["cover"]) & clear
    assert not wrong.any(), f"coverage differs at {int(wrong.sum())} unambiguous pixels, first (y, x) {np.argwhere(wrong)[:4].tolist()}"
    dc = np.abs(rgba.astype(np.float64) - ref["rgba"])[clear]
    dz = np.abs(eff.astype(np.float64) - ref["depth"])[clear]
    print(f"{name} {w}x{h}: covered {int(cover.sum())}, ambiguous {int(ref['ambiguous'].sum())}, colour {dc.max():.2e}, depth {dz.max():.2e}")
    assert dc.max() <= COLOUR_TOL and dz.max() <= DEPTH_TOL
    # nothing drawn, nothing there: zero colour and E = D, bit for bit (tiles no line touches among them)
    assert not rgba[~cover].any() and np.array_equal(eff[~cover], d0[~cover])
    if name == "diagonal_alpha128":  # one line: every covered pixel — the ambiguous ones, the shared diagonal, the tile seams — is blended ONCE
        assert cover.sum() > 150 and np.all(rgba[cover][:, 3] == np.float32(128) / np.float32(255))
    if name in ("end_behind_eye", "zero_length"):  # the first line is not drawn: the scene is the second one alone
        with _viewer() as v:
            v.update_hit_pairs(lines[1:])
            _frame(v, R.scene_camera(), size)
            alone = v.download_overlay()
        assert np.array_equal(alone[0], rgba) and np.array_equal(alone[1], eff)
    if name == "empty":
        assert not cover.any()


def test_crossing_lines_blend_in_array_order():
    size = R.VIEWPORTS[0]
    ab, ba = _ref(size, "crossing_ab")[2], _ref(size, "crossing_ba")[2]
    assert np.abs(ab["rgba"] - ba["rgba"]).max() > 0.05  # (the scene pair is order-dependent at all: the nearer line first hides the other)


def test_always_draws_the_lines_behind_every_splat():
    size = R.VIEWPORTS[1]
    lines = R.scenes(*size)["crossing_ab"][0]
    with _viewer() as v, _viewer() as plain:
        v.update_hit_pairs(lines)
        a = _frame(v, R.scene_camera(), size)
        always = v.download_overlay()
        b = _frame(plain, R.scene_camera(), size)
        assert np.array_equal(a, b)  # the (rgb, T) frame is the frame without lines
        v.set_depth_test(DepthCompare.Less)
        c = _frame(v, R.scene_camera(), size)
        less = v.download_overlay()
        assert np.array_equal(always[0], less[0]) and np.array_equal(always[1], less[1]) and (always[0][..., 3] > 0).sum() > 100
        assert not np.array_equal(a, c)  # ... and under `Less` the lines hide splats


VARIANTS = {
    "plain": dict(opts=dict(speculative=0)),
    "speculated": dict(opts=dict()),
    "not_progressive": dict(opts=dict(progressive=0, speculative=0)),
    "two_models": dict(opts=dict(), keys=("m", "n")),
    "staged": dict(opts=dict(), staged=True),
    "in_flight": dict(opts=dict(frames_in_flight=2)),
}


@pytest.mark.parametrize("caller_buffer", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_splat_frame_equals_the_frame_against_uploaded_E(variant, caller_buffer):
    """Exact by construction: the splats are tested against E, whoever made it."""
    cfg = VARIANTS[variant]
    keys, staged = cfg.get("keys", ("m",)), cfg.get("staged", False)
    size = R.VIEWPORTS[1] if caller_buffer else R.VIEWPORTS[0]
    w, h = size
    lines, plane = R.scenes(w, h)["caller_plane"]
    lines = np.concatenate([lines, R.scenes(w, h)["random200"][0][:80]])
    speculated = 0
    with _viewer(keys, **cfg["opts"]) as a, _viewer(keys, **cfg["opts"]) as b:
        a.set_depth_test(DepthCompare.Less)
        b.set_depth_test(DepthCompare.Less)
        a.update_hit_pairs(lines)
        if caller_buffer:
            a.update_depth_buffer(plane)
        for i in range(6):
            cam = _orbit(i)
            fa = _frame(a, cam, size, keys, staged)
            _, eff = a.download_overlay()
            assert (eff < (plane if caller_buffer else 1.0)).sum() > 100
            b.update_depth_buffer(eff)
            fb = _frame(b, cam, size, keys, staged)
            assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), f"{variant}, frame {i}: L-inf {np.abs(fa - fb).max()}"
            speculated += a.frame_stats(keys[0])["speculated"]
        if variant == "speculated":
            assert speculated > 0


def test_resolve_goes_over_the_overlay():
    size = R.VIEWPORTS[1]
    lines = R.scenes(*size)["random200"][0]
    bg = np.array([0.2, 0.5, 0.9], np.float32)
    with _viewer() as v:
        v.set_depth_test(DepthCompare.Less)
        v.update_hit_pairs(lines)
        fb = _frame(v, R.scene_camera(), size).astype(np.float64)
        rgba, _ = v.download_overlay()
        got = v.download_rgba8(bg)
    o = rgba.astype(np.float64)
    t = fb[..., 3:4]
    rgb = fb[..., :3] + t * (o[..., :3] + (1.0 - o[..., 3:4]) * bg.astype(np.float64))
    alpha = 1.0 - t * (1.0 - o[..., 3:4])
    want = np.floor(np.clip(np.concatenate([rgb, alpha], axis=2), 0.0, 1.0) * 255.0 + 0.5)
    assert np.abs(got.astype(np.float64) - want).max() <= 1
    assert (o[..., 3] > 0).sum() > 500 and (t[..., 0] > 0.05).sum() > 100  # (lines there, and seen through the splats somewhere)


def test_errors_name_the_overlay():
    size = R.VIEWPORTS[0]
    lines = R.scenes(*size)["crossing_ab"][0]
    with _viewer() as v:
        with pytest.raises(GsxError, match="overlay lines"):
            v.update_hit_pairs(np.zeros(4097, HIT_PAIR_DTYPE))
        v.update_hit_pairs(np.tile(lines, 2048))  # 4096 are taken
        v.update_hit_pairs(lines)
        v.update_camera(R.scene_camera(), size)
        # changed between preprocess and render: refused, as the depth calls are
        v.preprocessor.preprocess("m")
        v.radix_sorter.sort("m")
        v.update_hit_pairs(lines[:1])
        with pytest.raises(GsxError, match="overlay"):
            v.renderer.render(["m"])
        _frame(v, R.scene_camera(), size)  # (a whole frame is fine again)
        v.preprocessor.preprocess("m")
        v.radix_sorter.sort("m")
        v.update_hit_pairs(None)  # cleared in between: refused as well
        with pytest.raises(GsxError, match="overlay"):
            v.renderer.render(["m"])
        v.update_hit_pairs(lines)
        # sharded frames, gsx_render_more, band frames and an external framebuffer
        L, keys = v._L, (C.c_char_p * 1)(b"m")
        for status in (L.gsx_shard_set_windows(v._h, b"m", None), L.gsx_render_more(v._h, keys, 1),
                       L.gsx_shard_frame_begin(v._h, b"m", 2, 0, 0, None)):
            assert status == _lib.GSX_ERR_INVALID_ARG and b"overlay" in L.gsx_last_error_string()
        _lib.check(L.gsx_viewer_set_band(v._h, 0, 2))
        with pytest.raises(GsxError, match="overlay"):
            v.render_frame(["m"])
        _lib.check(L.gsx_viewer_set_band(v._h, 0, 0xFFFFFFFF))
        import torch

        ext = torch.empty(size[0] * size[1] * 4, dtype=torch.float32, device="cuda")
        _lib.check(L.gsx_viewer_set_external_framebuffer(v._h, ext.data_ptr(), ext.numel() * 4))
        with pytest.raises(GsxError, match="overlay"):
            v.render_frame(["m"])
        _lib.check(L.gsx_viewer_set_external_framebuffer(v._h, None, 0))
        _frame(v, R.scene_camera(), size)
        ptrs = v.overlay_device_ptrs()
        assert all(ptrs)


def _launches(v, cam, size):
    L = _lib.load()
    before = L.gsx_debug_launch_count()
    fb = _frame(v, cam, size)
    return fb, L.gsx_debug_launch_count() - before


@pytest.mark.parametrize("compare", [DepthCompare.Always, DepthCompare.Less])
def test_no_cost_when_unused(compare):
    size = R.VIEWPORTS[0]
    lines = R.scenes(*size)["crossing_ab"][0]
    with _viewer() as used, _viewer() as never:
        for v in (used, never):
            v.set_depth_test(compare)
            v.update_depth_buffer(np.full(size[::-1], 0.9805, np.float32))
        used.update_hit_pairs(lines)
        used.update_hit_pairs(None)
        for i in range(4):
            (fa, na), (fb, nb) = _launches(used, _orbit(i), size), _launches(never, _orbit(i), size)
            assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and na == nb, (i, na, nb)
        rgba, eff = used.download_overlay()  # a frame without lines has no overlay: zeros, and E = D
        assert not rgba.any() and np.all(eff == np.float32(0.9805))


def test_lines_add_one_launch_to_a_depth_tested_frame():
    size = R.VIEWPORTS[0]
    lines = R.scenes(*size)["random200"][0]
    with _viewer(speculative=0) as with_lines, _viewer(speculative=0) as without:
        for v in (with_lines, without):
            v.set_depth_test(DepthCompare.Less)
            v.update_depth_buffer(np.ones(size[::-1], np.float32))
        with_lines.update_hit_pairs(lines)
        for i in range(3):
            _, na = _launches(with_lines, _orbit(i), size)
            without.update_depth_buffer(with_lines.download_overlay()[1])  # the same limits: the same frame behind them
            _, nb = _launches(without, _orbit(i), size)
            # the raster launch subsumes k_depth_limits: the set-up launch is the one added
            assert na == nb + 1, (i, na, nb)
