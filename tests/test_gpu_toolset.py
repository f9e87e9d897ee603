"""GPU: the query toolset in the library (spec §7 "Toolset"; gsx_toolset_*, kernels_toolset.hip).

The strokes k_toolset_paint leaves in the query texture against query.QueryToolset's float64 texture (tests/toolset_cases.py: every texel
further than 1e-3 px from a cut must match), rendered step by step and all at once; a drag as the app runs it on two lanes, never handing
the library a host texture, against a plain viewer with the host toolset and the upload; the stroke overlay and the cursor in the RGBA8
resolve against a numpy restatement of the blend; and nothing at all — launches, bytes — while nothing of the toolset is set."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from tests import common, overlay_ref as R, toolset_cases as tc
from tests import test_gpu_query_paths as qp
from wgpu_3dgs_viewer_app_amd import _lib, camera, query, viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd._lib import GsxError
from wgpu_3dgs_viewer_app_amd.query import QuerySelectionOp as Op
from wgpu_3dgs_viewer_app_amd.query import QueryToolsetTool as Tool
from wgpu_3dgs_viewer_app_amd.viewer import GaussianDisplayMode, GaussianShDegree, MultiModelViewer

pytestmark = pytest.mark.gpu
BG = np.array([0.2, 0.5, 0.9], np.float32)
STROKE_RGBA, CURSOR_RGBA, THICKNESS = (1.0, 0.25, 0.0, 0.6), (0.1, 1.0, 0.3, 0.75), 2.5


# ---------------------------------------------------------------- 1. texture parity
@functools.lru_cache(maxsize=None)
def _painted(name, size):
    """(rendered after every step, every step queued before one render): the device's texture either way"""
    out = []
    for per_step in (True, False):
        with MultiModelViewer() as v:
            v.update_camera(camera.orbit_pose(3), size)
            t = query.DeviceQueryToolset(v)
            tc.play(t, tc.CASES[name], after_each=t.render if per_step else None)
            t.render()
            tex = t.texture
            tex.setflags(write=False)
            out.append(tex)
    return tuple(out)


@pytest.mark.parametrize("name,size", [(n, tc.SIZES[0]) for n in tc.CASES] + [("drag", tc.SIZES[1])], ids=lambda p: p if isinstance(p, str) else f"{p[0]}x{p[1]}")
def test_texture_equals_query_toolset(name, size):
    per_step, at_once = _painted(name, size)
    tc.assert_matches(per_step, name, size, "a render per step: ")
    tc.assert_matches(at_once, name, size, "one render: ")
    assert np.array_equal(per_step, at_once), "queueing every step before one render painted other bytes than a render per step"
    painted = tc.EXPECTED.get(name, (None, None))[0] if size == tc.SIZES[0] else None
    if painted in (0, 1, size[0] * size[1]):   # nothing, one texel, everything: no cut near a centre
        assert int((at_once != 0).sum()) == painted


def test_viewport_change_clears_and_resizes():
    a, b = tc.SIZES
    with MultiModelViewer() as v:
        t = query.DeviceQueryToolset(v)
        v.update_camera(camera.orbit_pose(3), a)
        tc.play(t, tc.CASES["drag"])
        t.render()
        v.update_camera(camera.orbit_pose(3), b)
        t.render()                                     # update_query_texture_size: the new texture holds nothing
        assert t.texture.shape == (b[1], b[0]) and not t.texture.any()
        tc.play(t, tc.CASES["drag"])
        t.render()
        tc.assert_matches(t.texture, "drag", b)
        v.update_camera(camera.orbit_pose(3), a)
        tc.play(t, tc.CASES["drag"][:2])               # back again, straight into a stroke: the disc start() paints lands on a cleared texture
        t.render()
        first = t.texture
        assert first.shape == (a[1], a[0]) and 200 < (first != 0).sum() < 320
        tc.play(t, tc.CASES["drag"][2:])
        t.render()
        tc.assert_matches(t.texture, "drag", a)


# ---------------------------------------------------------------- 2. the drag as the app runs it
def test_drag_on_two_lanes_without_a_host_texture():
    """The new counterpart of test_gpu_query_paths.test_drag_with_the_toolset_on_two_lanes: the two-lane viewer paints on the device
    (update_pos + render every frame, never gsx_update_query_texture), the plain viewer has the host toolset and uploads what it paints."""
    pod = "single_single"
    ref = qp._reference(pod)
    path = [(30.5, 40.0), (55.0, 52.25), (80.0, 47.0), (110.5, 70.0), (140.0, 95.75), (150.0, 100.0)]
    lanes, plain = qp._viewer(pod, frames_in_flight=2), qp._viewer(pod, speculative=0, slab_shading=0)
    dev, host = query.DeviceQueryToolset(lanes), query.QueryToolset((qp.W, qp.H))
    for t in (dev, host):
        t.update_brush_radius(9.5)
    uploads = []

    def frame(what, during_drag=False):
        """one frame of the app's loop on both viewers -> the two-lane viewer's query"""
        dev.render()                                   # query_toolset.render every frame, stroke or not (scene.rs:791)
        qd, qh = dev.query(), host.query()
        assert (qd.kind, qd.op) == (qh.kind, qh.op), what
        if during_drag or qh.kind == query.QueryKind.Texture:
            plain.update_query_texture(host.texture)   # what a host has to do without the device toolset
            uploads.append(what)
        lanes.update_query(qd)
        plain.update_query(qh)
        a, b = qp._frame(lanes)[0], qp._frame(plain)[0]
        assert np.array_equal(a, b), f"{what}: the two-lane frame differs from the plain viewer's, L-inf {np.abs(a - b).max()}"
        for v in (lanes, plain):
            for k in qp.KEYS:
                v.postprocessor.postprocess(k)
        return qd

    for i in range(4):                                 # every lane has rendered twice: both speculate from here on
        frame(f"before the drag {i}")
    assert all(lanes.frame_stats(k)["speculated"] for k in qp.KEYS)
    for t in (dev, host):
        t.start(Tool.Brush, Op.Add, path[0])
    for i, p in enumerate(path[1:]):
        for t in (dev, host):
            t.update_pos(p)
        q = frame(f"drag step {i}", during_drag=True)
        assert q.kind == query.QueryKind.None_
        assert all(lanes.frame_stats(k)["speculated"] == 1 for k in qp.KEYS), f"drag step {i}: a paint threw the lanes back to plain frames"
        assert dev.state() == (Tool.Brush, Op.Add, path[0], p)
    for t in (dev, host):
        t.end()
    q_tex = frame("end of the drag")
    assert q_tex.kind == query.QueryKind.Texture and q_tex.op == Op.Add
    tex = lanes.download_query_texture()
    ops = [("radius", 9.5), ("start", Tool.Brush, Op.Add, path[0])] + [("pos", p) for p in path[1:]]
    amb = tc.ambiguous(ops, (qp.W, qp.H))
    assert np.array_equal(tex[~amb], host.texture[~amb]) and 0.05 < (tex != 0).mean() < 0.5
    assert amb.sum() <= tc.AMBIGUOUS_CAP * (host.texture != 0).sum()
    n_sel = 0
    for k in qp.KEYS:
        got = lanes.models[k].gaussian_buffers.selection_buffer.download()
        assert np.array_equal(got, plain.models[k].gaussian_buffers.selection_buffer.download()), f"model {k}: selection differs from the host toolset's"
        if not amb.any():
            assert np.array_equal(got, oracle.query_flags(ref[k]["pr"], q_tex, host.texture)), f"model {k}: selection differs from the oracle's"
        assert np.array_equal(got, oracle.query_flags(ref[k]["pr"], q_tex, tex)), f"model {k}: selection differs from the oracle's on the device's own texture"
        n_sel += int(qp.qc.unpack_bits(got, qp.SIZES[k][0]).sum())
    assert n_sel > 500
    frame("idle after the drag")
    assert dev.query().kind == query.QueryKind.None_ and dev.state() is None
    for v in (lanes, plain):
        v.update_selection_edit_with_pod(qp.HSV_EDIT)
    frame("edited selection")
    frame("edited selection, next frame")
    assert all(lanes.frame_stats(k)["speculated"] for k in qp.KEYS), "the frames after the drag are speculated again"
    assert len(uploads) == len(path), uploads
    for v in (lanes, plain):
        v.close()


# ---------------------------------------------------------------- 3. nothing set, nothing changed
def _small_viewer(**opts):
    v = MultiModelViewer()
    v.set_render_options(min_slab=2048, **opts)
    g = _scene()
    v.add_model("m", g.shape[0])
    v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
    return v


@functools.lru_cache(maxsize=None)
def _scene():
    g = common.small_scene(6000, 900, scale_mul=10.0)
    g.setflags(write=False)
    return g


def _frame_and_resolve(v, i, size):
    """-> (launches of the frame and its resolve, rgba8)"""
    v.update_camera(R.scene_camera() if i is None else camera.orbit_pose(10 + i), size)
    n0 = viewer_mod.launch_count()
    v.render_frame(["m"])
    px = v.download_rgba8(BG)
    return viewer_mod.launch_count() - n0, px


def test_nothing_set_nothing_changed():
    size = tc.SIZES[0]
    with _small_viewer() as never, _small_viewer() as zero, _small_viewer() as used:
        zero.set_toolset_overlay((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), 3.0)     # both alphas 0, no toolset call
        t = query.DeviceQueryToolset(used)
        for i in range(5):
            na, a = _frame_and_resolve(never, i, size)
            nz, z = _frame_and_resolve(zero, i, size)
            assert na == nz, f"frame {i}: {nz} launches with alpha-0 colours set, {na} on a viewer that never heard of the toolset"
            assert np.array_equal(a, z)
            if i == 1:
                t.start(Tool.Brush, Op.Set, (40.2, 25.1))
            elif i > 1:
                t.update_pos((40.2 + 7 * i, 25.1 + 3 * i))
            t.render()
            _, u = _frame_and_resolve(used, i, size)
            assert np.array_equal(a, u), f"frame {i}: toolset calls with alpha 0 changed the resolved frame"
        assert used.download_query_texture().any()


def test_paints_between_recorded_frames():
    """With launch graphs on (frames recorded and submitted as HIP graphs) a paint between two frames is submitted where it was asked
    for: the texture, the frames and the graph statistics' launch totals are what they are without graphs, plus one launch per paint."""
    size = tc.SIZES[1]
    ops = tc.CASES["drag"]
    got = {}
    try:
        for graphs in (0, 2):   # 2: record even when the stream is idle (this loop reads every frame back)
            viewer_mod.set_launch_graphs(graphs)
            with _small_viewer() as v:
                t = query.DeviceQueryToolset(v)
                frames, n0 = [], viewer_mod.launch_count()
                for i, o in enumerate(ops):
                    tc.play(t, [o])
                    t.render()
                    v.update_camera(camera.orbit_pose(10 + i), size)
                    v.render_frame(["m"])
                    frames.append(v.download_framebuffer())
                got[graphs] = (t.texture, frames, viewer_mod.launch_count() - n0, v.launch_stats()["graph_launches"])
    finally:
        viewer_mod.set_launch_graphs(0)
    tc.assert_matches(got[2][0], "drag", size)
    assert np.array_equal(got[0][0], got[2][0])
    assert all(np.array_equal(a, b) for a, b in zip(got[0][1], got[2][1]))
    assert got[0][2] == got[2][2] and got[0][3] == 0 and got[2][3] > 0, (got[0][2:], got[2][2:])


# ---------------------------------------------------------------- 4. overlay and cursor in the resolve
def _resolved(fb, overlay=None):
    """the float colour the resolve rounds, float64 [h, w, 4]"""
    fb = fb.astype(np.float64)
    t = fb[..., 3:4]
    if overlay is None:
        rgb, alpha = fb[..., :3] + t * BG.astype(np.float64), 1.0 - t
    else:
        o = overlay.astype(np.float64)
        rgb, alpha = fb[..., :3] + t * (o[..., :3] + (1.0 - o[..., 3:4]) * BG.astype(np.float64)), 1.0 - t * (1.0 - o[..., 3:4])
    return np.clip(np.concatenate([rgb, alpha], axis=2), 0.0, 1.0)


def _blend(col, rgba):
    c = np.array(rgba, np.float32).astype(np.float64)
    out = col * (1.0 - c[3])
    out[..., :3] += c[:3] * c[3]
    out[..., 3] += c[3]
    return out


def _round8(col):
    return np.floor(col * 255.0 + 0.5)


def _check_drawn(got, base, col, cover, amb, rgba, what):
    """got: the resolve with the toolset drawn; base: without; col: the float colour under it; cover / amb: bool [h, w]"""
    assert amb.sum() <= tc.AMBIGUOUS_CAP * cover.sum(), f"{what}: {amb.sum()} of {cover.sum()} drawn pixels are ambiguous: move the case"
    assert cover.sum() > 20, what
    want = _round8(_blend(col, rgba))
    err = np.abs(got.astype(np.float64) - want).max(axis=2)
    sure = cover & ~amb
    assert err[sure].max() <= 1, f"{what}: {(err[sure] > 1).sum()} drawn pixels are off by more than 1, worst {err[sure].max()}"
    clear = ~cover & ~amb
    assert np.array_equal(got[clear], base[clear]), f"{what}: {(got[clear] != base[clear]).any(axis=1).sum()} pixels outside differ from the plain resolve"
    either = np.minimum(err, np.abs(got.astype(np.float64) - base.astype(np.float64)).max(axis=2))
    assert either[amb].max(initial=0) <= 1, f"{what}: an ambiguous pixel is neither drawn nor plain"
    assert (got[sure] != base[sure]).any(), f"{what}: nothing shows"


def _centres(size):
    yy, xx = np.mgrid[0:size[1], 0:size[0]]
    return xx + 0.5, yy + 0.5


def _ring(size, pos, radius):
    px, py = _centres(size)
    off = np.abs(np.hypot(px - np.float32(pos[0]), py - np.float32(pos[1])) - np.float32(radius)) - 0.5 * np.float32(THICKNESS)
    return off <= 0, np.abs(off) <= tc.AMBIGUOUS_PX


def _outline(size, p, q):
    px, py = _centres(size)
    x0, x1 = sorted((float(np.float32(p[0])), float(np.float32(q[0]))))
    y0, y1 = sorted((float(np.float32(p[1])), float(np.float32(q[1]))))
    outside = np.maximum(np.maximum(x0 - px, px - x1), np.maximum(y0 - py, py - y1))          # > 0 outside: the Chebyshev distance
    inside = np.minimum(np.minimum(px - x0, x1 - px), np.minimum(py - y0, y1 - py))           # > 0 inside: distance to the nearest edge
    off = np.where(outside > 0, outside, inside) - 0.5 * np.float32(THICKNESS)
    return off <= 0, np.abs(off) <= tc.AMBIGUOUS_PX


@pytest.mark.parametrize("size,lines", [(tc.SIZES[0], False), (tc.SIZES[1], False), (tc.SIZES[0], True)], ids=["83x51", "96x64", "83x51_overlay_lines"])
def test_stroke_overlay_and_cursor_in_the_resolve(size, lines):
    w, h = size
    with _small_viewer() as v:
        if lines:
            v.update_hit_pairs(R.scenes(w, h)["random200"][0])
        _, base = _frame_and_resolve(v, None, size)
        col = _resolved(v.download_framebuffer(), v.download_overlay()[0] if lines else None)
        assert np.abs(base.astype(np.float64) - _round8(col)).max() <= 1
        if lines:
            assert (v.download_overlay()[0][..., 3] > 0).sum() > 300
        t = query.DeviceQueryToolset(v)
        v.set_toolset_overlay(STROKE_RGBA, CURSOR_RGBA, THICKNESS)
        assert np.array_equal(v.download_rgba8(BG), base), "no position reported yet: nothing is drawn"
        # the stroke, while it is drawn
        t.update_brush_radius(6.3)
        t.start(Tool.Brush, Op.Set, (12.2, 14.1))
        for p in ((30.4, 22.7), (55.3, 20.2), (w - 4.4, h - 6.6)):
            t.update_pos(p)
        t.render()
        tex = v.download_query_texture()
        got = v.download_rgba8(BG)
        _check_drawn(got, base, col, tex != 0, np.zeros((h, w), bool), STROKE_RGBA, "stroke overlay")
        # a row range that starts inside a tile equals the same rows of the full resolve
        import torch
        y0, y1 = 5, h - 3
        rows = torch.zeros((y1 - y0, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                      # (the viewer writes on its own stream)
        _lib.check(v._L.gsx_resolve_rgba8_device(v._h, (C.c_float * 3)(*BG), y0, y1, rows.data_ptr()))
        v.poll()
        assert np.array_equal(rows.cpu().numpy().view(np.uint8).reshape(y1 - y0, w, 4), got[y0:y1])
        # the stroke ends: the texture query is handed out and the cursor takes over — a ring at the last position
        t.end()
        assert t.query().kind == query.QueryKind.Texture
        cover, amb = _ring(size, (w - 4.4, h - 6.6), 6.3)
        _check_drawn(v.download_rgba8(BG), base, col, cover, amb, CURSOR_RGBA, "cursor ring half outside")
        assert not cover[:, : w // 2].any()
        t.update_pos((40.2, 25.6))                    # no tool: only the cursor moves
        t.update_brush_radius(11.4)
        cover, amb = _ring(size, (40.2, 25.6), 11.4)
        _check_drawn(v.download_rgba8(BG), base, col, cover, amb, CURSOR_RGBA, "cursor ring inside")
        # an immediate-mode Rect stroke: the rectangle's outline
        t.set_use_texture(False)
        t.start(Tool.Rect, Op.Set, (60.3, 40.2))
        t.update_pos((15.7, 8.4))
        cover, amb = _outline(size, (60.3, 40.2), (15.7, 8.4))
        _check_drawn(v.download_rgba8(BG), base, col, cover, amb, CURSOR_RGBA, "rect outline")
        assert not cover[20:30, 30:50].any() and cover[8, 30] and cover[25, 15]
        # alpha 0 again: the plain resolve, byte for byte
        v.set_toolset_overlay(STROKE_RGBA[:3] + (0.0,), CURSOR_RGBA[:3] + (0.0,), THICKNESS)
        assert np.array_equal(v.download_rgba8(BG), base)


def test_overlay_in_the_resolve_of_frames_on_both_lanes():
    """Two frames in flight: every other frame is rendered by the lane, on the lane's stream, while the paints (and the clear start()
    asks for) run on the viewer's.  download_rgba8 right behind paint + frame draws the stroke as painted up to then, whichever of the
    two rendered the frame; so with the cursor."""
    size = tc.SIZES[0]
    w, h = size
    none = np.zeros((h, w), bool)
    steps = [("start", (12.2, 14.1)), ("pos", (40.4, 30.7)), ("pos", (70.3, 12.2)), ("start", (30.6, 40.3)), ("pos", (66.1, 44.4)),
             ("end", (66.1, 44.4)), ("move", (25.3, 20.8))]
    with _small_viewer(frames_in_flight=2) as v:
        t = query.DeviceQueryToolset(v)
        t.update_brush_radius(6.3)
        for i, (what, p) in enumerate(steps):
            v.update_camera(camera.orbit_pose(10 + i), size)   # (first: the texture follows the viewport)
            v.set_toolset_overlay(STROKE_RGBA, CURSOR_RGBA, THICKNESS)
            if what == "start":
                t.start(Tool.Brush, Op.Set, p)
                if i:   # not rendered yet: the texture still holds the stroke before, and nothing of it is shown as the new one
                    assert np.array_equal(v.download_rgba8(BG), base), f"frame {i}: the stroke before shows after start()"
            elif what == "end":
                t.end()
                assert t.query().kind == query.QueryKind.Texture
            else:
                t.update_pos(p)
            t.render()
            v.render_frame(["m"])
            got = v.download_rgba8(BG)                 # first: nothing but paint, frame and resolve has been enqueued
            fb = v.download_framebuffer()
            lane = i % 2                               # the frames are dealt in turn: the viewer itself, its lane, ...
            assert np.array_equal(v.debug_download_lane_framebuffer(lane), fb), f"frame {i} was not rendered by lane {lane}"
            v.set_toolset_overlay(STROKE_RGBA[:3] + (0.0,), CURSOR_RGBA[:3] + (0.0,), THICKNESS)
            base = v.download_rgba8(BG)
            col = _resolved(fb)
            assert np.abs(base.astype(np.float64) - _round8(col)).max() <= 1
            where = f"frame {i} (lane {lane}), {what}"
            if what in ("start", "pos"):
                tex = v.download_query_texture()
                ops, host = _ops_until(steps, i), query.QueryToolset(size)
                tc.play(host, ops)
                amb = tc.ambiguous(ops, size)
                assert amb.sum() <= tc.AMBIGUOUS_CAP * (host.texture != 0).sum(), where
                assert np.array_equal(tex[~amb], host.texture[~amb]), where + ": the texture"
                _check_drawn(got, base, col, tex != 0, none, STROKE_RGBA, where + ": stroke overlay")
            else:
                cover, amb = _ring(size, p, 6.3)
                _check_drawn(got, base, col, cover, amb, CURSOR_RGBA, where + ": cursor ring")


def _ops_until(steps, i):
    """the stroke under way at step i of test_overlay_in_the_resolve_of_frames_on_both_lanes, as tests.toolset_cases ops"""
    first = max(k for k in range(i + 1) if steps[k][0] == "start")
    return [("radius", 6.3), ("start", Tool.Brush, Op.Set, steps[first][1])] + [("pos", p) for _, p in steps[first + 1:i + 1]]


# ---------------------------------------------------------------- 5. errors
def test_errors():
    a, b = tc.SIZES
    with _small_viewer() as v:
        L, h = v._L, v._h
        pos = (C.c_float * 2)(3.0, 4.0)
        nan = (C.c_float * 2)(float("nan"), 4.0)
        assert L.gsx_toolset_start(h, 2, 0, pos) == _lib.GSX_ERR_INVALID_ARG and b"unknown tool" in L.gsx_last_error_string()
        assert L.gsx_toolset_start(h, 1, 3, pos) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_toolset_start(h, 1, 0, nan) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_toolset_start(h, 1, 0, None) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_toolset_update_pos(h, nan) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_toolset_query(h, None) == _lib.GSX_ERR_INVALID_ARG
        for r in (0.0, -1.0, float("inf"), float("nan")):
            assert L.gsx_toolset_update_brush_radius(h, r) == _lib.GSX_ERR_INVALID_ARG, r
        t = query.DeviceQueryToolset(v)
        assert t.state() is None and t.query().kind == query.QueryKind.None_      # none of the refused calls started anything
        v.update_camera(R.scene_camera(), a)
        with pytest.raises(GsxError, match="query texture"):
            v.download_query_texture()                                            # nothing rendered yet: there is no texture
        tc.play(t, tc.CASES["drag"])
        t.render()
        buf = np.zeros((b[1], b[0]), np.uint8)
        assert L.gsx_download_query_texture(h, buf.ctypes.data, b[0], b[1]) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_download_query_texture(h, None, a[0], a[1]) == _lib.GSX_ERR_INVALID_ARG
        # painted for 83x51, the viewport is 96x64 now and the toolset has not rendered since: the texture query is refused
        t.end()
        q = t.query()
        assert q.kind == query.QueryKind.Texture
        v.update_camera(R.scene_camera(), b)
        v.update_query(q)
        with pytest.raises(GsxError, match="texture query without a viewport-sized query texture"):
            v.render_frame(["m"])
        t.render()                                                                # ... and accepted once it has
        v.render_frame(["m"])
        v.poll()


# ---------------------------------------------------------------- 6. the C++ facade
def test_cpp_facade_drags_through_the_toolset():
    """tools/frame_driver.cpp ends with the app's default drag through gs::QueryToolset (include/gsx.hpp): the texture it leaves is
    query.QueryToolset's for the same stroke, the one texture query selected something, and the toolset is idle afterwards"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "frame_driver")
    assert os.path.exists(exe), "tools/frame_driver missing: run __graft_entry__.build()"
    out = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    m = re.search(r"drag texels=(\d+) selected=(\d+) active=(\d)", out.stdout)
    assert m, out.stdout
    ops = [("radius", 14.5), ("start", Tool.Brush, Op.Set, (70.25, 50.5)), ("pos", (120.0, 90.25)), ("pos", (200.5, 110.0)), ("pos", (260.0, 150.75))]
    t = query.QueryToolset((320, 200))
    tc.play(t, ops)
    want, amb = int((t.texture != 0).sum()), int(tc.ambiguous(ops, (320, 200)).sum())
    assert amb <= tc.AMBIGUOUS_CAP * want and abs(int(m.group(1)) - want) <= amb, (out.stdout, want, amb)
    assert int(m.group(2)) > 20 and m.group(3) == "0", out.stdout
