"""Mask gizmos (gsx_viewer_set_mask_gizmos, spec §10) without a device: the record's layout, the entry point in the header, the library
and the bindings; the wireframe of csrc/gizmo_math.h — played by tests/gizmo_driver.cpp, a stand-alone program built with the address
and undefined-behaviour sanitizers — against the float64 restatement tests/gizmo_ref.py and against the mask's own predicate; and the
condition on the scenes of tests/test_gpu_gizmos.py: the pixels at which float32 and float64 may differ are few."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import spec_f64
from tests import gizmo_ref as G
from wgpu_3dgs_viewer_app_amd import _lib, mask
from wgpu_3dgs_viewer_app_amd.viewer import MASK_GIZMO_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
FIELDS = {"kind": 0, "pos": 4, "quat_xyzw": 16, "scale": 32, "color": 44, "line_width": 60}


def test_mask_gizmo_is_64_bytes():
    assert C.sizeof(_lib.MaskGizmo) == 64 and MASK_GIZMO_DTYPE.itemsize == 64
    assert {f: getattr(_lib.MaskGizmo, f).offset for f in FIELDS} == FIELDS
    assert {f: MASK_GIZMO_DTYPE.fields[f][1] for f in FIELDS} == FIELDS
    rec = G.gizmo(1, (1, 2, 3), (0.1, 0.2, 0.3, 0.9), (4, 5, 6), (0.25, 0.5, 0.75, 1.0), 2.5)
    raw = _lib.MaskGizmo.from_buffer_copy(rec.tobytes())
    assert raw.kind == 1 and list(raw.pos) == [1, 2, 3] and list(raw.scale) == [4, 5, 6] and list(raw.color) == [0.25, 0.5, 0.75, 1.0]
    assert np.allclose(list(raw.quat_xyzw), [0.1, 0.2, 0.3, 0.9]) and raw.line_width == 2.5
    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    assert re.search(r"typedef struct gsx_mask_gizmo \{ uint32_t kind; float pos\[3\]; float quat_xyzw\[4\]; float scale\[3\]; float color\[4\]; "
                     r"float line_width; \} gsx_mask_gizmo;", hdr)
    assert re.search(r"#define GSX_GIZMO_MAX_SHAPES 256u", hdr) and _lib.GSX_GIZMO_MAX_SHAPES == 256
    assert re.search(r"#define GSX_GIZMO_CIRCLE_SEGMENTS 64u", hdr) and _lib.GSX_GIZMO_CIRCLE_SEGMENTS == G.CIRCLE_SEGMENTS == 64
    assert "static_assert(sizeof(gsx_mask_gizmo) == 64" in open(os.path.join(CSRC, "gsx_api_overlay.cpp")).read()


def test_entry_point_is_declared_exported_and_bound():
    fn = "gsx_viewer_set_mask_gizmos"
    L = _lib.load()
    assert re.search(r"^gsx_status " + fn + r"\(", open(os.path.join(ROOT, "include", "gsx.h")).read(), re.M)
    assert hasattr(L, fn) and fn in _lib.EXPORTS
    rust_sys = open(os.path.join(ROOT, "rust", "gsx-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn " + fn + r"\(", rust_sys) and "pub struct gsx_mask_gizmo" in rust_sys
    assert "fn set_mask_gizmos" in open(os.path.join(ROOT, "rust", "gsx", "src", "lib.rs")).read()
    assert "set_mask_gizmos" in open(os.path.join(ROOT, "include", "gsx.hpp")).read()
    assert L.gsx_viewer_set_mask_gizmos(None, None, 0) == _lib.GSX_ERR_INVALID_ARG  # without a device: a status code, not a crash


def test_gizmo_records_are_boxes_then_ellipsoids_per_model():
    B, E = mask.MaskShapeKind.Box, mask.MaskShapeKind.Ellipsoid
    first = [mask.MaskShape(E, pos=np.float32([1, 0, 0])), mask.MaskShape(B, pos=np.float32([2, 0, 0])), mask.MaskShape(B, pos=np.float32([3, 0, 0]))]
    second = [mask.MaskShape(E, pos=np.float32([4, 0, 0]), color=np.float32([1, 0, 0, 0.5])), mask.MaskShape(B, pos=np.float32([5, 0, 0]))]
    recs = mask.gizmo_records([first, second], 7.0)
    assert recs.dtype == MASK_GIZMO_DTYPE and recs["pos"][:, 0].tolist() == [2, 3, 1, 5, 4] and recs["kind"].tolist() == [0, 0, 1, 0, 1]
    assert np.all(recs["line_width"] == 7.0) and recs["color"][4].tolist() == [1, 0, 0, 0.5] and recs["color"][0].tolist() == [1, 1, 1, 1]
    assert mask.gizmo_records([]).shape == (0,) and mask.MaskShape().color.tolist() == [1, 1, 1, 1]


TRS = [G.gizmo(kind, (0.4, -0.7, 1.5), G._quat((1.0, 2.0, 0.5), 40.0), (2.0, 0.5, 1.2)) for kind in (G.BOX, G.ELLIPSOID)]


@pytest.mark.parametrize("g", TRS, ids=["box", "ellipsoid"])
def test_every_vertex_lies_on_the_boundary_the_mask_tests(g):
    """§2c's predicate (oracle/spec_f64.py) is true just inside every wireframe vertex and false just outside it."""
    g = g[0]
    shape = dict(kind=int(g["kind"]), pos=g["pos"], quat=g["quat_xyzw"], scale=g["scale"])
    ends = np.array([q for seg in G.shape_segments(g["kind"]) for q in seg])
    assert len(ends) == (24 if g["kind"] == G.BOX else 384)
    rot, pos, scale = G.quat_to_mat(g["quat_xyzw"]), np.asarray(g["pos"], np.float64), np.asarray(g["scale"], np.float64)
    for factor, want in ((0.999, True), (1.001, False)):
        world = pos + (scale * ends * factor) @ rot.T
        inside, _ = spec_f64.mask_evaluate(world, ("shape", 0), [shape])
        assert np.all(inside == want), factor
    # ... and the restatement's world ends are those points
    assert np.allclose(np.array([p for seg in G.world_segments(g) for p in seg]), pos + (scale * ends) @ rot.T, rtol=0, atol=1e-12)


def test_box_edges_come_in_the_spec_order():
    corner = lambda q: int(q[0] > 0) + 2 * int(q[1] > 0) + 4 * int(q[2] > 0)  # noqa: E731
    assert [(corner(a), corner(b)) for a, b in G.shape_segments(G.BOX)] == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7),
                                                                           (0, 4), (1, 5), (2, 6), (3, 7)]
    segs = G.shape_segments(G.ELLIPSOID)
    assert len(segs) == 192 and all(a[2] == 0 for a, _ in segs[:64]) and all(a[0] == 0 for a, _ in segs[64:128]) and all(a[1] == 0 for a, _ in segs[128:])
    assert all(np.array_equal(segs[k][1], segs[k + 1][0]) for k in range(191) if k % 64 != 63)  # chord j ends where chord j + 1 starts
    assert segs[0][0].tolist() == [1, 0, 0] and segs[64][0].tolist() == [0, 1, 0] and segs[128][0].tolist() == [0, 0, 1]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gizmo") / "gizmo_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "gizmo_driver.cpp"), "-o", exe])
    return exe


def _play(driver, gizmos, view, proj):
    lines = ["view " + " ".join(repr(float(x)) for x in np.asarray(view, np.float32).reshape(16)),
             "proj " + " ".join(repr(float(x)) for x in np.asarray(proj, np.float32).reshape(16))]
    for g in gizmos:
        lines.append(f"gizmo {int(g['kind'])} " + " ".join(repr(float(x)) for x in (*g["pos"], *g["quat_xyzw"], *g["scale"])))
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.mark.parametrize("name", ["box_trs", "ellipsoid_trs", "camera_inside_box", "box_ellipsoid_line_order", "past_batch_64_tail"])
def test_driver_agrees_with_the_restatement(driver, name):
    w, h = G.VIEWPORTS[0]
    gizmos = G.scenes(w, h)[name][0]
    _, view, proj = G.matrices(name, w, h)
    got = _play(driver, gizmos, view, proj)
    want = [(s, k, p0, p1) + G.clip_segment(p0, p1, view, proj) for s, g in enumerate(gizmos) for k, (p0, p1) in enumerate(G.world_segments(g))]
    assert len(got) == len(want) == sum(12 if g["kind"] == G.BOX else 192 for g in gizmos)
    statuses = set()
    for row, (s, k, p0, p1, status, _, _, c0, c1) in zip(got, want):
        assert row[0] == "seg" and (int(row[1]), int(row[2])) == (s, k)
        assert int(row[3]) == status, (s, k)  # which segments are clipped, at which end, or dropped: exactly
        f = np.array(row[4:], np.float64)
        scale = max(np.abs(p0).max(), np.abs(p1).max())
        assert np.abs(f[0:3] - p0).max() <= 1e-6 * scale and np.abs(f[3:6] - p1).max() <= 1e-6 * scale, (s, k)
        if status != G.DROPPED:  # the clipped clip-space ends: float32 through two 4 x 4 products and the lerp
            cs = max(np.abs(c0).max(), np.abs(c1).max())
            assert np.abs(f[6:10] - c0).max() <= 1e-5 * cs and np.abs(f[10:14] - c1).max() <= 1e-5 * cs, (s, k)
        statuses.add(status)
    if name == "camera_inside_box":
        assert statuses >= {G.WHOLE, G.CLIPPED_0, G.CLIPPED_1}


def _draw(size, name):
    return G.reference(size, name)[4]


@pytest.mark.parametrize("name", list(G.scenes(*G.VIEWPORTS[0])))
@pytest.mark.parametrize("size", G.VIEWPORTS)
def test_scenes_have_few_ambiguous_pixels(size, name):
    """A condition on the inputs, not a tolerance: a scene that breaks the cap is replaced."""
    r = _draw(size, name)
    covered, ambiguous = int(r["cover"].sum()), int((r["ambiguous"] & r["cover"]).sum())
    assert ambiguous <= G.AMBIGUOUS_CAP * covered, (name, covered, ambiguous)
    assert (covered > 100) == (name != "cleared"), (name, covered)
    assert G.EDGE_TOL <= G.EDGE_TOL_MAX == 0.01


@pytest.mark.parametrize("size", G.VIEWPORTS)
def test_camera_inside_box_keeps_its_edges(size):
    """Edges that cross the eye plane are clipped, not lost: under §9's rule alone (an end at w <= 0: not drawn) they would vanish."""
    segs = _draw(size, "camera_inside_box")["segments"]
    assert len(segs) == 12
    assert sum(1 for _, _, status, px in segs if px > 0) >= 8
    assert {status for _, _, status, px in segs if px > 0} == {G.WHOLE, G.CLIPPED_0, G.CLIPPED_1}  # clipped at either end, and seen
    assert sum(1 for _, _, status, px in segs if px > 0 and status == G.WHOLE) < 8  # ... without them the count above would not hold


@pytest.mark.parametrize("size", G.VIEWPORTS)
def test_shape_order_shows(size):
    a, b = _draw(size, "box_ellipsoid_line_order"), _draw(size, "ellipsoid_box_line_order")
    assert np.abs(a["rgba"] - b["rgba"]).max() > 0.05
    for name, seen in (("past_batch_64_tail", 21), ("past_batch_64_head", 0)):  # the 21 shapes aside reach no pixel; the box does
        segs = _draw(size, name)["segments"]
        assert len(segs) == 21 * 192 + 12
        assert sum(1 for s in segs if s[0] == seen and s[3] > 0) >= 6 and all(s[3] == 0 for s in segs if s[0] != seen)
