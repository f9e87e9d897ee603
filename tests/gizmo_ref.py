"""float64 numpy restatement of spec/RENDER_SPEC.md section 10 (mask gizmos), and the scenes the gizmo tests draw.  A helper, not a
test.  Written from the spec section: segment k of a shape in the shape frame, the shape-to-world map of section 2c, the clip against
the near plane, and from there section 9 — whose projection, triangles and edge distances are ``overlay_ref``'s, unchanged: a
clipped segment is handed to them as a line between its clipped world-space ends (the clip is linear, so the point at parameter t of
the clip-space segment is the image of the point at t of the world-space one).

``draw`` takes gizmos AND lines: they share one (C, A, E), gizmo segments first.  It returns what ``overlay_ref.draw`` returns, the
AMBIGUOUS mask included, and ``segments``: one ``(shape, k, status, pixels)`` per gizmo segment, status as ``clip_segment`` gives it.

EDGE_TOL.  ``overlay_ref`` marks a pixel centre within 0.01 px of an edge; a 64-chord circle has five edges to every 2 to 3 px of arc, and
at 0.01 px those alone would mark more than AMBIGUOUS_CAP.  What float32 can move is far less.  With corner coordinates of at most 128 px:
  * a corner is the end of some 16 float32 operations (shape to world, view, projection, the offset, the divide, the viewport map), each
    rounding by at most 2^-24 of a value no larger than the result's range: 16 * 2^-24 * 128 px = 1.2e-4 px;
  * the edge function ex (py - ay) - ey (px - ax) has products of at most L * 100 px^2 for an edge of length L, four roundings:
    4 * 2^-24 * L * 100 / L = 2.4e-5 px of distance, whatever L is — the shortest edge included.
Together 1.5e-4 px; EDGE_TOL is a little over three times that.  Both terms grow with the coordinates, so a segment one of whose corners
lies further out than 128 px — the near clip leaves ends thousands of pixels off screen, with w = z_near — gets EDGE_TOL scaled by
max |coordinate| / 128, and never more than overlay_ref's 0.01.
"""
from __future__ import annotations

import math

import numpy as np

from tests import overlay_ref as R
from tests.overlay_ref import AMBIGUOUS_CAP, DEPTH_TOL, VIEWPORTS, _corners, _segment_distance, _triangle  # noqa: F401
from wgpu_3dgs_viewer_app_amd import camera
from wgpu_3dgs_viewer_app_amd.mask import MaskShape, MaskShapeKind
from wgpu_3dgs_viewer_app_amd.viewer import HIT_PAIR_DTYPE, MASK_GIZMO_DTYPE, HitPair

EDGE_TOL = 5e-4       # px, for corners within EDGE_TOL_RANGE of the origin
EDGE_TOL_RANGE = 128.0
EDGE_TOL_MAX = 0.01   # overlay_ref.EDGE_TOL
CIRCLE_SEGMENTS = 64
#: (cos, sin) of 2 pi j / 64: float64, rounded to float32 — the bits the library starts from
CIRCLE = np.array([(math.cos(2.0 * math.pi * j / CIRCLE_SEGMENTS), math.sin(2.0 * math.pi * j / CIRCLE_SEGMENTS))
                   for j in range(CIRCLE_SEGMENTS)], np.float32).astype(np.float64)
DROPPED, WHOLE, CLIPPED_0, CLIPPED_1 = 0, 1, 2, 3


def quat_to_mat(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def shape_segments(kind):
    """The wireframe in the shape frame: a list of (a, b), in the spec's order."""
    if int(kind) == 0:
        corner = [np.array([1.0 if i & 1 else -1.0, 1.0 if i & 2 else -1.0, 1.0 if i & 4 else -1.0]) for i in range(8)]
        out = []
        for axis in range(3):  # four edges along x, then y, then z; by ascending lower corner
            step = 1 << axis
            out += [(corner[i], corner[i + step]) for i in range(8) if not i & step]
        return out
    out = []
    for put in (lambda c, s: np.array([c, s, 0.0]), lambda c, s: np.array([0.0, c, s]), lambda c, s: np.array([s, 0.0, c])):
        for j in range(CIRCLE_SEGMENTS):  # the planes q_z = 0, q_x = 0, q_y = 0
            out.append((put(*CIRCLE[j]), put(*CIRCLE[(j + 1) % CIRCLE_SEGMENTS])))
    return out


def world_segments(g):
    """p_w = pos + R (scale * q) for both ends of every segment of one record."""
    pos, scale = np.asarray(g["pos"], np.float64), np.asarray(g["scale"], np.float64)
    rot = quat_to_mat(g["quat_xyzw"])
    return [(pos + rot @ (scale * a), pos + rot @ (scale * b)) for a, b in shape_segments(g["kind"])]


def clip_segment(p0, p1, view, proj):
    """-> (status, clipped world end 0, clipped world end 1, clip-space end 0, clip-space end 1): the clip against c.z >= 0."""
    M = np.asarray(proj, np.float64).reshape(4, 4).T @ np.asarray(view, np.float64).reshape(4, 4).T
    c0, c1 = M @ np.append(p0, 1.0), M @ np.append(p1, 1.0)
    in0, in1 = c0[2] >= 0.0, c1[2] >= 0.0
    if in0 and in1:
        return WHOLE, p0, p1, c0, c1
    if not in0 and not in1:
        return DROPPED, p0, p1, c0, c1
    t = c0[2] / (c0[2] - c1[2])
    p, c = p0 + t * (p1 - p0), c0 + t * (c1 - c0)
    return (CLIPPED_0, p, p1, c, c1) if not in0 else (CLIPPED_1, p0, p, c0, c)


def draw(gizmos, lines, view, proj, w, h, depth=None):
    """-> dict(cover bool [h, w], rgba float64 [h, w, 4] premultiplied, depth float64 [h, w] = E, ambiguous bool [h, w], segments)."""
    gizmos = np.asarray(gizmos, MASK_GIZMO_DTYPE).reshape(-1) if gizmos is not None and len(gizmos) else np.zeros(0, MASK_GIZMO_DTYPE)
    lines = np.asarray(lines, HIT_PAIR_DTYPE).reshape(-1) if lines is not None and len(lines) else np.zeros(0, HIT_PAIR_DTYPE)
    todo = []  # (line for _corners, straight colour, edge tolerance base, (shape, k, status) or None)
    for s, g in enumerate(gizmos):
        for k, (p0, p1) in enumerate(world_segments(g)):
            status, q0, q1, _, _ = clip_segment(p0, p1, view, proj)
            line = None if status == DROPPED else {"p0": q0, "p1": q1, "line_width": g["line_width"]}
            todo.append((line, np.asarray(g["color"], np.float64), EDGE_TOL, (s, k, status)))
    for line in lines:
        todo.append((line, np.asarray(line["color"], np.float64) / 255.0, R.EDGE_TOL, None))
    D = np.ones((h, w), np.float64) if depth is None else np.asarray(depth, np.float64).copy()
    E = D.copy()
    C = np.zeros((h, w, 3), np.float64)
    A = np.zeros((h, w), np.float64)
    amb = np.zeros((h, w), bool)
    cover = np.zeros((h, w), bool)
    segments = []
    py, px = np.mgrid[0:h, 0:w].astype(np.float64)
    px += 0.5
    py += 0.5
    for line, col, tol, tag in todo:
        got = _corners(line, view, proj, w, h) if line is not None else None
        if got is None:
            if tag:
                segments.append(tag + (0,))
            continue
        (a, b, c, d), z0, z1 = got  # a, b: end 1 -, +; c, d: end 0 -, +
        if got[0][:, 0].max() < -1.0 or got[0][:, 0].min() > w + 1.0 or got[0][:, 1].max() < -1.0 or got[0][:, 1].min() > h + 1.0:
            if tag:  # (wholly off screen: no pixel is covered, none is near an edge)
                segments.append(tag + (0,))
            continue
        tol = min(tol * max(1.0, float(np.abs(got[0]).max()) / EDGE_TOL_RANGE), EDGE_TOL_MAX)
        for u, v in ((a, b), (b, d), (d, c), (c, a), (b, c)):
            amb |= _segment_distance(u, v, px, py) < tol
        in1, (wa, wb, wc) = _triangle(a, b, c, px, py)
        in2, (vb, vc, vd) = _triangle(b, c, d, px, py)
        z = np.where(in1, (wa + wb) * z1 + wc * z0, vb * z1 + (vc + vd) * z0)
        frag = in1 | in2
        amb |= frag & ((np.abs(z) < DEPTH_TOL) | (np.abs(z - 1.0) < DEPTH_TOL))
        frag &= (z >= 0.0) & (z <= 1.0)
        amb |= frag & (np.abs(z - E) < DEPTH_TOL)
        ok = frag & (z < E)
        E = np.where(ok, z, E)
        C = np.where(ok[..., None], col[3] * col[:3] + (1.0 - col[3]) * C, C)
        A = np.where(ok, col[3] + (1.0 - col[3]) * A, A)
        cover |= ok
        if tag:
            segments.append(tag + (int(ok.sum()),))
    return {"cover": cover, "rgba": np.concatenate([C, A[..., None]], axis=2), "depth": E, "ambiguous": amb, "segments": segments}


# ---- the scenes --------------------------------------------------------------------------------------------------------

def _quat(axis, degrees):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    half = math.radians(degrees) / 2.0
    return np.append(axis * math.sin(half), math.cos(half)).astype(np.float32)


def gizmo(kind, pos=(0, 0, 0), rotation=(0, 0, 0, 1), scale=(1, 1, 1), color=(1, 1, 1, 1), line_width=30.0):
    return MaskShape(MaskShapeKind(kind), np.asarray(pos, np.float32), np.asarray(rotation, np.float32), np.asarray(scale, np.float32),
                     np.asarray(color, np.float32)).to_mask_gizmo_pod(line_width)


def cat(*recs):
    return np.concatenate([np.asarray(r, MASK_GIZMO_DTYPE).reshape(-1) for r in recs]) if recs else np.zeros(0, MASK_GIZMO_DTYPE)


def inside_camera():
    """the eye at (-1.7, 0.6, 2.1), inside the box of ``camera_inside_box`` (half-extent 3 about the origin), looking at the far corner
    region with a vertical field of view of 90 degrees: nine edges reach the screen, two of them through the near plane (one clipped at
    either end) — under section 9's rule alone seven would be left"""
    return camera.CameraOrbitControl(target=np.array([2.8, -1.3, -2.2], np.float32), pos=np.array([-1.7, 0.6, 2.1], np.float32), z=(0.1, 20.0),
                                     vertical_fov=math.radians(90.0))


def scene_cameras():
    """scene name -> camera, where it is not overlay_ref.scene_camera()"""
    return {"camera_inside_box": inside_camera()}


def matrices(name, w, h):
    cam = scene_cameras().get(name) or R.scene_camera()
    return cam, cam.view(), cam.projection(w / h)


BOX, ELLIPSOID = 0, 1
ORANGE, CYAN, VIOLET = (1.0, 0.55, 0.1, 0.5), (0.1, 0.9, 0.85, 0.6), (0.7, 0.3, 1.0, 0.75)


def scenes(w, h):
    """name -> (gizmos, lines, caller depth buffer or None).  Each is there to break one thing (tests/test_gpu_gizmos.py)."""
    _, proj = R.matrices(w, h)
    skew = _quat((1.0, 2.0, 0.5), 40.0)
    # The ellipsoids stand two units from the eye, not five: consecutive chords overlap by their half-width, and where two overlapping
    # fragments' depths differ by less than DEPTH_TOL the pixel is ambiguous.  NDC depth changes with 1 / d^2, so up close the chords'
    # depth gradients differ enough for such ties to be few.
    box = gizmo(BOX, (-0.3, 0.7, -3.0), _quat((0.3, 1.0, 0.2), 25.0), (0.55, 0.45, 0.5), ORANGE, 14.0)
    ell = gizmo(ELLIPSOID, (0.4, 0.8, -3.0), _quat((1.0, 0.2, 0.4), 35.0), (0.8, 0.5, 0.6), CYAN, 12.0)
    line = HitPair((-1.2, 0.5, -2.95), (1.3, 1.0, -3.05), (255, 60, 200, 180), 14.0)
    # 21 ellipsoids (4032 records: 63 batches) far off to the side: every segment is projected, none of their pixel boxes reaches the
    # viewport, so the visible box's records lie in batch 63 (tail) or 0 (head) and the line's in batch 64, the outer ballot's second group
    aside = [gizmo(ELLIPSOID, (60.0 + 3.0 * i, 0.5, 2.0), _quat((0.0, 1.0, 0.0), 10.0 * i), (1.0, 1.2, 0.8), VIOLET, 30.0) for i in range(21)]
    seen = gizmo(BOX, (0.2, 0.6, 0.3), skew, (1.4, 0.9, 1.1), ORANGE, 38.0)
    tail_line = HitPair((-2.0, -0.4, 0.4), (2.1, 1.7, 0.2), (40, 255, 90, 200), 36.0)
    plane = np.full((h, w), R.ndc_depth(proj, 5.0), np.float32)  # a caller plane at view depth 5: through the middle of the box
    none = np.zeros(0, HIT_PAIR_DTYPE)
    return {
        "box_identity_alpha": (cat(gizmo(BOX, color=(1.0, 0.8, 0.2, 0.5), line_width=40.0)), none, None),
        "box_trs": (cat(gizmo(BOX, (0.4, 0.7, 0.5), skew, (2.0, 0.5, 1.2), CYAN, 36.0)), none, None),
        "ellipsoid_trs": (cat(gizmo(ELLIPSOID, (0.1, 0.75, -3.0), skew, (1.1, 0.6, 0.8), VIOLET, 12.0)), none, None),
        "camera_inside_box": (cat(gizmo(BOX, scale=(3.0, 3.0, 3.0), color=ORANGE, line_width=30.0)), none, None),
        "box_ellipsoid_line_order": (cat(box, ell), line, None),
        "ellipsoid_box_line_order": (cat(ell, box), line, None),
        "past_batch_64_tail": (cat(*aside, seen), tail_line, None),
        "past_batch_64_head": (cat(seen, *aside), tail_line, None),
        "caller_plane": (cat(gizmo(BOX, (0.0, 0.8, 0.0), skew, (1.5, 1.0, 1.5), CYAN, 38.0)), none, plane),
        "cleared": (cat(), none, None),
    }


_reference = {}


def reference(size, name):
    """(gizmos, lines, depth, camera, draw(...)) of one scene, computed once and shared (read-only)"""
    if (size, name) not in _reference:
        w, h = size
        gizmos, lines, depth = scenes(w, h)[name]
        cam, view, proj = matrices(name, w, h)
        r = draw(gizmos, lines, view, proj, w, h, depth)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _reference[(size, name)] = (gizmos, lines, depth, cam, r)
    return _reference[(size, name)]
