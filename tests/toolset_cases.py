"""The query toolset's painting cases (spec §7 "Toolset"), shared by tests/test_toolset_cpu.py and tests/test_gpu_toolset.py: every case
is a list of toolset calls; ``reference`` plays it on ``query.QueryToolset`` (the float64 statement of the rule) and says which texels are
within 1e-3 px of a cut — those may go either way on a float32 implementation, every other texel must match."""
import functools
import math

import numpy as np

from wgpu_3dgs_viewer_app_amd import query
from wgpu_3dgs_viewer_app_amd.query import QuerySelectionOp as Op
from wgpu_3dgs_viewer_app_amd.query import QueryToolsetTool as Tool

SIZES = [(83, 51), (96, 64)]
AMBIGUOUS_PX = 1e-3
AMBIGUOUS_CAP = 0.01          # a condition on the inputs: at most 1 % of a case's painted texels may be ambiguous
QUEUE = 64                    # pending brush segments one launch takes (csrc/toolset_math.h, kToolsetMaxSegs)


def _brush(r, path, op=Op.Set):
    return [("radius", r), ("start", Tool.Brush, op, path[0])] + [("pos", p) for p in path[1:]]


def _rect(corners, op=Op.Set):
    return [("start", Tool.Rect, op, corners[0])] + [("pos", p) for p in corners[1:]]


DRAG = [(10.5, 12), (25, 20.25), (40, 17), (60.5, 30), (75, 44.75), (90, 49)]
CASES = {
    "drag": _brush(9.5, DRAG, Op.Add),                                       # leaves the viewport at the end
    "dot": _brush(0.4, [(20.3, 20.3)]),                                      # one texel
    "everything": _brush(200.0, [(40, 25), (41, 26)]),                       # every texel
    "off_screen": _brush(9.5, [(-30, -30), (-12, -14)]),                     # nothing
    "both_side_edges": _brush(3.25, [(-5.25, 25), (88.5, 25.75)]),
    # more segments than the queue holds: the call that fills it paints
    "long_zigzag": _brush(1.7, [(3.3 + 0.85 * k, 25.2 + 18.0 * math.sin(0.7 * k)) for k in range(QUEUE + 27)]),
    "radius_changes": [("radius", 6.3), ("start", Tool.Brush, Op.Set, (12.2, 10.1)), ("pos", (30.4, 22.7)), ("radius", 2.1), ("pos", (55.3, 20.2)),
                       ("radius", 11.4), ("pos", (70.1, 40.6))],
    "rect_reversed": _rect([(60.25, 40.3), (12.75, 8.25)]),
    "rect_thin": _rect([(10.6, 5.6), (40.2, 5.9)]),                          # thinner than a texel, covers no centre
    "rect_partly_off": _rect([(-10.25, 30.25), (50.75, 70.0)]),
    "rect_shrinking": _rect([(5.25, 5.25), (70.75, 45.75), (40.25, 30.75), (20.75, 12.25)]),   # the old texels must go
    "two_strokes": _brush(9.5, DRAG) + _brush(4.2, [(70.3, 8.1), (50.2, 12.4)]),               # the second start clears the first
    "brush_then_rect": _brush(5.1, [(20.2, 30.3), (60.4, 35.1)]) + _rect([(30.25, 10.25), (44.75, 20.75)]),
}
EXPECTED = {"drag": (1698, 6), "dot": (1, None), "everything": (83 * 51, None), "off_screen": (0, None), "both_side_edges": (555, 0),
            "rect_thin": (0, None)}   # (painted texels, ambiguous texels or None = not pinned) at 83x51


def play(toolset, ops, after_each=None):
    for o in ops:
        if o[0] == "radius":
            toolset.update_brush_radius(o[1])
        elif o[0] == "start":
            toolset.start(o[1], o[2], o[3])
        elif o[0] == "pos":
            toolset.update_pos(o[1])
        else:
            raise ValueError(o)
        if after_each is not None and o[0] != "radius":
            after_each()


def _seg_distance(px, py, a, b):
    ax, ay, bx, by = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    dx, dy = bx - ax, by - ay
    len2 = dx * dx + dy * dy
    t = np.clip(((px - ax) * dx + (py - ay) * dy) / len2, 0.0, 1.0) if len2 > 0 else 0.0
    return np.sqrt((px - (ax + t * dx)) ** 2 + (py - (ay + t * dy)) ** 2)


def ambiguous(ops, size):
    """bool [h, w]: texels within AMBIGUOUS_PX of a cut of the texture the ops leave (the strokes since the last start)."""
    w, h = size
    last = max(i for i, o in enumerate(ops) if o[0] == "start")
    radius = 40.0
    for o in ops[:last]:
        if o[0] == "radius":
            radius = float(o[1])
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx + 0.5, yy + 0.5
    start = ops[last]
    if start[1] == Tool.Rect:
        p = [o[1] for o in ops[last + 1:] if o[0] == "pos"]
        end = p[-1] if p else start[3]
        x0, x1 = sorted((float(start[3][0]), float(end[0])))
        y0, y1 = sorted((float(start[3][1]), float(end[1])))
        near_x = (np.abs(px - x0) <= AMBIGUOUS_PX) | (np.abs(px - x1) <= AMBIGUOUS_PX)
        near_y = (np.abs(py - y0) <= AMBIGUOUS_PX) | (np.abs(py - y1) <= AMBIGUOUS_PX)
        return (near_x & (py >= y0 - AMBIGUOUS_PX) & (py <= y1 + AMBIGUOUS_PX)) | (near_y & (px >= x0 - AMBIGUOUS_PX) & (px <= x1 + AMBIGUOUS_PX))
    near = np.zeros((h, w), bool)
    prev = pos = start[3]
    segs = [(prev, pos, radius)]
    for o in ops[last + 1:]:
        if o[0] == "radius":
            radius = float(o[1])
        elif o[0] == "pos":
            prev, pos = pos, o[1]
            segs.append((prev, pos, radius))
    for a, b, r in segs:
        d = _seg_distance(px, py, a, b)
        near |= np.abs(d - r) <= AMBIGUOUS_PX
    return near


@functools.lru_cache(maxsize=None)
def reference(name, size=SIZES[0]):
    """(texture uint8 [h, w] of query.QueryToolset, ambiguous bool [h, w]); read-only"""
    t = query.QueryToolset(size)
    play(t, CASES[name])
    tex, amb = t.texture.copy(), ambiguous(CASES[name], size)
    assert amb.sum() <= AMBIGUOUS_CAP * int((tex != 0).sum()), \
        f"case {name} at {size}: {amb.sum()} of {(tex != 0).sum()} painted texels are ambiguous: replace the case"
    tex.setflags(write=False)
    amb.setflags(write=False)
    return tex, amb


def assert_matches(got, name, size=SIZES[0], what=""):
    tex, amb = reference(name, size)
    assert got.shape == tex.shape and got.dtype == np.uint8
    assert set(np.unique(got)) <= {0, 255}, f"{what}{name}: texel values {np.unique(got)[:8]}"
    bad = np.argwhere((got != tex) & ~amb)
    assert bad.size == 0, f"{what}{name} at {size}: {bad.shape[0]} texels differ from query.QueryToolset away from every cut, first (y, x) {bad[:6].tolist()}"
