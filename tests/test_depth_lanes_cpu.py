"""CPU: what the depth-tested frames on lanes promise outside the kernels — the A/B switch is read and documented, the C header states
the read-ordering contract in place of the old restriction, and the bindings repeat it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_depth_lanes_switch_has_its_row_in_design():
    text = _read("DESIGN.md")
    start = text.index("### Environment switches")
    table = text[start:text.index("\n## ", start)]
    rows = [r for r in table.splitlines() if r.startswith("| `GSX_DEPTH_LANES` |")]
    assert len(rows) == 1
    cells = [c.strip() for c in rows[0].strip("|").split("|")]
    assert len(cells) == 3 and all(cells), "variable | selects | why it stays / who uses it"
    assert "0:" in cells[1] and "viewer itself" in cells[1]
    assert "tests/test_gpu_depth_inflight.py" in cells[2], "the row names the test that renders both sides"
    assert os.path.exists(os.path.join(ROOT, "tests", "test_gpu_depth_inflight.py"))


def test_depth_lanes_switch_is_parsed_once_at_viewer_creation():
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api.cpp")
    create = api[api.index("gsx_status gsx_viewer_create("):api.index("void gsx_viewer_destroy(")]
    assert re.search(r'getenv\("GSX_DEPTH_LANES"\)\)\s*v->depth_lanes = atoi\(e\) != 0;', create), "read in gsx_viewer_create, 0 = off"
    everywhere = "".join(_read("wgpu_3dgs_viewer_app_amd", "csrc", n) for n in sorted(os.listdir(CSRC)) if n.endswith((".cpp", ".h", ".hip")))
    assert everywhere.count('getenv("GSX_DEPTH_LANES")') == 1, "read once: a viewer keeps the side it was created on"
    assert re.search(r"bool depth_lanes = true;", _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_state.h")), "default: on"
    # ... and it is what keeps a depth-tested frame off the lanes: the compare alone no longer does
    overlap = api[api.index("static bool frame_may_overlap("):api.index("namespace gsx {", api.index("static bool frame_may_overlap("))]
    assert re.search(r"depth_compare != GSX_DEPTH_ALWAYS && !v->depth_lanes", overlap)
    assert not re.search(r"\|\| v->depth_compare != GSX_DEPTH_ALWAYS\)", overlap)
    for clause in ("v->query.kind != GSX_QUERY_NONE", "v->ext_fb", "v->band_lo != 0", "shard_win_set"):
        assert clause in overlap, f"frames with {clause} still stay on the viewer"


def test_header_states_the_read_ordering_contract():
    h = _read("include", "gsx.h")
    block = h[h.index("/* ---- depth test against the caller's depth buffer"):h.index("typedef enum gsx_depth_compare")]
    assert "a depth-tested frame runs on the viewer itself, one at a time" not in h
    flat = " ".join(block.replace("*", " ").split())
    for phrase in ("dealt to a lane", "its own snapshot", "AS IF on the viewer's stream at the gsx_render_frame that uses them",
                   "waits for the snapshot", "no host wait", "GSX_DEPTH_LANES=0"):
        assert phrase in flat, phrase
    # sharded frames keep refusing the test: that bullet stays
    assert "frames (and gsx_render_more) return GSX_ERR_INVALID_ARG while the test is on" in flat


def test_bindings_and_guides_repeat_the_contract():
    for parts in (("include", "gsx.hpp"), ("rust", "gsx", "src", "lib.rs"), ("wgpu_3dgs_viewer_app_amd", "viewer.py"), ("INTEGRATION.md",)):
        flat = " ".join(_read(*parts).replace("///", " ").replace("//", " ").split())
        assert "as if on the viewer's stream at the" in flat, parts
        assert "runs on the viewer itself, one at a time (like a frame with a query)" not in flat, parts


def test_one_launch_caps_the_windows_and_builds_their_pyramids():
    spec = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_spec.hip")
    assert re.search(r"__launch_bounds__\(1024\) void k_depth_cap_pyramid\(", spec)
    assert re.search(r"GSX_LAUNCH\(k_depth_cap_pyramid, dim3\(1\), dim3\(1024\)", spec), "one 1024-lane workgroup, through GSX_LAUNCH"
    everywhere = "".join(_read("wgpu_3dgs_viewer_app_amd", "csrc", n) for n in sorted(os.listdir(CSRC)) if n.endswith((".cpp", ".h", ".hip")))
    assert "k_depth_cap_windows" not in everywhere and "launch_depth_cap_windows" not in everywhere
