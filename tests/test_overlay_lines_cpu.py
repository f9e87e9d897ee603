"""Overlay lines (gsx_viewer_set_overlay_lines, spec §9) without a device: the record's layout, the three entry points in the
header, the library and the Rust binding, and the condition on the scenes of tests/test_gpu_overlay_lines.py — the pixels at which
float32 and float64 may differ are few."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import overlay_ref as R
from wgpu_3dgs_viewer_app_amd import _lib
from wgpu_3dgs_viewer_app_amd.viewer import HIT_PAIR_DTYPE, HitPair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("gsx_viewer_set_overlay_lines", "gsx_download_overlay", "gsx_overlay_device_ptrs")


def test_overlay_line_is_the_32_byte_hit_pair():
    assert C.sizeof(_lib.OverlayLine) == 32
    assert [getattr(_lib.OverlayLine, f).offset for f in ("p0", "color", "p1", "line_width")] == [0, 12, 16, 28]
    assert HIT_PAIR_DTYPE.itemsize == 32 and [HIT_PAIR_DTYPE.fields[f][1] for f in ("p0", "color", "p1", "line_width")] == [0, 12, 16, 28]
    rec = HitPair((1, 2, 3), (4, 5, 6), (7, 8, 9, 10), 2.5)
    raw = _lib.OverlayLine.from_buffer_copy(rec.tobytes())
    assert list(raw.p0) == [1, 2, 3] and list(raw.color) == [7, 8, 9, 10] and list(raw.p1) == [4, 5, 6] and raw.line_width == 2.5
    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    assert re.search(r"typedef struct gsx_overlay_line \{ float p0\[3\]; uint8_t color\[4\]; float p1\[3\]; float line_width; \} gsx_overlay_line;", hdr)
    assert re.search(r"#define GSX_OVERLAY_MAX_LINES 4096u", hdr) and _lib.GSX_OVERLAY_MAX_LINES == 4096
    assert re.search(r"#define GSX_ABI_VERSION 3u", hdr)


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    rust_sys = open(os.path.join(ROOT, "rust", "gsx-sys", "src", "lib.rs")).read()
    L = _lib.load()
    for fn in FUNCTIONS:
        assert re.search(r"^gsx_status " + fn + r"\(", hdr, re.M), fn
        assert hasattr(L, fn) and fn in _lib.EXPORTS, fn
        assert re.search(r"pub fn " + fn + r"\(", rust_sys), fn
    assert "pub struct gsx_overlay_line" in rust_sys
    assert "fn update_hit_pairs" in open(os.path.join(ROOT, "rust", "gsx", "src", "lib.rs")).read()
    assert "update_hit_pairs" in open(os.path.join(ROOT, "include", "gsx.hpp")).read()
    # without a device: status codes, not crashes
    assert L.gsx_viewer_set_overlay_lines(None, None, 0) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_download_overlay(None, None, None) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_overlay_device_ptrs(None, None, None, None) == _lib.GSX_ERR_INVALID_ARG


@pytest.mark.parametrize("size", R.VIEWPORTS)
def test_scenes_have_few_ambiguous_pixels(size):
    """A condition on the inputs, not a tolerance: a scene that breaks the cap is replaced."""
    w, h = size
    view, proj = R.matrices(w, h)
    for name, (lines, depth) in R.scenes(w, h).items():
        r = R.draw(lines, view, proj, w, h, depth)
        covered, ambiguous = int(r["cover"].sum()), int(r["ambiguous"].sum())
        assert ambiguous <= R.AMBIGUOUS_CAP * covered, (name, covered, ambiguous)
        assert (covered > 0) == (name != "empty"), name


def test_restatement_on_a_line_one_can_check_by_hand():
    """An axis-aligned line at view depth 5 in the middle of a 96 x 64 viewport: a rectangle of known size, one blend, one depth."""
    w, h = 96, 64
    view, proj = R.matrices(w, h)
    V = np.asarray(view, np.float64).reshape(4, 4).T
    ends = [np.linalg.inv(V) @ np.array([x, 0.0, -5.0, 1.0]) for x in (-1.0, 1.0)]  # view space (-1, 0, -5) and (1, 0, -5)
    r = R.draw(HitPair(ends[0][:3], ends[1][:3], (255, 0, 0, 128), 50.0), view, proj, w, h)
    ys, xs = np.nonzero(r["cover"])
    half = 0.01 * 50.0 * h / (2.0 * np.sqrt(26.0))  # s H / (2 |v|), |v| = sqrt(1 + 25)
    fy = (1.0 / np.tan(np.radians(30.0))) * h / 2.0
    length = 2.0 * fy / 5.0 + 2.0 * half             # the segment's 2 world units at depth 5, extended by the half-width at either end
    assert abs((ys.max() - ys.min() + 1) - 2.0 * half) <= 1.0 and abs((xs.max() - xs.min() + 1) - length) <= 1.0
    assert abs(ys.mean() + 0.5 - h / 2.0) <= 0.5 and abs(xs.mean() + 0.5 - w / 2.0) <= 0.5
    a = 128.0 / 255.0
    assert np.allclose(r["rgba"][r["cover"]], [a, 0.0, 0.0, a]) and np.allclose(r["depth"][r["cover"]], R.ndc_depth(proj, 5.0), atol=1e-6)
    assert not r["rgba"][~r["cover"]].any() and np.all(r["depth"][~r["cover"]] == 1.0)
