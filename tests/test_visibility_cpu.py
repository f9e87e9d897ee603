"""CPU: what the GPU tests of gsx_model_visibility (spec/RENDER_SPEC.md §24) stand on.

1. tests/visibility_ref.py, the numpy reference of the walk, against oracle.composite_tiles on the oracle's own projection and lists:
   per pixel sum_g w * rgb_g and the final T, to within the t_epsilon tail (the oracle blends everything; the reference, like the
   device, closes a pixel at T < t_epsilon) — tests/test_gpu_fullsize_oracle.py's stated difference.
2. The header, the ctypes layer and the Rust and C++ facades declare the three calls; the ABI stays 3.
3. The test conditions: for every seed the GPU tests compare with the reference, and both pod kinds, at most 2 % of the Gaussians
   have an uncertain pair under the oracle's projection, and the certain decisions keep their margin."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from tests import common
from tests import visibility_ref as R
from tests import visibility_scenes as S
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("gsx_visibility_desc_default", "gsx_visibility_select_desc_default", "gsx_model_visibility", "gsx_model_select_visibility",
             "gsx_model_visibility_reset")
# tests/test_gpu_fullsize_oracle.py, FB_OBSERVED: "the compositor stops a pixel at T < t_epsilon = 1e-4 (the oracle blends everything)"
FB_OBSERVED = 4e-4
INRIA = dict(alpha_max=0.99, alpha_min=1.0 / 255.0)


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _oracle_lists(spec, kind=(0, 0), display_mode=0, params=None):
    g, cam, (w, h) = S.scene(spec)
    sp = None
    if params:
        sp = oracle.SpecParams.default()
        for k, val in params.items():
            setattr(sp, k, val)
    f = common.oracle_frame(cam, w, h, display_mode=display_mode, params=sp)
    pr = oracle.project(f, *oracle.convert_pod(g, *kind))
    idx, nvis = oracle.depth_sort(pr["key"])
    off, lst = oracle.tile_lists(f, idx, nvis, pr["rect"])
    return f, pr, off, lst, (w, h)


def _walk(f, pr, off, lst, size, rgb=True):
    return R.walk(pr["mean2d"], pr["conic_opacity"], off, lst, size[0], size[1], f.k2, f.alpha_max, f.alpha_min, 1e-4, f.display_mode,
                  rgb=pr["rgb"] if rgb else None)


# ---- 1. the reference against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,table,display_mode,params", [
    ("5x3", S.REF, 0, None), ("partial", S.REF, 0, None), ("long-list", S.REF, 0, None), ("7x5", S.REF, 0, None),
    ("5x3", S.SOLID, 0, None), ("partial", S.SOLID, 0, INRIA), ("one-tile", S.SOLID, 1, None), ("long-list", S.SOLID, 2, INRIA), ("7x5", S.SOLID, 0, None)])
def test_reference_frame_is_the_oracles_to_the_t_epsilon_tail(name, table, display_mode, params):
    f, pr, off, lst, (w, h) = _oracle_lists(table[name], display_mode=display_mode, params=params)
    ref = _walk(f, pr, off, lst, (w, h))
    fb = oracle.new_framebuffer(f)
    oracle.composite_tiles(f, pr, off, lst, fb)
    assert ref.n_pairs > 0
    assert np.abs(ref.T - fb[..., 3]).max() <= FB_OBSERVED
    assert np.abs(ref.rgb - fb[..., :3]).max() <= FB_OBSERVED
    if table is S.SOLID and name != "7x5":
        assert (ref.T < 1e-4).any(), "the solid scenes close pixels"
    # what closing costs is the tail alone: an open pixel is the oracle's to float32 rounding
    open_px = ref.T >= 1e-4
    assert np.abs(ref.T - fb[..., 3])[open_px].max(initial=0.0) <= (ref.l_max + 2) * 2.0 ** -21
    # the telescoping sum, in float64: sum_g weight_g = sum_p (1 - T_p) when no pixel ever closes (t_epsilon = 0: every pair counts)
    own = R.walk(pr["mean2d"], pr["conic_opacity"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 0.0, f.display_mode)
    assert abs(own.weight_hi.sum() - (1.0 - own.T).sum()) <= 1e-9 * max(own.n_pairs, 1)


def test_reference_on_a_hand_made_pixel():
    # one tile of 2 x 1 pixels, two Gaussians centred on pixel 0: isotropic conic 0.5, opacities 0.5 and 0.25
    mean2d = np.array([[0.5, 0.5], [0.5, 0.5]], np.float32)
    conic = np.array([[0.5, 0.0, 0.5, 0.5], [0.5, 0.0, 0.5, 0.25]], np.float32)
    ref = R.walk(mean2d, conic, [0, 2], [0, 1], 2, 1, k2=9.0)
    e1 = np.exp(-0.25)  # pixel 1: dx = 1, q = 0.5
    assert np.allclose(ref.peak_lo, [0.5, 0.5 * 0.25]) and np.array_equal(ref.pixels_lo, [2, 2])
    assert np.allclose(ref.weight_lo, [0.5 + 0.5 * e1, 0.5 * 0.25 + (1 - 0.5 * e1) * 0.25 * e1])
    assert np.allclose(ref.T[0], [0.5 * 0.75, (1 - 0.5 * e1) * (1 - 0.25 * e1)]) and not ref.uncertain.any()
    # an opaque front Gaussian closes pixel 0 for certain: the second gets nothing from it
    conic[0, 3] = 1.0
    ref = R.walk(mean2d, conic, [0, 2], [0, 1], 2, 1, k2=9.0)
    assert ref.pixels_lo[1] == 1 and ref.pixels_hi[1] == 1 and ref.T[0, 0] == 0.0
    # alpha_min removes a pair, alpha_max clamps one
    ref = R.walk(mean2d, conic, [0, 2], [0, 1], 2, 1, k2=9.0, alpha_max=0.99, alpha_min=0.2)
    assert ref.peak_lo[0] == pytest.approx(0.99) and ref.pixels_lo[1] == 1 and ref.peak_lo[1] == pytest.approx(0.01 * 0.25)


# ---- 2. header and facades -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^#define GSX_VIS_ACCUMULATE 1u", hdr, re.M) and _lib.GSX_VIS_ACCUMULATE == 1
    assert re.search(r"typedef enum gsx_visibility_measure \{ GSX_VIS_PEAK = 0, GSX_VIS_WEIGHT = 1, GSX_VIS_PIXELS = 2 \}", hdr)
    assert (_lib.GSX_VIS_PEAK, _lib.GSX_VIS_WEIGHT, _lib.GSX_VIS_PIXELS) == (0, 1, 2)
    assert re.search(r"typedef struct gsx_visibility_desc \{ uint32_t flags; uint32_t reserved\[3\]; \} gsx_visibility_desc;", hdr)
    assert re.search(r"typedef struct gsx_visibility_stats_t \{\s*uint64_t n_visible;[^}]*uint64_t n_seen;[^}]*uint64_t n_pairs;[^}]*uint64_t weight_fixed;[^}]*"
                     r"float peak_max;[^}]*uint32_t views;[^}]*\} gsx_visibility_stats_t;", hdr)
    assert re.search(r"typedef struct gsx_visibility_select_desc \{\s*uint32_t measure;[^}]*uint32_t filter;[^}]*uint32_t selection_op;[^}]*uint32_t reserved;[^}]*"
                     r"double lo, hi;[^}]*\} gsx_visibility_select_desc;", hdr)
    assert re.search(r"^gsx_status gsx_model_visibility\(gsx_viewer\* v, const char\* key, const gsx_visibility_desc\* desc, float\* out_peak /\*[^/]*\*/,\s*"
                     r"double\* out_weight /\*[^/]*\*/, uint32_t\* out_pixels /\*[^/]*\*/,\s*float\* out_transmittance /\*[^/]*\*/, "
                     r"gsx_visibility_stats_t\* out /\*[^/]*\*/\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_visibility\(gsx_viewer\* v, const char\* key, const gsx_visibility_select_desc\* desc, uint64_t\* out_hit,\s*"
                     r"uint64_t\* out_selected\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_visibility_reset\(gsx_viewer\* v, const char\* key\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    # the four refusals are out of scope by design, and the header says so
    assert "Out of scope (GSX_ERR_INVALID_ARG, by design, not forgotten)" in hdr
    for what in ("GSX_DEPTH_LESS", "overlay lines or mask gizmos", "a band", "an external framebuffer", "a sharded model"):
        assert what in hdr[hdr.index("Out of scope (GSX_ERR_INVALID_ARG, by design"):][:400]
    assert "section 24" in hdr and "## 24. Visibility [BUILD-SPEC]" in _read("spec", "RENDER_SPEC.md")


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.VisibilityDesc) == 16 and offsets(_lib.VisibilityDesc) == {"flags": 0, "reserved": 4}
    assert C.sizeof(_lib.VisibilitySelectDesc) == 32
    assert offsets(_lib.VisibilitySelectDesc) == {"measure": 0, "filter": 4, "selection_op": 8, "reserved": 12, "lo": 16, "hi": 24}
    assert C.sizeof(_lib.VisibilityStats) == 40
    assert offsets(_lib.VisibilityStats) == {"n_visible": 0, "n_seen": 8, "n_pairs": 16, "weight_fixed": 24, "peak_max": 32, "views": 36}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_visibility.cpp")
    assert "static_assert(sizeof(gsx_visibility_desc) == 16 && sizeof(gsx_visibility_select_desc) == 32 && sizeof(gsx_visibility_stats_t) == 40" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[2:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_visibility_desc", "gsx_visibility_select_desc", "gsx_visibility_stats_t"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub const GSX_VIS_ACCUMULATE: u32 = 1;" in rust_sys and "pub lo: f64, pub hi: f64" in rust_sys and "out_weight: *mut f64" in rust_sys
    for method in ("visibility", "select_visibility", "visibility_reset", "visibility_orbit"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.VisibilityDesc(7, (C.c_uint32 * 3)(7, 7, 7))
    L.gsx_visibility_desc_default(C.byref(d))
    assert (d.flags, tuple(d.reserved)) == (0, (0, 0, 0))
    sd = _lib.VisibilitySelectDesc(7, 7, 7, 7, 7.0, 7.0)
    L.gsx_visibility_select_desc_default(C.byref(sd))
    assert (sd.measure, sd.filter, sd.selection_op, sd.reserved, sd.hi) == (_lib.GSX_VIS_PEAK, 0, 0, 0, np.inf)
    assert sd.lo == float(np.float32(1e-45)) and np.float32(sd.lo) > 0  # the smallest positive float: "seen at all"
    L.gsx_visibility_desc_default(None)
    L.gsx_visibility_select_desc_default(None)
    # without a device: a status code and a message, not a crash
    assert L.gsx_model_visibility(None, b"a", C.byref(d), None, None, None, None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_visibility" in L.gsx_last_error_string()
    assert L.gsx_model_select_visibility(None, b"a", C.byref(sd), None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_visibility" in L.gsx_last_error_string()
    assert L.gsx_model_visibility_reset(None, b"a") == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_visibility_reset" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("visibility", "select_visibility", "visibility_reset", "visibility_orbit"))


def test_the_build_lists_the_sources_and_the_frame_path_is_not_the_kernels():
    mk = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_visibility.hip" in mk and "gsx_api_visibility.cpp" in mk
    kernels = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_visibility.hip")
    # integer atomics only: a floating-point atomic would break "the same bytes on every call"
    assert not re.search(r"atomic(Add|Max|Min)\s*\(\s*(\(float|\(double|&\w+\.\w*f\b)", kernels) and "unsafeAtomic" not in kernels and "atomicAdd_f" not in kernels
    assert '#include "wave_reduce.h"' in kernels and '#include "selection_write.h"' in kernels
    assert "select_write(" in kernels and "launch_select_finish(" in kernels and "group_fold(" in kernels


# ---- 3. the test conditions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(S.KINDS), ids=list(S.KINDS))
@pytest.mark.parametrize("name", list(S.REF))
def test_reference_scenes_stay_inside_the_uncertain_cap(name, kind):
    f, pr, off, lst, size = _oracle_lists(S.REF[name], S.KINDS[kind])
    ref = _walk(f, pr, off, lst, size, rgb=False)
    assert ref.uncertain.mean() <= S.UNCERTAIN_CAP, f"{name}: {ref.uncertain.mean():.2%} of the Gaussians have an uncertain pair"
    assert ref.margin > 1.0  # (by construction: a decision is certain beyond the tolerance)
    assert (ref.pixels_hi > 0).sum() >= 0.8 * pr["n_visible"], "most of what is visible blends somewhere"
    if name == "long-list":
        assert ref.l_max > 256, "two LDS batches and the pipeline's third gather"
    if name == "partial":
        assert size[0] % 16 and size[1] % 2, "partial tiles, a lane's second pixel outside"


def test_some_reference_scene_closes_a_pixel():
    closed = 0
    for name in ("5x3", "partial"):
        f, pr, off, lst, size = _oracle_lists(S.REF[name])
        closed += int((_walk(f, pr, off, lst, size, rgb=False).T < 1e-4).sum())
    assert closed > 0, "the closing decision is part of what the reference checks"
