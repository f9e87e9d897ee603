"""CPU: what the GPU tests of gsx_render_depth_map (spec/RENDER_SPEC.md §25) stand on.

1. tests/depthmap_ref.py, the numpy reference of the walk: a hand-made pixel, a model behind continuing from the model in front, and —
   on the oracle's own projection and lists — the same frame as tests/visibility_ref.py walks, with A = 1 - T.
2. gsx_depth_map_unproject against a float64 numpy inverse of view and proj, at pixel centres and corners.
3. The header, the ctypes layer and the Rust and C++ facades declare the calls; the ABI stays 3.
4. The test conditions: for every scene the GPU tests compare with the reference, both pod kinds and both thresholds, at most 2 % of
   the pixels have an uncertain crossing and at least 25 % cross, under the oracle's projection; the three-model scene
   (visibility_scenes.THREE) as well, with its empty tiles where the GPU test needs them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from tests import common
from tests import depthmap_ref as D
from tests import visibility_ref as R
from tests import visibility_scenes as S
from wgpu_3dgs_viewer_app_amd import _lib, camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("gsx_depth_map_desc_default", "gsx_render_depth_map", "gsx_depth_map_device_ptrs", "gsx_depth_map_unproject")
THRESHOLDS = (0.5, 1.0)
NONE = D.NONE


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _oracle_lists(spec, kind=(0, 0)):
    g, cam, (w, h) = S.scene(spec)
    f = common.oracle_frame(cam, w, h)
    pr = oracle.project(f, *oracle.convert_pod(g, *kind))
    idx, nvis = oracle.depth_sort(pr["key"])
    off, lst = oracle.tile_lists(f, idx, nvis, pr["rect"])
    return f, pr, off, lst, (w, h)


def _walk(f, pr, off, lst, size, threshold):
    return D.walk(pr["mean2d"], pr["conic_opacity"], pr["key"], off, lst, size[0], size[1], f.k2, f.alpha_max, f.alpha_min, 1e-4, f.display_mode, threshold)


# ---- 1. the reference --------------------------------------------------------------------------------------------------------------------
def _key(*depths):
    return np.asarray(depths, np.float32).view(np.uint32)


def test_reference_on_a_hand_made_pixel():
    # one tile of 2 x 1 pixels, two Gaussians centred on pixel 0: isotropic conic 0.5, opacities 0.4 and 0.5, depths 2 and 3
    mean2d = np.array([[0.5, 0.5], [0.5, 0.5]], np.float32)
    conic = np.array([[0.5, 0.0, 0.5, 0.4], [0.5, 0.0, 0.5, 0.5]], np.float32)
    o0, o1 = float(np.float32(0.4)), 0.5
    ref = D.walk(mean2d, conic, _key(2.0, 3.0), [0, 2], [0, 1], 2, 1, k2=9.0)
    e1 = np.exp(-0.25)  # pixel 1: dx = 1, q = 0.5
    # pixel 0: T = 0.6 after the first (no crossing at 0.5), 0.3 after the second: the surface is the second
    assert np.allclose(ref.T[0], [(1 - o0) * (1 - o1), (1 - o0 * e1) * (1 - o1 * e1)])
    assert np.allclose(ref.A[0], 1.0 - ref.T[0]) and not ref.uncertain.any() and not ref.candidates
    assert np.allclose(ref.S[0], [o0 * 2 + (1 - o0) * o1 * 3, o0 * e1 * 2 + (1 - o0 * e1) * o1 * e1 * 3])
    assert ref.index[0, 0] == 1 and ref.layer[0, 0] == 0 and ref.surface[0, 0] == 3.0
    # pixel 1: T = 0.688 after the first, 0.420 after the second: the second as well
    assert 0.4 < ref.T[0, 1] < 0.5 and ref.index[0, 1] == 1 and ref.layer[0, 1] == 0 and ref.surface[0, 1] == 3.0
    assert np.array_equal(ref.steps[0], [2, 2])
    # at threshold 0.7 pixel 0 crosses at the first record (T = 0.6), pixel 1 at the first as well (0.688)
    ref = D.walk(mean2d, conic, _key(2.0, 3.0), [0, 2], [0, 1], 2, 1, k2=9.0, threshold=0.7)
    assert np.array_equal(ref.index[0], [0, 0]) and np.array_equal(ref.surface[0], [2.0, 2.0])
    # outside the support (k2 = 0.4 < q = 0.5) pixel 1 blends nothing
    ref = D.walk(mean2d, conic, _key(2.0, 3.0), [0, 2], [0, 1], 2, 1, k2=0.4)
    assert ref.index[0, 1] == NONE and ref.layer[0, 1] == NONE and np.isinf(ref.surface[0, 1]) and ref.A[0, 1] == 0 and ref.T[0, 1] == 1 and ref.steps[0, 1] == 0


def test_reference_thresholds_closing_and_a_model_behind():
    mean2d = np.array([[0.5, 0.5], [0.5, 0.5]], np.float32)
    conic = np.array([[0.5, 0.0, 0.5, 0.4], [0.5, 0.0, 0.5, 1.0]], np.float32)
    # threshold 1.0: the first record that lowers T at all
    ref = D.walk(mean2d, conic, _key(2.0, 3.0), [0, 2], [0, 1], 1, 1, k2=9.0, threshold=1.0)
    assert ref.index[0, 0] == 0 and ref.surface[0, 0] == 2.0 and not ref.uncertain.any()
    # an opaque second record closes the pixel for certain: T = 0, A = 1
    assert ref.T[0, 0] == 0.0 and ref.A[0, 0] == pytest.approx(1.0)
    # a record of opacity 0 decides nothing, at either threshold
    conic0 = np.array([[0.5, 0.0, 0.5, 0.0], [0.5, 0.0, 0.5, 0.7]], np.float32)
    ref0 = D.walk(mean2d, conic0, _key(2.0, 3.0), [0, 2], [0, 1], 1, 1, k2=9.0, threshold=1.0)
    assert ref0.index[0, 0] == 1 and not ref0.uncertain.any()
    # a T that lands on the threshold is an uncertain crossing: the record and the next are candidates
    half = np.array([[0.5, 0.0, 0.5, 0.5], [0.5, 0.0, 0.5, 0.5]], np.float32)
    refh = D.walk(mean2d, half, _key(2.0, 3.0), [0, 2], [0, 1], 1, 1, k2=9.0, threshold=0.5)
    assert refh.uncertain[0, 0] and refh.candidates[(0, 0)] == [(0, 0), (0, 1)] and not refh.allow_none[0, 0]
    # ... and with nothing behind it, "no crossing" is one too
    refh = D.walk(mean2d[:1], half[:1], _key(2.0), [0, 1], [0], 1, 1, k2=9.0, threshold=0.5)
    assert refh.uncertain[0, 0] and refh.candidates[(0, 0)] == [(0, 0)] and refh.allow_none[0, 0]
    # a model behind continues: front model T = 0.6 (no crossing), the model behind crosses with its first record, layer 0
    front = D.walk(mean2d[:1], conic[:1], _key(2.0), [0, 1], [0], 1, 1, k2=9.0, layer=1)
    assert front.index[0, 0] == NONE
    both = D.walk(mean2d[:1], half[:1], _key(1.5), [0, 1], [0], 1, 1, k2=9.0, layer=0, state=front)
    o0 = float(np.float32(0.4))
    assert both.layer[0, 0] == 0 and both.index[0, 0] == 0 and both.surface[0, 0] == 1.5 and both.steps[0, 0] == 2
    assert both.T[0, 0] == pytest.approx((1 - o0) * 0.5) and both.S[0, 0] == pytest.approx(o0 * 2.0 + (1 - o0) * 0.5 * 1.5)
    assert front.steps[0, 0] == 1 and front.index[0, 0] == NONE, "the state handed in is not changed"
    # the bounds grow with the blends: A's is s * 1.5 * 2^-21, S's is at least s * 2^-21 * the last depth
    assert both.bound_A[0, 0] == 2 * 1.5 * 2.0 ** -21 and both.bound_S[0, 0] > 2 * 2.0 ** -21 * 1.5


@pytest.mark.parametrize("name", ["5x3", "7x5"])
def test_reference_frame_is_the_visibility_references(name):
    f, pr, off, lst, (w, h) = _oracle_lists(S.REF[name])
    ref = _walk(f, pr, off, lst, (w, h), 0.5)
    vis = R.walk(pr["mean2d"], pr["conic_opacity"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 1e-4, f.display_mode)
    assert np.array_equal(ref.T, vis.T)
    assert np.abs(ref.A - (1.0 - ref.T)).max() <= 1e-12
    depth = pr["key"].view(np.float32)
    crossed = ref.index != NONE
    assert crossed.any() and np.array_equal(ref.surface[crossed], depth[ref.index[crossed]])
    # the expected depth lies between the nearest and the farthest visible depth
    vis_d = depth[pr["key"] != 0xFFFFFFFF]
    cov = ref.A > 0
    assert np.all(ref.S[cov] / ref.A[cov] >= vis_d.min() * (1 - 1e-9)) and np.all(ref.S[cov] / ref.A[cov] <= vis_d.max() * (1 + 1e-9))


# ---- 2. unproject ------------------------------------------------------------------------------------------------------------------------
def test_unproject_matches_a_float64_inverse():
    L = _lib.load()
    w, h = 83, 51
    for pose in (5, 6, 17):
        cam = camera.orbit_pose(pose)
        view = np.ascontiguousarray(cam.view(), np.float32).reshape(16)
        proj = np.ascontiguousarray(cam.projection(w / h), np.float32).reshape(16)
        V, P = view.astype(np.float64).reshape(4, 4).T, proj.astype(np.float64).reshape(4, 4).T  # column-major
        inv = np.linalg.inv(P @ V)
        for px, py in ((0.5, 0.5), (41.5, 25.5), (82.5, 50.5), (0.0, 0.0), (83.0, 51.0), (83.0, 0.0), (0.0, 51.0), (12.25, 40.75)):
            for d in (0.37, 2.5, 40.0):
                clip = P @ np.array([0.0, 0.0, -d, 1.0])
                ndc = np.array([2.0 * px / w - 1.0, 1.0 - 2.0 * py / h, clip[2] / clip[3], 1.0])
                want = inv @ ndc
                want = want[:3] / want[3]
                got = (C.c_float * 3)()
                st = L.gsx_depth_map_unproject(view.ctypes.data_as(C.POINTER(C.c_float)), proj.ctypes.data_as(C.POINTER(C.c_float)), w, h, px, py, d, got)
                assert st == 0, L.gsx_last_error_string()
                # float64 inside: what is left is the rounding of the three results to float32 (and of d, px, py on the way in)
                assert np.abs(np.asarray(got, np.float64) - want).max() <= 4e-7 * max(1.0, np.abs(want).max(), d)
                # and the point projects back to the pixel at that view depth
                back = P @ V @ np.append(np.asarray(got, np.float64), 1.0)
                assert abs((back[0] / back[3] * 0.5 + 0.5) * w - px) <= 1e-3 and abs((0.5 - back[1] / back[3] * 0.5) * h - py) <= 1e-3
                assert abs(-(V @ np.append(np.asarray(got, np.float64), 1.0))[2] - d) <= 1e-5 * max(1.0, d)
    bad = (C.c_float * 3)()
    assert L.gsx_depth_map_unproject(None, None, w, h, 0.0, 0.0, 1.0, bad) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_depth_map_unproject" in L.gsx_last_error_string()
    zero = (C.c_float * 16)()
    assert L.gsx_depth_map_unproject(zero, zero, w, h, 0.0, 0.0, 1.0, bad) == _lib.GSX_ERR_INVALID_ARG
    ident = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    assert L.gsx_depth_map_unproject(ident, ident, 0, h, 0.0, 0.0, 1.0, bad) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_depth_map_unproject(ident, ident, w, h, 0.0, 0.0, float("nan"), bad) == _lib.GSX_ERR_INVALID_ARG
    # the Python helper
    from wgpu_3dgs_viewer_app_amd.viewer import depth_map_unproject

    p = depth_map_unproject(ident, ident, (2, 2), 1.0, 1.0, 3.0)
    assert np.array_equal(p, np.array([0.0, 0.0, -3.0], np.float32))


# ---- 3. header and facades -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^#define GSX_DEPTH_MAP_NDC 1u", hdr, re.M) and _lib.GSX_DEPTH_MAP_NDC == 1
    assert re.search(r"typedef struct gsx_depth_map_desc \{ uint32_t flags; float threshold; uint32_t reserved\[2\]; \} gsx_depth_map_desc;", hdr)
    assert re.search(r"typedef struct gsx_depth_map_stats_t \{ uint64_t n_covered, n_crossed; float surface_min, surface_max; uint32_t models, reserved; \} "
                     r"gsx_depth_map_stats_t;", hdr)
    assert re.search(r"^void gsx_depth_map_desc_default\(gsx_depth_map_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_render_depth_map\(gsx_viewer\* v, const char\* const\* keys_far_to_near, uint32_t n_keys, const gsx_depth_map_desc\* desc,\s*"
                     r"float\* out_surface, float\* out_sum, float\* out_alpha, float\* out_transmittance,\s*uint32_t\* out_index, uint32_t\* out_layer, "
                     r"gsx_depth_map_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_depth_map_device_ptrs\(gsx_viewer\* v, void\*\* surface, void\*\* sum, void\*\* alpha, void\*\* transmittance,\s*"
                     r"void\*\* index, void\*\* layer, void\*\* ndc, uint32_t\* width, uint32_t\* height\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_depth_map_unproject\(const float view\[16\], const float proj\[16\], uint32_t width, uint32_t height,\s*"
                     r"float px, float py, float view_depth, float out_world\[3\]\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    block = hdr[hdr.index("---- depth map:"):hdr.index("#define GSX_DEPTH_MAP_NDC")]
    # the refusals are out of scope by design, the ordering of the ndc plane is spelt out, and the header says so
    assert "Out of scope (GSX_ERR_INVALID_ARG, by design, not forgotten)" in block
    for what in ("GSX_DEPTH_LESS", "overlay lines or mask gizmos", "a band", "an external framebuffer", "a sharded model", "communicator"):
        assert what in block[block.index("Out of scope (GSX_ERR_INVALID_ARG, by design"):][:400]
    for what in ("tightly packed [height][width] float32", "gsx_viewer_set_depth_buffer_device", "on the viewer's\n *      stream", "reads behind them",
                 "parity in that band", "section 25", "the next gsx_render_depth_map, a viewport change or gsx_viewer_destroy"):
        assert what in block, what
    assert "## 25. Depth map [BUILD-SPEC]" in _read("spec", "RENDER_SPEC.md")


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.DepthMapDesc) == 16 and offsets(_lib.DepthMapDesc) == {"flags": 0, "threshold": 4, "reserved": 8}
    assert C.sizeof(_lib.DepthMapStats) == 32
    assert offsets(_lib.DepthMapStats) == {"n_covered": 0, "n_crossed": 8, "surface_min": 16, "surface_max": 20, "models": 24, "reserved": 28}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_depthmap.cpp")
    assert "static_assert(sizeof(gsx_depth_map_desc) == 16 && sizeof(gsx_depth_map_stats_t) == 32" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[1:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_depth_map_desc", "gsx_depth_map_stats_t"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub const GSX_DEPTH_MAP_NDC: u32 = 1;" in rust_sys and "pub threshold: f32" in rust_sys and "ndc: *mut *mut c_void" in rust_sys
    for method in ("render_depth_map", "depth_map_device_ptrs", "depth_map_unproject"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.DepthMapDesc(7, 7.0, (C.c_uint32 * 2)(7, 7))
    L.gsx_depth_map_desc_default(C.byref(d))
    assert (d.flags, d.threshold, tuple(d.reserved)) == (0, 0.5, (0, 0))
    L.gsx_depth_map_desc_default(None)
    # without a device: a status code and a message, not a crash
    keys = (C.c_char_p * 1)(b"a")
    assert L.gsx_render_depth_map(None, keys, 1, C.byref(d), None, None, None, None, None, None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_render_depth_map" in L.gsx_last_error_string()
    assert L.gsx_depth_map_device_ptrs(None, None, None, None, None, None, None, None, None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_depth_map_device_ptrs" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import DepthMap, MultiModelViewer

    assert all(callable(getattr(MultiModelViewer, m)) for m in ("render_depth_map", "depth_map_device_ptrs"))
    assert [f.name for f in __import__("dataclasses").fields(DepthMap)][:6] == ["surface", "sum", "alpha", "transmittance", "index", "layer"]


def test_the_build_lists_the_sources_and_the_frame_path_is_shared_not_copied():
    mk = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_depthmap.hip" in mk and "gsx_api_depthmap.cpp" in mk
    kernels = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_depthmap.hip")
    # integer atomics only, and none in the walk: a floating-point atomic would break "the same bytes on every call"
    assert not re.search(r"atomic(Add|Max|Min)\s*\(\s*(\(float|\(double)", kernels) and "unsafeAtomic" not in kernels and "atomicAdd_f" not in kernels
    walk = kernels[kernels.index("void k_depth_tiles("):kernels.index("struct DepthStatsPartial")]
    assert "atomic" not in walk and "rec_c" not in walk and "rec_key" in walk
    # FrameIsolation is written once, in a header both calls include
    iso = _read("wgpu_3dgs_viewer_app_amd", "csrc", "frame_isolation.h")
    assert "struct FrameIsolation {" in iso
    for name in ("gsx_api_visibility.cpp", "gsx_api_depthmap.cpp"):
        src = _read("wgpu_3dgs_viewer_app_amd", "csrc", name)
        assert '#include "frame_isolation.h"' in src and "struct FrameIsolation" not in src and "FrameIsolation iso(v, m);" in src


# ---- 4. the test conditions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("kind", list(S.KINDS), ids=list(S.KINDS))
@pytest.mark.parametrize("name", list(S.REF))
def test_reference_scenes_stay_inside_the_cap(name, kind, threshold):
    f, pr, off, lst, size = _oracle_lists(S.REF[name], S.KINDS[kind])
    ref = _walk(f, pr, off, lst, size, threshold)
    unc, crossed = float(ref.uncertain.mean()), float((ref.index != NONE).mean())
    print(f"depth map {name} {kind} threshold {threshold}: {int(ref.uncertain.sum())} of {ref.uncertain.size} pixels uncertain, {crossed:.1%} cross, "
          f"L_max {ref.l_max}, most blends of a pixel {int(ref.steps.max())}")
    assert unc <= S.UNCERTAIN_CAP, f"{name}: {unc:.2%} of the pixels have an uncertain crossing"
    assert crossed >= 0.25, f"{name}: only {crossed:.2%} of the pixels cross"
    if name == "long-list":
        assert ref.l_max > 256, "two LDS batches and the pipeline's third gather"
    if name == "partial":
        assert size[0] % 16 and size[1] % 2, "partial tiles, a lane's second pixel outside"
    if threshold == 1.0:
        assert np.array_equal(ref.index == NONE, ref.A == 0.0), "the front surface: a crossing exactly where anything was blended"


def test_the_three_model_scene_stays_inside_the_cap_and_has_its_empty_tiles():
    """visibility_scenes.THREE under the oracle's projection, walked near to far as test_gpu_depthmap.py walks the device's lists: the
    cap and the floor of the GPU test hold for the reference alone, every model holds surfaces, "mid" has no entry in the right three
    tile columns and "near" none in the left three, and "near" crosses pixels in tiles where the launches of "mid" find nothing."""
    models, cam, (w, h) = S.three_models()
    keys = list(models)
    assert keys == ["far", "mid", "near"] and (w, h) == (83, 51) and all(50 <= g.shape[0] <= 500 for g in models.values())
    f = common.oracle_frame(cam, w, h)
    assert (f.tiles_x, f.tiles_y) == (6, 4)
    ref, counts = None, {}
    for layer in (2, 1, 0):  # the last key first
        pr = oracle.project(f, *oracle.convert_pod(models[keys[layer]], 0, 0))
        idx, nvis = oracle.depth_sort(pr["key"])
        off, lst = oracle.tile_lists(f, idx, nvis, pr["rect"])
        counts[keys[layer]] = np.diff(off).reshape(4, 6)
        ref = D.walk(pr["mean2d"], pr["conic_opacity"], pr["key"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 1e-4, f.display_mode, 0.5, layer=layer, state=ref)
    unc, crossed = float(ref.uncertain.mean()), float((ref.index != NONE).mean())
    print(f"depth map of three models: {int(ref.uncertain.sum())} of {ref.uncertain.size} pixels uncertain, {crossed:.1%} cross, layers "
          f"{[int((ref.layer == k).sum()) for k in range(3)]}, entries a tile: far {counts['far'].tolist()}, mid {counts['mid'].tolist()}, near {counts['near'].tolist()}")
    assert unc <= S.UNCERTAIN_CAP and crossed >= 0.25
    assert all((ref.layer == k).any() for k in range(3)), "every model holds surfaces"
    assert (counts["far"] > 0).all() and not counts["mid"][:, 3:].any() and (counts["mid"][:, :3] > 0).all()
    assert not counts["near"][:, :3].any() and (counts["near"][:, 3:] > 0).all()
    # a pixel "near" crosses lies in a tile where the launch of "mid" returns early: the planes must keep it
    assert (ref.layer[:, 48:] == 2).any()
