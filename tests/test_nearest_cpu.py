"""Model nearest across models (gsx_model_nearest, gsx_model_select_nearest, gsx_model_align_step; spec §23) without a device: the
entry points and the structs in the header, the library, the bindings and the facades; the rules of csrc/nearest_math.h, the signed
cell of csrc/neighbors_math.h and the solve of csrc/align_math.h — played by tests/nearest_driver.cpp, a stand-alone program built
with the address and undefined-behaviour sanitizers and run as a child process, through a plain C++ version of the whole search —
against an O(n m) loop and against the numpy restatement tests/nearest_ref.py, bit for bit on index and d2; and the solve against
numpy's float64 SVD."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import nearest_ref as R
from tests import neighbors_ref as N
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCTIONS = ("gsx_nearest_desc_default", "gsx_model_nearest", "gsx_model_select_nearest", "gsx_model_align_step")
IDENTITY = np.eye(3, 4, dtype=F)


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    for name, value in (("GSX_NEAREST_NONE", "0xFFFFFFFF"), ("GSX_NEAREST_MODEL_TRANSFORMS", "1"), ("GSX_NEAREST_SELECT_RANGE", "0"),
                        ("GSX_NEAREST_SELECT_TRANSFER", "1"), ("GSX_ALIGN_SCALE", "1")):
        assert re.search(rf"^#define {name} {value}u", hdr, re.M) and getattr(_lib, name) == int(value, 0)
    assert (R.NONE, R.MODEL_TRANSFORMS, R.SELECT_RANGE, R.SELECT_TRANSFER, R.ALIGN_SCALE) == (0xFFFFFFFF, 1, 0, 1, 1)
    assert re.search(r"typedef struct gsx_nearest_desc \{\s*uint32_t src_filter; uint32_t dst_filter; uint32_t flags; uint32_t grid_bits;[^}]*"
                     r"float max_distance; float radius_hint; uint32_t max_rounds; uint32_t reserved;\s*float xform\[12\];\s*\} gsx_nearest_desc;", hdr)
    assert re.search(r"typedef struct gsx_nearest_stats_t \{\s*uint64_t count; uint64_t n_nonfinite; uint64_t targets; uint64_t targets_nonfinite; "
                     r"uint64_t n_found; uint64_t n_brute;\s*double mean; double rms;\s*float d_min; float d_max; float first_radius; uint32_t rounds; "
                     r"uint32_t grid_bits; uint32_t reserved;\s*float xform\[12\];\s*\} gsx_nearest_stats_t;", hdr)
    assert re.search(r"typedef struct gsx_nearest_select_desc \{\s*gsx_nearest_desc nearest;\s*uint32_t selection_op; uint32_t mode; float lo; float hi;"
                     r"[^}]*\} gsx_nearest_select_desc;", hdr)
    assert re.search(r"typedef struct gsx_align_desc \{ gsx_nearest_desc nearest; uint32_t flags; uint32_t reserved; \} gsx_align_desc;", hdr)
    assert re.search(r"typedef struct gsx_align_step_t \{\s*double pos\[3\]; double quat\[4\]; double scale;\s*float xform_next\[12\];\s*uint64_t n_pairs; "
                     r"double rms_before;\s*uint32_t degenerate; uint32_t reserved;\s*gsx_nearest_stats_t nearest;\s*\} gsx_align_step_t;", hdr)
    assert re.search(r"^void gsx_nearest_desc_default\(gsx_nearest_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_nearest\(gsx_viewer\* v, const char\* src_key, const char\* dst_key, const gsx_nearest_desc\* desc,\s*"
                     r"uint32_t\* out_index /\*[^/]*\*/, float\* out_d2 /\*[^/]*\*/,\s*gsx_nearest_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_nearest\(gsx_viewer\* v, const char\* src_key, const char\* dst_key, const gsx_nearest_select_desc\* desc, "
                     r"uint64_t\* out_hit,\s*uint64_t\* out_selected, gsx_nearest_stats_t\* out_stats[^)]*\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_align_step\(gsx_viewer\* v, const char\* src_key, const char\* dst_key, const gsx_align_desc\* desc, "
                     r"gsx_align_step_t\* out\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    assert "§23" in hdr and "## 23. Model nearest (across models) [BUILD-SPEC]" in _read("spec", "RENDER_SPEC.md")


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.NearestDesc) == 80
    assert offsets(_lib.NearestDesc) == {"src_filter": 0, "dst_filter": 4, "flags": 8, "grid_bits": 12, "max_distance": 16, "radius_hint": 20,
                                         "max_rounds": 24, "reserved": 28, "xform": 32}
    assert C.sizeof(_lib.NearestStats) == 136
    assert offsets(_lib.NearestStats) == {"count": 0, "n_nonfinite": 8, "targets": 16, "targets_nonfinite": 24, "n_found": 32, "n_brute": 40, "mean": 48,
                                          "rms": 56, "d_min": 64, "d_max": 68, "first_radius": 72, "rounds": 76, "grid_bits": 80, "reserved": 84, "xform": 88}
    assert C.sizeof(_lib.NearestSelectDesc) == 96
    assert offsets(_lib.NearestSelectDesc) == {"nearest": 0, "selection_op": 80, "mode": 84, "lo": 88, "hi": 92}
    assert C.sizeof(_lib.AlignDesc) == 88 and offsets(_lib.AlignDesc) == {"nearest": 0, "flags": 80, "reserved": 84}
    assert C.sizeof(_lib.AlignStep) == 272
    assert offsets(_lib.AlignStep) == {"pos": 0, "quat": 24, "scale": 56, "xform_next": 64, "n_pairs": 112, "rms_before": 120, "degenerate": 128,
                                       "reserved": 132, "nearest": 136}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_nearest.cpp")
    assert "static_assert(sizeof(gsx_nearest_desc) == 80 && sizeof(gsx_nearest_stats_t) == 136 && sizeof(gsx_nearest_select_desc) == 96" in api
    assert "static_assert(sizeof(gsx_align_desc) == 88 && sizeof(gsx_align_step_t) == 272" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[1:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_nearest_desc", "gsx_nearest_stats_t", "gsx_nearest_select_desc", "gsx_align_desc", "gsx_align_step_t"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub const GSX_NEAREST_NONE: u32 = 0xFFFF_FFFF;" in rust_sys and "pub mean: f64, pub rms: f64" in rust_sys
    for method in ("nearest", "select_nearest", "align_step", "align"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.NearestDesc(7, 7, 7, 7, 7.0, 7.0, 7, 7, (C.c_float * 12)(*([7.0] * 12)))
    L.gsx_nearest_desc_default(C.byref(d))
    assert (d.src_filter, d.dst_filter, d.flags, d.grid_bits, d.max_distance, d.radius_hint, d.max_rounds, d.reserved) == (0, 0, 0, 0, 0.0, 0.0, 0, 0)
    assert np.array_equal(np.array(d.xform[:], F).reshape(3, 4), IDENTITY)
    L.gsx_nearest_desc_default(None)
    # without a device: a status code and a message, not a crash
    index, d2, stats = (C.c_uint32 * 4)(), (C.c_float * 4)(), _lib.NearestStats()
    assert L.gsx_model_nearest(None, b"a", b"b", C.byref(d), index, d2, C.byref(stats)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_nearest" in L.gsx_last_error_string()
    sd = _lib.NearestSelectDesc(d, 0, _lib.GSX_NEAREST_SELECT_TRANSFER, 0.0, 0.0)
    assert L.gsx_model_select_nearest(None, b"a", b"b", C.byref(sd), None, None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_nearest" in L.gsx_last_error_string()
    step = _lib.AlignStep()
    assert L.gsx_model_align_step(None, b"a", b"b", C.byref(_lib.AlignDesc(d, 0, 0)), C.byref(step)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_align_step" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("nearest", "select_nearest", "align_step", "align"))


def test_the_rules_have_one_copy_and_the_build_lists_the_sources():
    kernels, api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_nearest.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_nearest.cpp")
    math_h, align_h, driver = (_read("wgpu_3dgs_viewer_app_amd", "csrc", "nearest_math.h"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "align_math.h"),
                               _read("tests", "nearest_driver.cpp"))
    nb_h = _read("wgpu_3dgs_viewer_app_amd", "csrc", "neighbors_math.h")
    for text in (kernels, api, driver):
        assert '#include "nearest_math.h"' in text
        for rule in ("inline float nearest_map_row(", "inline bool nearest_better(", "inline float nearest_cap2(", "inline float nearest_round_radius(",
                     "inline int32_t nb_cell_signed(", "inline float nb_d2(", "inline bool knn_go_brute(", "inline AlignDelta align_solve("):
            assert rule not in text
    for rule in ("inline float nearest_map_row(", "inline bool nearest_better(", "inline float nearest_cap2(", "inline float nearest_reach2(",
                 "inline bool nearest_final(", "inline float nearest_round_radius(", "inline void nearest_model_matrix("):
        assert math_h.count(rule) == 1, rule
    assert nb_h.count("inline int32_t nb_cell_signed(") == 1 and nb_h.count("inline uint32_t nb_cell(") == 1  # the unsigned cell is untouched
    assert '#include "knn_math.h"' in math_h and "merge_unit_quat(" in math_h and "nb_d2(" not in math_h.split("#pragma once")[1]
    assert align_h.count("inline AlignDelta align_solve(") == 1 and "hip" not in align_h.split("#pragma once")[1].lower()
    assert '#include "align_math.h"' in api and '#include "align_math.h"' in driver
    assert "below the origin" in _read("wgpu_3dgs_viewer_app_amd", "csrc", "neighbors_grid.h").lower()  # the proof is extended in writing
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_nearest.hip" in makefile and "gsx_api_nearest.cpp" in makefile and "-ffp-contract=off" in makefile
    # the loop over the rounds has one copy too: the library and the driver run radius_search.h, and neither decides the fallback itself
    search = driver.split("static void search(")[1].split("\n}\n")[0]
    assert '#include "radius_search.h"' in api and '#include "radius_search.h"' in driver and "radius_search<" in api and "radius_search<" in search
    assert "knn_go_brute(" not in api and "knn_go_brute(" not in search
    sources = [_read("tests", f) for f in sorted(os.listdir(os.path.join(ROOT, "tests"))) if f.endswith((".cpp", ".h"))]
    assert sum(s.count("struct Grid {") for s in sources) == 1 and sum(s.count("Grid build_grid(") for s in sources) == 1  # grid_replay.h


# ---- 2. the driver ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nearest") / "nearest_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "nearest_driver.cpp"), "-o", exe])
    return exe


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def _fx(x):
    return f"{int(np.array([x], F).view(np.uint32)[0]):x}"


def _hex(a):
    return " ".join(f"{w:x}" for w in np.ascontiguousarray(a, F).reshape(-1).view(np.uint32))


def _floats(ws):
    return np.array([int(w, 16) for w in ws], np.uint32).view(F)


def _same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def _search(driver, q, t, xform=IDENTITY, max_distance=0.0, hint=0.0, grid_bits=0, max_rounds=0):
    """(queries, targets, rounds, n_brute, first_radius, cells seen, index, d2) of the driver's search, checked against its own O(n m)
    loop and against the numpy restatement, bit for bit"""
    q, t = np.ascontiguousarray(q, F).reshape(-1, 3), np.ascontiguousarray(t, F).reshape(-1, 3)
    text = f"search {_fx(max_distance)} {_fx(hint)} {grid_bits:x} {max_rounds:x} {q.shape[0]:x} {_hex(xform)} {_hex(q)} {_hex(t)}\n"
    head, index, d2 = _play(driver, text)
    assert head[0] == "search" and head[6:8] == ["0", "0"], head  # indices / d2 that differ from the driver's definition
    index, d2 = np.array([int(w, 16) for w in index[1:]], np.uint32), _floats(d2[1:])
    mapped, part, _ = R.query_participates(xform, q)
    want_index, want_d2 = R.brute(mapped, part, t, N.participates(t), max_distance)
    assert np.array_equal(index, want_index) and _same(d2, want_d2)
    assert int(head[1]) == part.sum() and int(head[2]) == N.participates(t).sum()
    return int(head[1]), int(head[2]), int(head[3]), int(head[4]), _floats([head[5]])[0], int(head[8]), index, d2


def _uniform(n, seed=0):
    return np.random.default_rng(seed).random((n, 3)).astype(F)


def test_the_signed_cell(driver):
    inv_h = F(4.0)
    cases = [(0.0, 0.0, 0), (0.24, 0.0, 0), (0.25, 0.0, 1), (-0.01, 0.0, -1), (-0.25, 0.0, -1), (-0.26, 0.0, -2), (-1e30, 0.0, -2), (-3e38, 3e38, -2),
             (1e30, 0.0, 32767), (8191.75, 0.0, 32767), (8191.7, 0.0, 32766), (3e38, -3e38, 32767), (5.0, 5.0, 0), (4.9, 5.0, -1)]
    out = _play(driver, "".join(f"cell {_fx(x)} {_fx(o)} {_fx(inv_h)}\n" for x, o, _ in cases))
    assert [int(ln[1]) for ln in out] == [c[2] for c in cases]
    # at or above the origin it is section 18's cell
    xs = np.random.default_rng(1).random(200).astype(F) * F(9000)
    out = _play(driver, "".join(f"cell {_fx(x)} {_fx(0.5)} {_fx(inv_h)}\n" for x in xs))
    above = xs >= F(0.5)
    assert np.array_equal(np.array([int(ln[1]) for ln in out])[above], N.cells(xs[above], F(0.5), inv_h))


def test_queries_inside_straddling_below_and_far_above_the_box(driver):
    """the cells -2, -1, 0 and the clamp all occur, on every axis, and no answer differs from the definition"""
    t = _uniform(3000, 2)
    inside = _uniform(1500, 3)
    seen = 0
    for axis in range(3):
        shift = np.zeros(3, F)
        for offset in (-0.5, 0.5, -0.02, -30.0, 1e9):  # straddling below and above, just below, far below, far above (the clamp)
            shift[axis] = offset
            P, T, rounds, n_brute, _, cells, index, d2 = _search(driver, inside + shift, t)
            seen |= cells
            assert (index != R.NONE).all()  # unlimited: every query has an answer
        shift[axis] = -30.0
        P, T, rounds, n_brute, _, cells, index, d2 = _search(driver, np.concatenate([inside, inside + shift]), t, max_distance=0.05)
        assert cells & 1 and n_brute == 0 and (index[1500:] == R.NONE).all() and (index[:1500] != R.NONE).sum() > 1000
    assert seen == 15
    P, T, rounds, n_brute, _, cells, index, d2 = _search(driver, inside, t)
    assert rounds >= 1 and cells & 4


def test_no_knob_changes_an_answer(driver):
    t, q = _uniform(2500, 4), _uniform(1300, 5) * F(1.2) - F(0.1)
    base = _search(driver, q, t)
    d = float(np.sqrt(np.median(base[7])))
    seen = set()
    for hint, grid_bits, max_rounds in ((0.0, 0, 0), (d * 1e-6, 0, 1), (d * 1e-6, 0, 2), (d * 1e-6, 0, 0), (d * 1e6, 0, 0), (d, 0, 0), (d * 3, 3, 0),
                                        (d * 0.5, 12, 2), (0.0, 1, 0)):
        got = _search(driver, q, t, hint=hint, grid_bits=grid_bits, max_rounds=max_rounds)
        assert np.array_equal(got[6], base[6]) and _same(got[7], base[7]), (hint, grid_bits, max_rounds)
        seen.add((got[2], got[3]))
    assert len(seen) >= 3  # the paths differ; the answers do not


def test_engineered_sets(driver):
    lat = N.lattice()  # spacing 0.25: the cell centres are at exactly the same distance from 8 lattice points
    centres = (lat + F(0.125))[:200]
    P, T, rounds, n_brute, _, _, index, d2 = _search(driver, centres, lat)
    full = R._d2(centres, lat)
    assert ((full == d2[:, None]).sum(axis=1) >= 2).any()  # exact ties exist ...
    assert np.array_equal(index, full.argmin(axis=1))       # ... and the smallest index wins
    _, _, _, _, _, _, index, d2 = _search(driver, np.tile(lat[:50], (2, 1)), np.tile(lat, (2, 1)), hint=1e-3)
    assert not d2.any() and np.array_equal(index, np.tile(np.arange(50), 2))  # coincident points: distance 0, the first copy
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    _, _, _, _, _, _, index, d2 = _search(driver, same, same)
    assert not d2.any() and not index.any()
    one = F([[0.5, 0.5, 0.5]])
    P, T, rounds, n_brute, _, _, index, d2 = _search(driver, _uniform(1500, 6), one)  # one target: a box that is a point
    assert T == 1 and not index.any()
    far = _uniform(1100, 8)
    far[3], far[4] = [3e38, 0, 0], [-3e38, -3e38, 3e38]  # differences overflow: +inf, out of reach also without a max_distance
    P, T, rounds, n_brute, _, _, index, d2 = _search(driver, far, _uniform(900, 9))
    assert index[3] == R.NONE and index[4] == R.NONE and np.isinf(d2[[3, 4]]).all() and (index[5:] != R.NONE).all() and not np.isnan(d2).any()
    t = _uniform(2000, 10)
    t[7] = [np.nan, 0, 0]
    q = _uniform(1200, 11)
    q[5] = [0, np.inf, 0]
    P, T, _, _, _, _, index, d2 = _search(driver, q, t)
    assert (P, T) == (1199, 1999) and index[5] == R.NONE and (index != 7).all()


def test_small_sets_go_straight_to_the_fallback(driver):
    for n, m in ((1, 1), (1, 5000), (63, 2), (1024, 1025), (1025, 1024)):
        P, T, rounds, n_brute, _, _, _, _ = _search(driver, _uniform(n, n), _uniform(m, m + 1))
        assert (rounds, n_brute) == (0, n) if n <= 1024 else rounds >= 1


def test_max_distance_includes_its_own_distance_and_excludes_the_float_below(driver):
    t = np.concatenate([_uniform(1500, 12), F([[5.0, 5.0, 5.0]])])
    q = np.concatenate([_uniform(1200, 13), F([[5.0, 5.0, 5.75]])])  # the last pair is 0.75 apart, exactly: d2 = 0.5625
    for hint in (0.0, 0.01, 3.0):
        _, _, _, n_brute, _, _, index, d2 = _search(driver, q, t, max_distance=0.75, hint=hint)
        assert index[-1] == 1500 and d2[-1] == F(0.5625)
        _, _, _, n_brute, _, _, index, d2 = _search(driver, q, t, max_distance=np.nextafter(F(0.75), F(0)), hint=hint)
        assert index[-1] == R.NONE and np.isinf(d2[-1])
    # the rule of the round radius: exactly max_distance once the radius would pass it, unless the floor forbids it
    P, T, rounds, n_brute, first, _, index, d2 = _search(driver, q, t, max_distance=0.002, hint=0.5)
    assert first == F(0.002) and rounds == 1 and n_brute == 0
    P, T, rounds, n_brute, first, _, index, d2 = _search(driver, q, t, max_distance=1e-7, hint=0.5)  # below the floor of a box 5 wide
    assert first == F(0.5) and rounds == 1 and n_brute == 0 and (index == R.NONE).all()


def test_the_mapping_and_the_matrix_of_two_model_transforms(driver):
    rng = np.random.default_rng(14)
    src = (rng.normal(size=3), rng.normal(size=4), [1.5, 0.5, 2.0])
    dst = (rng.normal(size=3), rng.normal(size=4) * 3, [0.25, 3.0, 1.0])
    line = "matrix " + " ".join(_hex(a) for a in (*src, *dst)) + "\n"
    got = _floats(_play(driver, line)[0][1:]).reshape(3, 4)
    want = R.model_matrix(src, dst)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 2 * ulp).all()
    t, q = _uniform(2000, 15), rng.normal(size=(1200, 3)).astype(F)
    base = _search(driver, q, t, xform=got)
    assert (base[6] != R.NONE).all()
    big = np.array(got)
    big[1, 1] = F(3e38)  # q overflows to inf for |y| above about 1.13: those queries do not participate
    P, _, _, _, _, _, index, _ = _search(driver, q, t, xform=big)
    assert 0 < P < 1200 and (index[np.abs(q[:, 1]) > 2] == R.NONE).all()


# ---- 3. csrc/align_math.h against numpy's SVD ------------------------------------------------------------------------------------------
ALIGN_TOL = 1.2e-13  # the largest deviation measured over the cases below, 1.11e-15 (the 4-point cloud with a scale), times 100, rounded up


def _similarity(rng, scale=1.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0.2, 2.5)
    quat = np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])
    return R.quat_rows(quat), scale, rng.normal(size=3)


def _align(driver, q, t, with_scale):
    ln = _play(driver, f"align {int(with_scale):x} {q.shape[0]:x} {_hex(q)} {_hex(t)}\n")[0]
    v = [float(x) for x in ln[2:]]
    return int(ln[1]), np.array(v[0:4]), v[4], np.array(v[5:8])


def test_the_solve_equals_numpys_svd(driver):
    """Horn's quaternion by Jacobi against Kabsch / Umeyama by numpy's float64 SVD on the same sums.  The largest deviation of a
    rotation entry, the scale or a translation component (relative to the cloud's size) over all cases, measured: 1.11e-15; the bound
    is that times 100, rounded up to 1.2e-13, far inside the 1e-9 past which the solver would be wrong."""
    rng = np.random.default_rng(16)
    worst = 0.0
    for n, with_scale, planar in ((3, False, False), (4, False, False), (100, False, False), (3, True, False), (4, True, False), (100, True, False),
                                  (100, False, True), (100, True, True)):
        q = rng.normal(size=(n, 3))
        if planar:
            q[:, 2] = 0.0
        q = q.astype(F)
        Rm, s, p = _similarity(rng, 1.7 if with_scale else 1.0)
        t = (s * (q.astype(np.float64) @ Rm.T) + p + rng.normal(size=(n, 3)) * 1e-3).astype(F)
        degenerate, quat, scale, pos = _align(driver, q, t, with_scale)
        want = R.align_solve(R.align_sums(q, t), with_scale)
        assert not degenerate and quat[3] >= 0 and abs(np.linalg.norm(quat) - 1) < 1e-15
        dev = max(np.abs(R.quat_rows(quat) - want["R"]).max(), abs(scale - want["scale"]), np.abs(pos - want["pos"]).max() / (1 + np.abs(p).max()))
        print(f"n {n} scale {with_scale} planar {planar}: deviation {dev:.3g}")
        worst = max(worst, dev)
        assert np.abs(R.quat_rows(quat) - Rm).max() < 5e-3 and abs(scale - s) < 5e-3  # and it is the similarity the cloud went through
    print(f"largest deviation {worst:.3g}")
    assert worst <= ALIGN_TOL


def test_degenerate_pairs_are_flagged_and_give_the_identity(driver):
    rng = np.random.default_rng(17)
    line = (np.linspace(-1, 1, 50)[:, None] * np.array([[1.0, 2.0, -0.5]])).astype(F)  # collinear: no single best rotation
    Rm, s, p = _similarity(rng)
    for q in (line, rng.normal(size=(2, 3)).astype(F), np.tile(F([[0.3, 0.1, 0.2]]), (40, 1))):  # ... two pairs, no spread
        t = ((q.astype(np.float64) @ Rm.T) + p).astype(F)
        degenerate, quat, scale, pos = _align(driver, q, t, True)
        assert degenerate == 1 and np.array_equal(quat, [0, 0, 0, 1]) and scale == 1.0 and not pos.any()


def test_the_composition_is_taken_in_double_and_rounded_once(driver):
    rng = np.random.default_rng(18)
    for _ in range(20):
        Rm, s, p = _similarity(rng, rng.uniform(0.5, 2))
        delta = dict(quat=R.rows_quat(Rm).astype(F), scale=F(s), pos=p.astype(F))
        xform = rng.normal(size=(3, 4)).astype(F)
        got = _floats(_play(driver, f"compose {_hex(delta['quat'])} {_fx(delta['scale'])} {_hex(delta['pos'])} {_hex(xform)}\n")[0][1:]).reshape(3, 4)
        want = R.compose({k: np.asarray(v, np.float64) for k, v in delta.items()}, xform)
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()  # (the sums' order: one ulp at most)


# ---- 4. the restatement: what the GPU tests expect of it --------------------------------------------------------------------------------
def test_the_restatement_statistics_and_hits(driver):
    """on the driver's answer (which _search has compared with the restatement's, bit for bit)"""
    t, q = _uniform(800, 19), _uniform(500, 20) * F(2)
    mapped, part, nonfinite = R.query_participates(IDENTITY, q)
    index, d2 = _search(driver, q, t, max_distance=0.2)[6:]
    found = index != R.NONE
    assert 0 < found.sum() < 500 and (np.sqrt(d2[found]) <= F(0.2)).all()
    st = R.stats(index, d2)
    d = np.sqrt(d2[found]).astype(np.float64)
    assert st["n_found"] == found.sum() and st["mean"] == pytest.approx(d.mean(), rel=1e-14) and st["d_max"] == np.sqrt(d2[found]).max()
    assert st["rms"] == pytest.approx(np.sqrt((d2[found].astype(np.float64)).mean()), rel=1e-14)
    assert np.array_equal(R.hit(index, d2, part, R.SELECT_RANGE, 0.0, np.inf), part)
    assert np.array_equal(R.hit(index, d2, part, R.SELECT_RANGE, 0.0, 0.2), found)
    sel = np.zeros(800, bool)
    sel[::3] = True
    assert np.array_equal(R.hit(index, d2, part, R.SELECT_TRANSFER, dst_selected=sel), found & sel[np.where(found, index, 0)])
    assert not R.hit(index, d2, part, R.SELECT_TRANSFER, dst_selected=None).any()
    assert R.stats(np.full(4, R.NONE, np.uint32), np.full(4, np.inf, F)) == dict(n_found=0, d_min=0, d_max=0, mean=0.0, rms=0.0)
