"""Model normals (gsx_model_normals, gsx_model_select_normals; spec §26) without a device: the entry points and the structs in the
header, the library, the bindings and the facades; the rules of csrc/normals_math.h — played by tests/normals_driver.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process, through a plain C++ version
of the whole search — against an O(n^2) loop and against the numpy restatement tests/normals_ref.py, whose eigen-solve is
numpy.linalg.eigh; and the restatement's expectations the GPU tests rely on.

The bounds.  The neighbour lists are integers: equal exactly.  The fit is a fixed five-sweep cyclic Jacobi solve in double; against
eigh, a numpy restatement of it on k = 3, 8, 16 neighbourhoods of the three families below (uniform cube, noisy sheet, a 1 cm cloud at
offset 1000) differed by at most 3.1e-16 in the variation and 6.7e-14 in a normal's component, and the float32-rounded normals were
equal but for 3.3e-16 in a near-zero component; four sweeps gave the figures of eight.  Hence: the variation within 1 float32 unit in
the last place of the reference's (the double error is 2^-29 of one; only a rounding boundary can show), every component of a normal
within 2^-23 (one unit in the last place of a component near 1, the largest any has).  A normal is only defined where the two
smallest eigenvalues differ: it is compared on the certain Gaussians, (l1 - l2) / l0 >= 1e-6.
Two kinds of rows the reference itself cannot decide; both are found from the reference ALONE, counted, and the count is bounded.
(1) Tiny variations.  eigh's eigenvalues carry an absolute error of a few 2^-53 of the trace, so the reference's variation is known to
2^-50 absolutely and no better.  Where the reference's variation is below 2^-26 that error exceeds a float32 ulp of the value: four
float32 points of the far cloud are often exactly coplanar, the true variation is 0, eigh returns 4e-17 and the library 8e-19.  On
those rows, and on no others, the bound is 1 ulp plus 2^-50; everywhere else it is 1 ulp alone.  A fixture may hold at most 1 % of
them.  (2) Unsigned normals.  The canonical sign is decided by the first non-zero component; where the reference's lies within 2^-23
of 0 — inside the normals' own tolerance — two correct solves may round it to either side of 0.  A direction drawn at random has
that chance 2^-23 a row; only the far cloud at k = 3 (four points on a lattice of 160 float32 steps an axis, whose planes are
sometimes exactly parallel to an axis) has any.  There (normals_ref.fit: `signed` is false) the normal is compared up to its sign,
with the same 2^-23; on every other certain row the sign is asserted.  A fixture may hold at most 4 such rows."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import knn_ref as K
from tests import neighbors_ref as N
from tests import normals_ref as R
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCTIONS = ("gsx_normals_desc_default", "gsx_model_normals", "gsx_model_select_normals")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    for name, value in (("GSX_NORMALS_MIN_K", "3"), ("GSX_NORMALS_MAX_K", "16"), ("GSX_NORMALS_ORIENT_CANONICAL", "0"),
                        ("GSX_NORMALS_ORIENT_TOWARD", "1"), ("GSX_NORMALS_SELECT_VARIATION", "0"), ("GSX_NORMALS_SELECT_FACING", "1"),
                        ("GSX_NORMALS_ABS", "1"), ("GSX_NORMALS_NONE", "0xFFFFFFFF")):
        assert re.search(rf"^#define {name} {value}u", hdr, re.M) and getattr(_lib, name) == int(value, 0)
    assert (R.MIN_K, R.MAX_K, R.ORIENT_CANONICAL, R.ORIENT_TOWARD, R.SELECT_VARIATION, R.SELECT_FACING, R.ABS, R.NONE) == (3, 16, 0, 1, 0, 1, 1, 0xFFFFFFFF)
    assert re.search(r"typedef struct gsx_normals_desc \{\s*uint32_t filter; uint32_t flags; uint32_t k; uint32_t orient;[^}]*float radius_hint; "
                     r"uint32_t grid_bits; uint32_t max_rounds; uint32_t reserved;\s*float toward\[3\]; uint32_t reserved2;\s*\} gsx_normals_desc; /\* 48 B \*/", hdr)
    assert re.search(r"typedef struct gsx_normals_stats_t \{\s*uint64_t count; uint64_t n_nonfinite; uint64_t n_fitted; uint64_t n_brute; double mean;\s*"
                     r"float variation_min; float variation_max; float first_radius; uint32_t rounds; uint32_t grid_bits; uint32_t reserved;"
                     r"\s*\} gsx_normals_stats_t; /\* 64 B \*/", hdr)
    assert re.search(r"typedef struct gsx_normals_select_desc \{\s*uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t mode;[^}]*"
                     r"uint32_t k; uint32_t orient; float radius_hint; uint32_t grid_bits;\s*uint32_t max_rounds; float lo; float hi; uint32_t reserved;\s*"
                     r"float dir\[3\]; float toward\[3\]; uint32_t reserved2\[2\];\s*\} gsx_normals_select_desc; /\* 80 B \*/", hdr)
    assert re.search(r"^void gsx_normals_desc_default\(gsx_normals_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_normals\(gsx_viewer\* v, const char\* key, const gsx_normals_desc\* desc, float\* out_normal /\*[^/]*\*/,\s*"
                     r"float\* out_variation /\*[^/]*\*/, uint32_t\* out_index /\*[^/]*\*/,\s*gsx_normals_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_normals\(gsx_viewer\* v, const char\* key, const gsx_normals_select_desc\* desc, uint64_t\* out_hit, "
                     r"uint64_t\* out_selected,\s*gsx_normals_stats_t\* out_stats[^)]*\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    spec = _read("spec", "RENDER_SPEC.md")
    assert "§26" in hdr and "## 26. Model normals [BUILD-SPEC]" in spec
    for word in ("Point-to-plane registration", "normals plane in the depth map", "propagation", "covariance-aware", "Sharded models", "model-session fuzz"):
        assert word in spec.split("## 26. Model normals [BUILD-SPEC]")[1], word  # what §26 leaves out


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.NormalsDesc) == 48
    assert offsets(_lib.NormalsDesc) == {"filter": 0, "flags": 4, "k": 8, "orient": 12, "radius_hint": 16, "grid_bits": 20, "max_rounds": 24,
                                         "reserved": 28, "toward": 32, "reserved2": 44}
    assert C.sizeof(_lib.NormalsStats) == 64
    assert offsets(_lib.NormalsStats) == {"count": 0, "n_nonfinite": 8, "n_fitted": 16, "n_brute": 24, "mean": 32, "variation_min": 40,
                                          "variation_max": 44, "first_radius": 48, "rounds": 52, "grid_bits": 56, "reserved": 60}
    assert C.sizeof(_lib.NormalsSelectDesc) == 80
    assert offsets(_lib.NormalsSelectDesc) == {"filter": 0, "flags": 4, "selection_op": 8, "mode": 12, "k": 16, "orient": 20, "radius_hint": 24,
                                               "grid_bits": 28, "max_rounds": 32, "lo": 36, "hi": 40, "reserved": 44, "dir": 48, "toward": 60,
                                               "reserved2": 72}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_normals.cpp")
    assert "static_assert(sizeof(gsx_normals_desc) == 48 && sizeof(gsx_normals_stats_t) == 64 && sizeof(gsx_normals_select_desc) == 80" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[1:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_normals_desc", "gsx_normals_stats_t", "gsx_normals_select_desc"):
        assert "pub struct " + s + " " in rust_sys and s in _read("tools", "gen_rust_sys.py")
    assert "pub const GSX_NORMALS_MAX_K: u32 = 16;" in rust_sys and "pub const GSX_NORMALS_NONE: u32 = 0xFFFF_FFFF;" in rust_sys
    for method in ("normals", "select_normals"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.NormalsDesc(7, 7, 7, 7, 7.0, 7, 7, 7, (C.c_float * 3)(7, 7, 7), 7)
    L.gsx_normals_desc_default(C.byref(d))
    assert (d.filter, d.flags, d.k, d.orient, d.radius_hint, d.grid_bits, d.max_rounds, d.reserved, tuple(d.toward), d.reserved2) == \
        (0, 0, 8, _lib.GSX_NORMALS_ORIENT_CANONICAL, 0.0, 0, 0, 0, (0.0, 0.0, 0.0), 0)
    L.gsx_normals_desc_default(None)
    # without a device: a status code and a message, not a crash
    normal, variation, index, stats = (C.c_float * 12)(), (C.c_float * 4)(), (C.c_uint32 * 32)(), _lib.NormalsStats()
    assert L.gsx_model_normals(None, b"a", C.byref(d), normal, variation, index, C.byref(stats)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_normals" in L.gsx_last_error_string()
    sd = _lib.NormalsSelectDesc(0, 0, 0, _lib.GSX_NORMALS_SELECT_VARIATION, 8, 0, 0.0, 0, 0, 0.0, 0.1, 0)
    assert L.gsx_model_select_normals(None, b"a", C.byref(sd), None, None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_normals" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("normals", "select_normals"))


def test_the_rules_have_one_copy_and_the_build_lists_the_sources():
    kernels, api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_normals.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_normals.cpp")
    math_h, driver = _read("wgpu_3dgs_viewer_app_amd", "csrc", "normals_math.h"), _read("tests", "normals_driver.cpp")
    rules = ("inline void nm_offer(", "inline bool nm_list_proven(", "inline bool nm_list_fitted(", "inline NormalFit nm_plane_fit(",
             "inline bool nm_flip(", "inline bool nm_select_hit(", "inline bool nm_direction(", "inline uint64_t nm_key(")
    for text in (kernels, api, driver):
        assert '#include "normals_math.h"' in text
        for rule in rules + ("inline float nb_d2(", "inline void ex_rotate(", "inline void ex_sort_pair(", "inline bool knn_go_brute("):
            assert rule not in text
    for rule in rules:
        assert math_h.count(rule) == 1, rule
    # the distance is section 18's, the rotation and the sort section 14's, called, not copied; the solve is in double
    assert '#include "neighbors_math.h"' in math_h and '#include "export_math.h"' in math_h
    assert "inline float nb_d2(" not in math_h and "ex_rotate<double, 0, 1>" in math_h and "ex_sort_pair<double, 0, 1>" in math_h and "kExportSweeps" in math_h
    csrc = [_read("wgpu_3dgs_viewer_app_amd", "csrc", f) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".cpp"))]
    assert sum(s.count("inline float nb_d2(") for s in csrc) == 1 and sum(s.count("inline void ex_rotate(") for s in csrc) == 1
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_normals.hip" in makefile and "gsx_api_normals.cpp" in makefile and "-ffp-contract=off" in makefile
    # the loop over the rounds is radius_search.h's: the library and the driver run it, and neither decides the fallback itself
    search = driver.split("static void search(")[1].split("\n}\n")[0]
    assert '#include "radius_search.h"' in api and '#include "radius_search.h"' in driver and "radius_search<" in api and "radius_search<" in search
    assert "knn_go_brute(" not in api and "knn_go_brute(" not in search and "knn_next_radius(" not in api
    assert '#include "grid_replay.h"' in driver and "struct Grid {" not in driver


# ---- 2. csrc/normals_math.h: the driver -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("normals") / "normals_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "normals_driver.cpp"), "-o", exe])
    return exe


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def _fx(x):
    return f"{int(np.array([x], F).view(np.uint32)[0]):x}"


def _words(ws):
    return np.array([int(w, 16) for w in ws], np.uint32)


def search(driver, pos, k, toward=None, hint=0.0, grid_bits=0, max_rounds=0, command="search") -> dict:
    """the driver's search; its own O(n^2) check must hold (command "replay": the search without that check)"""
    pos = np.ascontiguousarray(pos, F)
    orient, t = (R.ORIENT_CANONICAL, (0.0, 0.0, 0.0)) if toward is None else (R.ORIENT_TOWARD, toward)
    text = (f"{command} {k:x} {orient:x} {_fx(t[0])} {_fx(t[1])} {_fx(t[2])} {_fx(hint)} {grid_bits:x} {max_rounds:x} "
            f"{' '.join(f'{w:x}' for w in pos.reshape(-1).view(np.uint32))}\n")
    head, index, normal, variation, stats = _play(driver, text)
    assert head[0] == "search" and head[5:] == ["0", "0"], head  # lists / fits that differ from the driver's definition
    n = pos.shape[0]
    st = _words(stats[1:])
    return dict(participants=int(head[1]), rounds=int(head[2]), n_brute=int(head[3]), first_radius=_words([head[4]]).view(F)[0],
                index=_words(index[1:]).reshape(n, k), normal=_words(normal[1:]).view(F).reshape(n, 3), variation=_words(variation[1:]).view(F),
                n_fitted=int(st[0]), variation_min=st[1:2].view(F)[0], variation_max=st[2:3].view(F)[0],
                mean=float(np.array([int(st[3]) | (int(st[4]) << 32)], np.uint64).view(np.float64)[0]))


def ulps(a, b) -> np.ndarray:
    """the distance in float32 units in the last place between finite non-negative a and b; equal infinities are 0 apart"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_fit(got_normal, got_variation, want, what="", tiny_rows=None):
    """got against normals_ref.fit: the same Gaussians fitted, the variation within 1 ulp, the certain normals within 2^-23 a component;
    the two counted exceptions of this file's docstring.  tiny_rows: bool[n], the only rows that may have a tiny reference variation"""
    fitted = want["fitted"]
    assert np.array_equal(np.isfinite(got_variation), fitted), what
    assert np.isinf(got_variation[~fitted]).all() and not got_normal[~fitted].any(), what
    ref = want["variation"][fitted]
    tiny = ref < R.TINY_VARIATION  # (the reference alone: its own error exceeds an ulp there)
    if tiny_rows is None:
        assert tiny.sum() <= 0.01 * fitted.size, what
    else:  # an engineered fixture names the rows whose true variation is 0
        assert not (tiny & ~np.asarray(tiny_rows, bool)[fitted]).any(), what
    bound = np.spacing(ref).astype(np.float64) + np.where(tiny, R.REF_VARIATION_ERROR, 0.0)
    assert (np.abs(got_variation[fitted].astype(np.float64) - ref.astype(np.float64)) <= bound).all(), what
    certain = fitted & (want["gap"] >= R.CERTAIN)
    signed = want["signed"][certain]
    assert (~signed).sum() <= R.UNSIGNED_MAX, what
    g, w = got_normal[certain].astype(np.float64), want["normal"][certain].astype(np.float64)
    worst = np.abs(g - w).max(axis=1, initial=0.0)
    assert worst[signed].max(initial=0.0) <= R.NORMAL_ATOL, what  # the sign too
    assert np.minimum(worst, np.abs(g + w).max(axis=1, initial=0.0))[~signed].max(initial=0.0) <= R.NORMAL_ATOL, what  # up to the sign
    length = np.sqrt((got_normal[fitted].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max(initial=0.0) <= 2e-7, what
    return certain


@pytest.mark.parametrize("family", [f[0] for f in R.FAMILIES])
@pytest.mark.parametrize("k", [3, 8, 16])
def test_the_search_and_the_fit_equal_the_restatement_on_the_three_families(driver, family, k):
    pos = dict(R.FAMILIES)[family](1500, k)
    pos[7] = [np.nan, 0, 0]
    part = N.participates(pos)
    index, d2 = R.lists(pos, part, k)
    assert np.array_equal(d2.view(np.uint32), K.brute(pos, part, k).view(np.uint32))  # the list's d2 are the nearest neighbours' rows
    want = R.fit(pos, index, d2)
    assert (want["fitted"] & ((want["gap"] < R.CERTAIN) | ~want["signed"])).sum() <= 0.01 * 1500  # the reference alone: few are uncertain
    got = search(driver, pos, k)
    assert got["participants"] == 1499 and got["rounds"] >= 1
    assert np.array_equal(got["index"], index)
    check_fit(got["normal"], got["variation"], want, (family, k))
    assert (got["index"][7] == R.NONE).all() and np.isinf(got["variation"][7]) and not got["normal"][7].any()
    assert ((got["variation"][part] >= 0) & (got["variation"][part] <= F(1.0 / 3.0) + F(1e-7))).all()
    st = R.stats(got["variation"])
    assert (got["n_fitted"], got["variation_min"], got["variation_max"]) == (st["n_fitted"], st["variation_min"], st["variation_max"])
    assert got["mean"] == pytest.approx(st["mean"], rel=2e-12, abs=0)
    if family == "sheet" and k >= 8:  # (four points are always close to some plane: k = 3 tells a sheet from a cube poorly)
        assert np.median(got["variation"][part]) < 0.01 < 0.05 < np.median(search(driver, R.uniform_cube(1500, 4), k)["variation"])


def test_no_knob_changes_a_word(driver):
    pos = R.noisy_sheet(1400, 5)
    part = N.participates(pos)
    d = K.kth_distance_median(pos, part)
    base = search(driver, pos, 5)
    seen = set()
    for hint, grid_bits, max_rounds in ((d * 1e-6, 0, 1), (d * 1e-6, 0, 0), (d * 1e6, 0, 0), (d, 0, 0), (d * 3, 3, 0), (d * 0.5, 12, 2), (0.0, 1, 0)):
        got = search(driver, pos, 5, hint=hint, grid_bits=grid_bits, max_rounds=max_rounds)
        for name in ("index", "normal", "variation"):
            assert got[name].tobytes() == base[name].tobytes(), (name, hint, grid_bits, max_rounds)
        assert (got["n_fitted"], got["mean"]) == (base["n_fitted"], base["mean"])
        seen.add((got["rounds"], got["n_brute"]))
    assert len(seen) >= 3  # the paths differ; the words do not


def test_lattice_with_ties_at_the_kth_distance(driver):
    lat = N.lattice(0.25, 11)  # 1331 points: the grid rounds answer
    every = np.ones(lat.shape[0], bool)
    interior = (np.abs(np.rint(lat / F(0.25))) < 5).all(axis=1)
    for k in (5, 6, 7):  # six neighbours at exactly 0.25: at k = 5 the index decides who is left out
        index, d2 = R.lists(lat, every, k)
        got = search(driver, lat, k)
        assert np.array_equal(got["index"], index)
        assert (d2[interior, :min(k, 6)] == F(0.0625)).all()
        assert (np.diff(index[interior, :min(k, 6)].astype(np.int64), axis=1) > 0).all()  # equal distances: ascending indices
        for bits in (1, 3):
            assert np.array_equal(search(driver, lat, k, grid_bits=bits)["index"], index)
    got = search(driver, lat, 6)
    assert (ulps(got["variation"][interior], np.full(int(interior.sum()), 1.0 / 3.0, F)) <= 1).all()  # isotropic: 1/3 (normals not compared)
    assert got["n_fitted"] == lat.shape[0]


def at_most_three_points(pos, index) -> np.ndarray:
    """bool[n]: the Gaussian and its k listed neighbours are at most three distinct points (coincident groups): they lie in a plane,
    the scatter has rank 2 at the most and the true variation is 0"""
    p = np.concatenate([pos[:, None, :], pos[np.where(index == R.NONE, 0, index).astype(np.int64)]], axis=1)
    distinct = np.array([np.unique(row, axis=0).shape[0] for row in p])
    return (index != R.NONE).all(axis=1) & (distinct <= 3)


def test_partially_coincident_points(driver):
    rng = np.random.default_rng(6)
    groups = np.concatenate([np.tile(rng.random((40, 1, 3)), (1, 3, 1)).reshape(-1, 3),   # groups of 3: smaller than k
                             np.tile(rng.random((4, 1, 3)), (1, 40, 1)).reshape(-1, 3),   # groups of 40: larger than k
                             rng.random((1200, 3))]).astype(F)
    every = np.ones(groups.shape[0], bool)
    index, d2 = R.lists(groups, every, 8)
    got = search(driver, groups, 8)
    assert np.array_equal(got["index"], index)
    assert (d2[120:280] == 0).all() and not R.fitted_rows(d2)[120:280].any()  # all 8 coincide with the Gaussian: not fitted
    assert np.isinf(got["variation"][120:280]).all() and not got["normal"][120:280].any()
    assert (got["index"][120:280] != R.NONE).all()  # the list exists, the plane does not
    # among coincident points the smaller indices come first, whichever lane or cell saw them
    assert (np.diff(got["index"][120:280].astype(np.int64), axis=1) > 0).all()
    assert np.isfinite(got["variation"][:120]).all()  # two coincident and six others: fitted
    check_fit(got["normal"], got["variation"], R.fit(groups, index, d2), "groups", tiny_rows=at_most_three_points(groups, index))


def test_the_plane_z_0(driver):
    rng = np.random.default_rng(8)
    pos = np.concatenate([rng.random((1300, 2)) * 4 - 2, np.zeros((1300, 1))], axis=1).astype(F)
    for k in (3, 8, 16):
        got = search(driver, pos, k)
        assert got["n_fitted"] == 1300
        assert (got["normal"] == F([0, 0, 1])).all() and not got["variation"].any()  # exactly
        assert (got["normal"].view(np.uint32)[:, :2] == 0).all()  # +0, not -0
    below = search(driver, pos, 8, toward=(0.0, 0.0, -5.0))
    assert (below["normal"] == F([0, 0, -1])).all() and (below["normal"].view(np.uint32)[:, :2] == 0).all()
    inside = search(driver, pos, 8, toward=(0.5, 0.5, 0.0))  # in the plane: the dot product is exactly 0, the canonical rule decides
    assert (inside["normal"] == F([0, 0, 1])).all()


def test_a_sphere_oriented_toward_its_centre_and_toward_a_far_point(driver):
    rng = np.random.default_rng(9)
    v = rng.normal(size=(1500, 3))
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    pos = (radial * 2.0 + [1.0, -2.0, 0.5]).astype(F)
    centre, far = (1.0, -2.0, 0.5), (1000.0, 0.0, 0.0)
    inward = search(driver, pos, 8, toward=centre)
    dots = (inward["normal"].astype(np.float64) * radial).sum(axis=1)
    assert inward["n_fitted"] == 1500 and (dots < -0.9).all()  # the normal is the radial direction, pointing in
    toward_far = search(driver, pos, 8, toward=far)
    side = ((np.asarray(far) - pos.astype(np.float64)) * toward_far["normal"]).sum(axis=1)
    assert (side > 0).all()
    assert np.array_equal(np.abs(toward_far["normal"]), np.abs(inward["normal"])) and toward_far["variation"].tobytes() == inward["variation"].tobytes()
    canonical = search(driver, pos, 8)
    assert not R.canonical_flip(canonical["normal"]).any() and np.array_equal(np.abs(canonical["normal"]), np.abs(inward["normal"]))
    index, d2 = R.lists(pos, np.ones(1500, bool), 8)
    check_fit(inward["normal"], inward["variation"], R.fit(pos, index, d2, R.ORIENT_TOWARD, centre), "sphere")


def test_coincident_points_and_sets_smaller_than_k_plus_one_are_not_fitted(driver):
    same = np.tile(F([0.3, -1.7, 2.9]), (1300, 1))
    for n in (300, 1300):  # through the exact fallback, and through a grid round
        got = search(driver, same[:n], 16)
        assert got["n_fitted"] == 0 and np.isinf(got["variation"]).all() and not got["normal"].any()
        want = np.tile(np.arange(16, dtype=np.uint32), (n, 1))
        want[:16] += np.triu(np.ones((16, 16), np.uint32))  # (i's own index is skipped)
        assert np.array_equal(got["index"], want)  # no early exit: the sixteen smallest indices, not the first sixteen seen
        assert (got["mean"], got["variation_min"], got["variation_max"]) == (0.0, 0.0, 0.0)
    for n, k in ((1, 3), (3, 3), (4, 4), (10, 16)):
        pos = R.uniform_cube(n, n)
        got = search(driver, pos, k)
        index, d2 = R.lists(pos, np.ones(n, bool), k)
        assert np.array_equal(got["index"], index) and (got["index"][:, n - 1:] == R.NONE).all() and (got["index"][:, :n - 1] != R.NONE).all()
        assert got["n_fitted"] == 0 and np.isinf(got["variation"]).all() and not got["normal"].any()
    four = search(driver, R.uniform_cube(4, 1), 3)  # k + 1 points: fitted
    assert four["n_fitted"] == 4
    far = R.uniform_cube(1100, 8)
    far[3], far[4], far[5] = [3e38, 0, 0], [-3e38, -3e38, 3e38], [3e38, 3e38, 3e38]  # differences overflow: d2 = +inf, the index NONE
    got = search(driver, far, 3)
    index, d2 = R.lists(far, np.ones(1100, bool), 3)
    assert np.array_equal(got["index"], index) and (got["index"][4] == R.NONE).all() and np.isinf(got["variation"][3:6]).all()
    assert not np.isnan(got["normal"]).any() and not np.isnan(got["variation"]).any()


@pytest.mark.parametrize("width", [4, 8, 16])
def test_the_chain_keeps_the_smallest_keys(driver, width):
    rng = np.random.default_rng(width)
    text, want = "", []
    for k in range(1, width + 1):
        for count in (0, 1, k - 1, k, k + 1, 200):
            d2 = (rng.integers(0, 6, count).astype(F) * F(0.25)).view(np.uint32).astype(np.uint64)  # many ties, zeros among them
            keys = (d2 << np.uint64(32)) | rng.permutation(1000)[:count].astype(np.uint64)          # (unique indices; 0 may be among them)
            text += f"chain {width:x} {k:x} {' '.join(f'{int(x) >> 32:x} {int(x) & 0xFFFFFFFF:x}' for x in keys)}\n"
            want.append(np.concatenate([np.sort(keys), np.full(k, (0x7F800000 << 32) | 0xFFFFFFFF, np.uint64)])[:k])
    for ln, w in zip(_play(driver, text), want):
        got = _words(ln[1:]).astype(np.uint64)
        assert ln[0] == "chain" and np.array_equal((got[0::2] << np.uint64(32)) | got[1::2], w)


def test_the_select_tests_equal_the_restatement(driver):
    rng = np.random.default_rng(12)
    v = rng.normal(size=(400, 3))
    normal = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    variation = (rng.random(400) / 3).astype(F)
    variation[::9], normal[::9] = np.inf, 0
    rows = " ".join(f"{a:x}" for a in np.concatenate([normal.view(np.uint32), variation.view(np.uint32)[:, None]], axis=1).reshape(-1))
    for mode, flags, lo, hi, d in ((R.SELECT_VARIATION, 0, 0.0, 0.1, (0, 0, 0)), (R.SELECT_VARIATION, 0, 0.2, np.inf, (0, 0, 0)),
                                   (R.SELECT_FACING, 0, 0.5, 1.0, (0, 0, 3)), (R.SELECT_FACING, R.ABS, 0.5, 1.0, (1, -2, 0.5)),
                                   (R.SELECT_FACING, 0, -1.0, -0.2, (1e-30, 2e-30, 0)), (R.SELECT_FACING, R.ABS, 0.0, 0.0, (3e38, 3e38, 3e38))):
        hits, direction = _play(driver, f"hit {mode:x} {flags:x} {_fx(lo)} {_fx(hi)} {_fx(d[0])} {_fx(d[1])} {_fx(d[2])} {rows}\n")
        want = R.hit(normal, variation, mode, lo, hi, d if mode == R.SELECT_FACING else None, flags)
        assert np.array_equal(np.array(hits[1:], int).astype(bool), want), (mode, flags, lo, hi, d)
        assert not want[::9].any()
        if mode == R.SELECT_FACING:
            assert direction[1] == "1" and np.array_equal(_words(direction[2:]).view(F), R.direction(d))
    for bad in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0)):
        assert _play(driver, f"hit 1 0 0 0 {_fx(bad[0])} {_fx(bad[1])} {_fx(bad[2])}\n")[1][1] == "0"
