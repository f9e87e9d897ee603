"""Model nearest neighbours (gsx_model_knn, gsx_model_select_knn; spec §20) without a device: the entry points and the structs in the
header, the library, the bindings and the facades; the rules of csrc/knn_math.h — played by tests/knn_driver.cpp, a stand-alone
program built with the address and undefined-behaviour sanitizers and run as a child process, through a plain C++ version of the
whole search — against an O(n^2) loop and against the numpy restatement tests/knn_ref.py; and the restatement's expectations the
GPU tests rely on (lattice, coincident points, scores, statistics, outliers)."""
from __future__ import annotations

import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import knn_ref as K
from tests import neighbors_ref as N
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCTIONS = ("gsx_knn_desc_default", "gsx_model_knn", "gsx_model_select_knn")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    for name, value in (("GSX_KNN_MAX_K", 16), ("GSX_KNN_SCORE_KTH", 0), ("GSX_KNN_SCORE_MEAN", 1), ("GSX_KNN_SELECT_RANGE", 0),
                        ("GSX_KNN_SELECT_OUTLIERS", 1)):
        assert re.search(rf"^#define {name} {value}u", hdr, re.M) and getattr(_lib, name) == value
    assert (K.MAX_K, K.SCORE_KTH, K.SCORE_MEAN, K.SELECT_RANGE, K.SELECT_OUTLIERS) == (16, 0, 1, 0, 1)
    assert re.search(r"typedef struct gsx_knn_desc \{ uint32_t filter; uint32_t flags; uint32_t k; uint32_t score; float radius_hint; "
                     r"uint32_t grid_bits; uint32_t max_rounds; uint32_t reserved; \} gsx_knn_desc;", hdr)
    assert re.search(r"typedef struct gsx_knn_stats_t \{\s*uint64_t count; uint64_t n_nonfinite; uint64_t n_scored; uint64_t n_brute; double mean; "
                     r"double std;\s*float score_min; float score_max; float first_radius; float threshold; uint32_t rounds; uint32_t grid_bits;"
                     r"\s*\} gsx_knn_stats_t;", hdr)
    assert re.search(r"typedef struct gsx_knn_select_desc \{\s*uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t mode;[^}]*"
                     r"uint32_t k; uint32_t score; float radius_hint; uint32_t grid_bits;\s*uint32_t max_rounds; float lo; float hi; "
                     r"float std_ratio;\s*\} gsx_knn_select_desc;", hdr)
    assert re.search(r"^void gsx_knn_desc_default\(gsx_knn_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_knn\(gsx_viewer\* v, const char\* key, const gsx_knn_desc\* desc, float\* out_d2 /\*[^/]*\*/,\s*"
                     r"float\* out_score /\*[^/]*\*/, gsx_knn_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_knn\(gsx_viewer\* v, const char\* key, const gsx_knn_select_desc\* desc, uint64_t\* out_hit, "
                     r"uint64_t\* out_selected,\s*gsx_knn_stats_t\* out_stats[^)]*\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    assert "§20" in hdr and "## 20. Model nearest neighbours [BUILD-SPEC]" in _read("spec", "RENDER_SPEC.md")


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.KnnDesc) == 32
    assert offsets(_lib.KnnDesc) == {"filter": 0, "flags": 4, "k": 8, "score": 12, "radius_hint": 16, "grid_bits": 20, "max_rounds": 24,
                                     "reserved": 28}
    assert C.sizeof(_lib.KnnStats) == 72
    assert offsets(_lib.KnnStats) == {"count": 0, "n_nonfinite": 8, "n_scored": 16, "n_brute": 24, "mean": 32, "std": 40, "score_min": 48,
                                      "score_max": 52, "first_radius": 56, "threshold": 60, "rounds": 64, "grid_bits": 68}
    assert C.sizeof(_lib.KnnSelectDesc) == 48
    assert offsets(_lib.KnnSelectDesc) == {"filter": 0, "flags": 4, "selection_op": 8, "mode": 12, "k": 16, "score": 20, "radius_hint": 24,
                                           "grid_bits": 28, "max_rounds": 32, "lo": 36, "hi": 40, "std_ratio": 44}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_knn.cpp")
    assert "static_assert(sizeof(gsx_knn_desc) == 32 && sizeof(gsx_knn_stats_t) == 72 && sizeof(gsx_knn_select_desc) == 48" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[1:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_knn_desc", "gsx_knn_stats_t", "gsx_knn_select_desc"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub const GSX_KNN_MAX_K: u32 = 16;" in rust_sys and "pub mean: f64, pub std: f64" in rust_sys
    for method in ("knn", "select_knn"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.KnnDesc(7, 7, 7, 7, 7.0, 7, 7, 7)
    L.gsx_knn_desc_default(C.byref(d))
    assert (d.filter, d.flags, d.k, d.score, d.radius_hint, d.grid_bits, d.max_rounds, d.reserved) == (0, 0, 3, _lib.GSX_KNN_SCORE_MEAN, 0.0, 0, 0, 0)
    L.gsx_knn_desc_default(None)
    # without a device: a status code and a message, not a crash
    rows, score, stats = (C.c_float * 12)(), (C.c_float * 4)(), _lib.KnnStats()
    assert L.gsx_model_knn(None, b"a", C.byref(d), rows, score, C.byref(stats)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_knn" in L.gsx_last_error_string()
    sd = _lib.KnnSelectDesc(0, 0, 0, _lib.GSX_KNN_SELECT_OUTLIERS, 3, _lib.GSX_KNN_SCORE_MEAN, 0.0, 0, 0, 0.0, 0.0, 2.0)
    assert L.gsx_model_select_knn(None, b"a", C.byref(sd), None, None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_knn" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("knn", "select_knn"))


def test_the_rules_have_one_copy_and_the_build_lists_the_sources():
    kernels, api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_knn.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_knn.cpp")
    math_h, driver = _read("wgpu_3dgs_viewer_app_amd", "csrc", "knn_math.h"), _read("tests", "knn_driver.cpp")
    for text in (kernels, api, driver):
        assert '#include "knn_math.h"' in text
        for rule in ("inline void knn_insert(", "inline bool knn_proven(", "inline float knn_score(", "inline bool knn_go_brute(", "inline float nb_d2("):
            assert rule not in text
    for rule in ("inline void knn_insert(", "inline bool knn_proven(", "inline float knn_score(", "inline float knn_threshold(",
                 "inline float knn_radius_floor(", "inline float knn_first_radius(", "inline float knn_next_radius(", "inline bool knn_go_brute("):
        assert math_h.count(rule) == 1, rule
    assert '#include "neighbors_math.h"' in math_h and "nb_d2(" not in math_h.split("#pragma once")[1]  # the distance is section 18's
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_knn.hip" in makefile and "gsx_api_knn.cpp" in makefile and "-ffp-contract=off" in makefile
    # the loop over the rounds has one copy too: the library and the driver run radius_search.h, and neither decides the fallback itself
    search = driver.split("static void search(")[1].split("\n}\n")[0]
    assert '#include "radius_search.h"' in api and '#include "radius_search.h"' in driver and "radius_search<" in api and "radius_search<" in search
    assert "knn_go_brute(" not in api and "knn_go_brute(" not in search and "#include <hip" not in _read("wgpu_3dgs_viewer_app_amd", "csrc", "radius_search.h")
    sources = [_read("tests", f) for f in sorted(os.listdir(os.path.join(ROOT, "tests"))) if f.endswith((".cpp", ".h"))]
    assert sum(s.count("struct Grid {") for s in sources) == 1 and sum(s.count("Grid build_grid(") for s in sources) == 1  # grid_replay.h


# ---- 2. csrc/knn_math.h: the driver -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knn") / "knn_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "knn_driver.cpp"), "-o", exe])
    return exe


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def _fx(x):
    return f"{int(np.array([x], F).view(np.uint32)[0]):x}"


def _floats(ws):
    return np.array([int(w, 16) for w in ws], np.uint32).view(F)


def _search(driver, pos, k, score=K.SCORE_MEAN, hint=0.0, grid_bits=0, max_rounds=0):
    """(participants, rounds, n_brute, first_radius, rows, scores) of the driver's search; its own O(n^2) check must hold"""
    pos = np.ascontiguousarray(pos, F)
    text = f"search {k:x} {score:x} {_fx(hint)} {grid_bits:x} {max_rounds:x} {' '.join(f'{w:x}' for w in pos.reshape(-1).view(np.uint32))}\n"
    head, rows, scores = _play(driver, text)
    assert head[0] == "search" and head[5:] == ["0", "0"], head  # rows / scores that differ from the driver's definition
    return (int(head[1]), int(head[2]), int(head[3]), _floats([head[4]])[0], _floats(rows[1:]).reshape(pos.shape[0], k), _floats(scores[1:]))


def _same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def _uniform(n, seed=0):
    return np.random.default_rng(seed).random((n, 3)).astype(F)


def _two_scales(seed=1):
    """a dense blob and a sparse cloud at densities 1 : 1000 per axis"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.random((800, 3)) * 1e-3, rng.random((800, 3)) + 5.0]).astype(F)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 9, 16])
def test_the_search_equals_the_definition_and_the_restatement_on_a_uniform_set(driver, k):
    pos = _uniform(2000, k)
    pos[7] = [np.nan, 0, 0]
    part = N.participates(pos)
    want = K.brute(pos, part, k)
    for score in (K.SCORE_KTH, K.SCORE_MEAN):
        P, rounds, n_brute, _, rows, scores = _search(driver, pos, k, score)
        assert P == 1999 and rounds >= 1
        assert _same(rows, want) and _same(scores, K.score(want, score))
        assert np.isinf(rows[7]).all() and np.isinf(scores[7])


def test_no_knob_changes_a_row(driver):
    """tiny, huge and chosen first radii; max_rounds 1, 2 and 0; forced tables"""
    for uniform, pos in ((True, _uniform(1200, 3)), (False, _two_scales())):
        part = N.participates(pos)
        want = K.brute(pos, part, 5)
        d = K.kth_distance_median(pos, part)
        seen = set()
        for hint, grid_bits, max_rounds in ((0.0, 0, 0), (d * 1e-6, 0, 1), (d * 1e-6, 0, 2), (d * 1e-6, 0, 0), (d * 1e6, 0, 0), (d, 0, 0),
                                            (d * 3, 3, 0), (d * 0.5, 12, 2), (0.0, 1, 0)):
            P, rounds, n_brute, first, rows, scores = _search(driver, pos, 5, K.SCORE_MEAN, hint, grid_bits, max_rounds)
            assert _same(rows, want) and _same(scores, K.score(want, K.SCORE_MEAN)), (hint, grid_bits, max_rounds)
            seen.add((rounds, n_brute))
            if hint == F(d * 1e-6):
                assert first > F(hint)  # the floor lifted it
                if max_rounds == 1 and uniform:
                    assert (rounds, n_brute) == (1, P)  # one round proves nothing at that radius: everything goes to the fallback
                if max_rounds == 0 and uniform:
                    assert rounds >= 2
            if hint == F(d * 1e6):
                assert (rounds, n_brute) == (1, 0)  # one cell, one round
        assert len(seen) >= 3  # the paths differ; the rows do not


def test_engineered_sets(driver):
    lat = N.lattice()
    every = np.ones(lat.shape[0], bool)
    for k in (6, 7):  # the k-th distance ties at 6, and the 7th is 0.25 * sqrt(2) away
        _, _, _, _, rows, scores = _search(driver, lat, k, K.SCORE_KTH)
        assert _same(rows, K.brute(lat, every, k))
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    _, _, _, _, rows, scores = _search(driver, same, 16)
    assert not rows.any() and not scores.any()
    few = np.tile(F([0.3, -1.7, 2.9]), (10, 1))  # fewer than k others: nine zeros and seven +inf
    P, rounds, n_brute, _, rows, scores = _search(driver, few, 16)
    assert (rows[:, :9] == 0).all() and np.isinf(rows[:, 9:]).all() and np.isinf(scores).all() and n_brute == 10
    groups = np.concatenate([np.tile(_uniform(40, 5)[:, None, :], (1, 3, 1)).reshape(-1, 3),   # groups of 3: smaller than k
                             np.tile(_uniform(4, 6)[:, None, :], (1, 40, 1)).reshape(-1, 3),   # groups of 40: larger than k
                             _uniform(1200, 7)])
    _, _, _, _, rows, _ = _search(driver, groups, 8)
    assert _same(rows, K.brute(groups, np.ones(groups.shape[0], bool), 8)) and (rows[:120, :2] == 0).all() and (rows[120:280, :8] == 0).all()
    far = _uniform(1100, 8)
    far[3], far[4], far[5] = [3e38, 0, 0], [-3e38, -3e38, 3e38], [3e38, 3e38, 3e38]  # differences overflow: +inf, no NaN
    P, rounds, n_brute, _, rows, scores = _search(driver, far, 3)
    assert _same(rows, K.brute(far, np.ones(1100, bool), 3)) and n_brute >= 3 and not np.isnan(rows).any()
    assert np.isinf(rows[4]).all() and np.isinf(scores[4])


def test_small_sets_go_straight_to_the_fallback(driver):
    for n, k in ((1, 3), (2, 3), (65, 1), (1024, 3), (1025, 3)):
        pos = _uniform(n, n)
        P, rounds, n_brute, _, rows, _ = _search(driver, pos, k)
        assert _same(rows, K.brute(pos, np.ones(n, bool), k))
        assert (rounds, n_brute) == (0, n) if n <= 1024 else rounds >= 1
    assert np.isinf(_search(driver, _uniform(2, 2), 3)[4][:, 1:]).all()


@pytest.mark.parametrize("width", [4, 8, 16])
def test_the_chain_keeps_the_smallest_with_multiplicity(driver, width):
    rng = np.random.default_rng(width)
    text, want = "", []
    for k in range(1, width + 1):
        for count in (0, 1, k - 1, k, k + 1, 200):
            v = rng.integers(0, 12, count).astype(F) * F(0.25)  # many ties, zeros among them
            if count == 200 and k % 2:
                v[::7] = np.inf
            text += f"chain {width:x} {k:x} {' '.join(_fx(x) for x in v)}\n"
            want.append(np.concatenate([np.sort(v), np.full(k, np.inf, F)])[:k])
    for ln, w in zip(_play(driver, text), want):
        assert ln[0] == "chain" and _same(_floats(ln[1:]), w)


def test_the_radius_floor_keeps_the_extent_within_32000_cells(driver):
    extents = [(1.0, 0.5, 0.1), (1e-3, 0, 0), (0, 0, 0), (7e5, 3.0, 2e4), (1e30, 1.0, 1.0), (3.4e38, 3.4e38, 3.4e38), (1e-30, 1e-31, 0)]
    out = _play(driver, "".join(f"floor {_fx(a)} {_fx(b)} {_fx(c)}\n" for a, b, c in extents))
    for e, ln in zip(extents, out):
        floor = float(_floats(ln[1:])[0])
        largest = float(F(max(e)))
        if largest / 32000.0 < 1.8e19:
            assert floor == float(F(largest / 32000.0))
            if floor >= 1e-22:  # the cell edge is above the radius: the extent spans fewer than 32 000 of them, under the clamp at 32 767
                _, h, _ = N.grid_of(floor)
                assert largest / float(h) < 32000 < N.MAX_CELL
        else:
            assert floor == float(F(1.8e19)) and N.radius_ok(floor)
    out = _play(driver, "first 3f800000 3f800000 3f800000 f4240 3\nfirst 3f800000 3f800000 0 f4240 3\nfirst 0 0 0 a 3\nfirst 7f7fffff 7f7fffff 7f7fffff 2 10\n")
    cube, flat, point, huge = (float(_floats(ln[1:])[0]) for ln in out)
    assert cube == float(F(np.cbrt(0.48 * 3 / 1e6))) and flat == float(F(np.sqrt(0.64 * 3 / 1e6))) and point == 1.0 and huge == float(F(1.8e19))


def test_the_budget_rule_overrides_max_rounds(driver):
    nxt = _fx(1.0)
    cases = [  # U, P, rounds, max_rounds, next radius, coarse -> go to the fallback?
        (5000, 5000, 0, 0, nxt, 0, 0), (1024, 10 ** 6, 0, 0, nxt, 0, 1), (1025, 1025, 0, 0, nxt, 0, 0), (1024, 1024, 0, 5, nxt, 0, 1),
        (5000, 5000, 1, 1, nxt, 0, 1), (5000, 5000, 1, 2, nxt, 0, 0), (5000, 5000, 2, 2, nxt, 0, 1),
        (10 ** 6, 10 ** 7, 1, 1, nxt, 0, 0), (10 ** 6, 10 ** 7, 64, 64, nxt, 1, 0),   # the knob cannot start 10^13 tests
        (13743, 10 ** 7, 1, 1, nxt, 0, 1), (13745, 10 ** 7, 1, 1, nxt, 0, 0),         # 2^37 / 10^7 = 13743.9
        (1024, 2 ** 27, 3, 0, nxt, 0, 1), (1024, 2 ** 27 + 1, 3, 0, nxt, 0, 0),
        (5000, 5000, 0, 0, nxt, 1, 0), (5000, 5000, 1, 0, nxt, 1, 1), (10000, 10 ** 7, 2, 0, nxt, 1, 1),  # a coarse grid, after a round
        (10 ** 6, 10 ** 7, 9, 0, "0", 0, 1),                                          # the radius cannot grow: there is no other way
    ]
    out = _play(driver, "".join(f"brute {u:x} {p:x} {r:x} {m:x} {n} {c:x}\n" for u, p, r, m, n, c, _ in cases))
    assert [int(ln[1]) for ln in out] == [c[6] for c in cases]
    one = _fx(1.0)
    out = _play(driver, f"coarse {_fx(0.05)} {one} {one} {one}\ncoarse {_fx(0.0499)} {one} {one} {one}\ncoarse {_fx(0.2)} {_fx(4.0)} {_fx(4.0)} 0\n"
                        f"coarse {_fx(0.19)} {_fx(4.0)} {_fx(4.0)} 0\ncoarse {one} 0 0 0\n")
    assert [int(ln[1]) for ln in out] == [1, 0, 1, 0, 0]


def test_the_threshold_is_the_double_expression_rounded_once(driver):
    rng = np.random.default_rng(5)
    text, want = "", []
    for _ in range(200):
        mean, std, ratio = rng.random() * 3, rng.random(), F(rng.normal() * 3)
        lo, hi = struct.unpack("<II", struct.pack("<d", mean))
        slo, shi = struct.unpack("<II", struct.pack("<d", std))
        text += f"threshold {lo:x} {hi:x} {slo:x} {shi:x} {_fx(ratio)}\n"
        want.append(K.threshold(mean, std, ratio))
    got = _floats([ln[1] for ln in _play(driver, text)])
    assert _same(got, np.array(want, F))


# ---- 3. the restatement: what the GPU tests expect of it ---------------------------------------------------------------------------------
def test_the_restatement_on_the_lattice_and_on_coincident_points():
    lat = N.lattice()
    every = np.ones(lat.shape[0], bool)
    rows = K.brute(lat, every, 7)
    interior = (np.abs(np.rint(lat / F(0.25))) < 4).all(axis=1)
    assert (rows[interior, :6] == F(0.0625)).all() and (rows[interior, 6] == F(0.125)).all()  # six at 0.25, the next at 0.25 sqrt 2
    assert (K.score(rows[:, :6], K.SCORE_KTH)[interior] == F(0.25)).all() and (K.score(rows[:, :6], K.SCORE_MEAN)[interior] == F(0.25)).all()
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    rows = K.brute(same, np.ones(300, bool), 16)
    st = K.stats(K.score(rows, K.SCORE_MEAN))
    assert not rows.any() and st == dict(n_scored=300, score_min=0, score_max=0, mean=0.0, std=0.0)
    rows = K.brute(same[:10], np.ones(10, bool), 16)
    assert (rows[:, :9] == 0).all() and np.isinf(rows[:, 9:]).all()
    assert K.stats(K.score(rows, K.SCORE_KTH)) == dict(n_scored=0, score_min=0, score_max=0, mean=0.0, std=0.0)
    part = np.ones(10, bool)
    part[3] = False
    rows = K.brute(same[:10], part, 3)
    assert np.isinf(rows[3]).all() and not rows[part].any()


def test_the_restatement_scores_statistics_and_hits():
    pos = _uniform(600, 11)
    pos[5] = [40, 40, 40]  # a floater
    part = np.ones(600, bool)
    part[::50] = False
    rows = K.brute(pos, part, 3)
    mean = K.score(rows, K.SCORE_MEAN)
    want = ((np.sqrt(rows[:, 0]) + np.sqrt(rows[:, 1])).astype(F) + np.sqrt(rows[:, 2])).astype(F) / F(3)
    assert _same(mean, want) and _same(K.score(rows, K.SCORE_KTH), np.sqrt(rows[:, 2]))
    st = K.stats(mean)
    finite = mean[np.isfinite(mean)].astype(np.float64)
    assert st["n_scored"] == part.sum() and st["mean"] == pytest.approx(finite.mean(), rel=1e-14) and st["std"] == pytest.approx(finite.std(ddof=1), rel=1e-12)
    out = K.hit(mean, part, K.SELECT_OUTLIERS, std_ratio=2.0)
    assert out[5] and 1 <= out.sum() < 60 and not out[~part].any()
    t = K.threshold(st["mean"], st["std"], 2.0)
    assert np.array_equal(out, part & (mean > t))
    assert np.array_equal(K.hit(mean, part, K.SELECT_RANGE, 0.0, np.inf), part)
    assert K.hit(mean, part, K.SELECT_RANGE, st["score_min"], st["score_min"]).sum() >= 1
    assert not K.hit(np.full(4, np.inf, F), np.ones(4, bool), K.SELECT_OUTLIERS, std_ratio=0.0).any()  # no finite score: nobody is hit


def test_the_restatement_agrees_with_a_kd_tree_where_scipy_is_there():
    spatial = pytest.importorskip("scipy.spatial")
    pos = _uniform(3000, 13)
    rows = K.brute(pos, np.ones(3000, bool), 8)
    d, _ = spatial.cKDTree(pos.astype(np.float64)).query(pos.astype(np.float64), k=9)
    assert np.allclose(np.sqrt(rows.astype(np.float64)), d[:, 1:], rtol=1e-5, atol=0)
