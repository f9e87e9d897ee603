"""Model decimate (gsx_model_decimate, gsx_model_decimate_edge; spec §22) without a device: the entry points and the structs in the
header, the library, the bindings and the facades; and the float32 rules of csrc/decimate_math.h — played by
tests/decimate_driver.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers and run as a child
process — against the float64 restatement tests/decimate_ref.py: cells, representatives, order, map and statistics exactly, merged
values within a measured tolerance.

The tolerance.  Over FIXTURES, float32 driver against float64 reference, the worst deviation of a merged cell's output relative to
the largest magnitude of that output in the cell (the mean: relative to the larger of that and the cell edge, since its error is in
the offset from the representative) was measured as OBSERVED below; the bound is 8 x that: headroom for other seeds, not for other
arithmetic.  The fixtures keep det Sigma within 1e-11 .. 1e-4."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import decimate_ref as D
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = D.ROOT
F = np.float32
FUNCTIONS = ("gsx_decimate_desc_default", "gsx_model_decimate", "gsx_model_decimate_edge")
#: (seed, n, cell): a few members a cell, dozens, mostly singletons, ONE cell of 1800 members, nearly all singletons
FIXTURES = ((1, 3000, 0.25), (2, 3000, 0.5), (3, 4000, 0.1), (4, 2000, 2.5), (5, 3000, 0.05))
OBSERVED = {"pos": 2.24e-7, "cov": 3.36e-6, "sh": 2.33e-6, "alpha": 2.58e-6}
BOUND = {k: 8.0 * v for k, v in OBSERVED.items()}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"typedef struct gsx_decimate_desc\s*\{ uint32_t filter; uint32_t flags; float cell; uint32_t grid_bits; uint32_t reserved\[2\]; \} "
                     r"gsx_decimate_desc;", hdr)
    assert re.search(r"typedef struct gsx_decimate_stats_t \{ uint64_t count; uint64_t n_nonfinite; uint64_t cells; uint64_t singletons; "
                     r"uint32_t largest_cell; uint32_t grid_bits; \} gsx_decimate_stats_t;", hdr)
    assert re.search(r"^void gsx_decimate_desc_default\(gsx_decimate_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_decimate\(gsx_viewer\* v, const char\* src_key, const char\* dst_key[^,]*, const gsx_decimate_desc\* desc,\s*"
                     r"uint32_t\* out_map[^;]*, gsx_decimate_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_decimate_edge\(gsx_viewer\* v, const char\* key, uint32_t filter, uint32_t flags, uint64_t target_cells,\s*"
                     r"float\* out_cell, uint64_t\* out_cells\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays


def test_ctypes_mirrors_have_the_header_layout(driver):
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.DecimateDesc) == 24
    assert offsets(_lib.DecimateDesc) == {"filter": 0, "flags": 4, "cell": 8, "grid_bits": 12, "reserved": 16}
    assert C.sizeof(_lib.DecimateStats) == 40
    assert offsets(_lib.DecimateStats) == {"count": 0, "n_nonfinite": 8, "cells": 16, "singletons": 24, "largest_cell": 32, "grid_bits": 36}
    assert D.play_desc(driver) == (24, 40, 8, 12, 16, 16, 24, 32, 36)  # the C compiler's layout of include/gsx.h
    assert "static_assert(sizeof(gsx_decimate_desc) == 24 && sizeof(gsx_decimate_stats_t) == 40" in _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_decimate.cpp")
    assert _lib.GSX_DECIMATE_NO_CELL == D.NO_CELL == 0xFFFFFFFF


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[1:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_decimate_desc", "gsx_decimate_stats_t"):
        assert "pub struct " + s + " " in rust_sys
    for method in ("decimate", "decimate_count", "decimate_edge"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.DecimateDesc(7, 7, 7.0, 7, (7, 7))
    L.gsx_decimate_desc_default(C.byref(d))
    assert bytes(d) == bytes(24)  # filter 0, flags 0, cell 0 (must be set), the library's table, reserved 0
    L.gsx_decimate_desc_default(None)
    # without a device: a status code and a message, not a crash
    stats, cell, cells = _lib.DecimateStats(), C.c_float(), C.c_uint64()
    d.cell = 1.0
    assert L.gsx_model_decimate(None, b"a", b"b", C.byref(d), None, C.byref(stats)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_decimate" in L.gsx_last_error_string()
    assert L.gsx_model_decimate_edge(None, b"a", 0, 0, 10, C.byref(cell), C.byref(cells)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_decimate_edge" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("decimate", "decimate_count", "decimate_edge"))


def test_the_rules_have_one_copy_and_the_build_lists_the_sources():
    kernels, api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_decimate.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_decimate.cpp")
    math_h, driver = _read("wgpu_3dgs_viewer_app_amd", "csrc", "decimate_math.h"), _read("tests", "decimate_driver.cpp")
    for text in (kernels, api, driver):
        assert '#include "decimate_math.h"' in text and "inline uint32_t nb_cell(" not in text and "inline float dec_acc(" not in text
    assert math_h.count("inline float dec_acc(") == 1 and "inline uint32_t nb_cell(" not in math_h
    assert "decimate_math" not in _read("tests", "decimate_ref.py").split('"""', 2)[2]  # the reference does not lean on the header
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_decimate.hip" in makefile and "gsx_api_decimate.cpp" in makefile and "-ffp-contract=off" in makefile
    assert int(re.search(r"kDecLdsBucket = (\d+)u", math_h).group(1)) <= 30000  # the GPU tests put 2 x that + 3 into one cell


# ---- 2. csrc/decimate_math.h: the driver against the float64 reference ---------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return D.build_driver(tmp_path_factory.mktemp("decimate"))


def _same_integers(got, want, what=""):
    assert np.array_equal(got["map"], want["map"]), what
    for k in ("count", "n_nonfinite", "cells", "singletons", "largest_cell"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["members"], want["members"]), what


def _deviations(got, want, cell):
    """worst relative deviation per output over the merged cells, and the worst byte differences"""
    mg = want["members"] > 1
    out = {}
    for name, floor in (("pos", float(cell)), ("cov", 0.0), ("sh", 0.0)):
        a, b = got[name][mg].astype(np.float64), want[name][mg]
        out[name] = float((np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), floor)).max())
    a, b = got["alpha"][mg].astype(np.float64), want["alpha"][mg]
    out["alpha"] = float((np.abs(a - b) / np.where(b > 0, b, 1.0)).max())
    rgb = np.stack([(got["color"] >> (8 * k)) & 0xFF for k in range(3)], axis=1).astype(np.int64)
    out["rgb"] = int(np.abs(rgb - want["rgb"])[mg].max())
    out["a"] = int(np.abs((got["color"] >> 24).astype(np.int64) - want["a"])[mg].max())
    return out


def _singletons_are_copies(got, want, planes):
    s = want["members"] == 1
    rep = want["rep"][s]
    for k, plane in enumerate(planes):
        assert np.ascontiguousarray(got["planes"][k][s]).tobytes() == np.ascontiguousarray(plane[rep]).tobytes(), k


@pytest.mark.parametrize("seed,n,cell", FIXTURES)
def test_driver_against_the_reference(driver, seed, n, cell):
    planes = D.random_planes(n, seed)
    kept = np.random.default_rng(seed).random(n) < 0.9
    got, want = D.play(driver, planes, kept, cell), D.decimate(planes[0], planes[1], planes[3], planes[2], kept, cell)
    _same_integers(got, want, seed)
    assert want["cells"] > 0 and (want["members"] > 1).any() and want["mass"].all()
    assert np.array_equal(np.sort(want["rep"]), want["rep"])  # dst is in ascending order of representative
    dev = _deviations(got, want, cell)
    print(seed, dev)
    for k in ("pos", "cov", "sh", "alpha"):
        assert dev[k] <= BOUND[k], (k, dev[k], BOUND[k])
    assert dev["rgb"] <= 1 and dev["a"] <= 1  # a byte is a rounded value: a tie may fall either way
    _singletons_are_copies(got, want, planes)
    if seed == 4:
        assert want["cells"] == 1 and want["largest_cell"] == want["count"] > 1500  # all of it in one cell
    if seed == 5:
        assert want["singletons"] > 0.9 * want["cells"]


def test_nonfinite_filtered_and_clamped(driver):
    n = 600
    pos, color, sh, cov = (np.array(a) for a in D.random_planes(n, 6))
    pos[5, 0], pos[77, 1], pos[599, 2] = np.nan, np.inf, -np.inf
    pos[10] = [40000.0, 0, 0]   # u = 40000 / cell: beyond the clamp on x, and
    pos[11] = [50000.0, 0, 0]   # ... joined with it
    kept = np.ones(n, bool)
    kept[[77, 100, 101]] = False
    planes = (pos, color, sh, cov)
    cell = 1.0
    got, want = D.play(driver, planes, kept, cell), D.decimate(pos, color, cov, sh, kept, cell)
    _same_integers(got, want)
    assert want["n_nonfinite"] == 2 and want["count"] == n - 5
    assert (want["map"][[5, 77, 100, 101, 599]] == D.NO_CELL).all()
    assert want["map"][10] == want["map"][11] != D.NO_CELL  # cells 39999 and 49999 are both the clamp, 32767
    # nothing kept: no cells
    none = D.play(driver, planes, np.zeros(n, bool), cell)
    assert none["cells"] == 0 and none["count"] == 0 and (none["map"] == D.NO_CELL).all() and none["pos"].size == 0


def _copies(k, alpha_byte, seed=7):
    """k coincident copies of each of 50 Gaussians with det Sigma = 1 (diag 0.25, 1, 4, rotated by a quarter turn: exact) at
    well-separated places: every mass is alpha, every cell holds one Gaussian's copies"""
    rng = np.random.default_rng(seed)
    base = 50
    pos = (np.arange(base)[:, None] * np.float32([3, 0, 0]) + rng.random((base, 3)).astype(F)).astype(F)
    cov = np.tile(F([0.25, 0, 0, 4, 0, 1]), (base, 1))
    color = (rng.integers(0, 256, base, dtype=np.uint32) | (rng.integers(0, 256, base, dtype=np.uint32) << 8) | np.uint32(alpha_byte << 24)).astype(np.uint32)
    sh = (rng.normal(size=(base, 45)) * 0.3).astype(F)
    order = rng.permutation(base * k)  # the copies are scattered over the index range
    rows = np.repeat(np.arange(base), k)[order]
    return (pos[rows], color[rows], sh[rows], cov[rows]), rows


@pytest.mark.parametrize("k", [2, 4])
def test_coincident_duplicates_keep_their_bits_and_clamp_opacity(driver, k):
    planes, rows = _copies(k, 255)
    n = rows.size
    got = D.play(driver, planes, np.ones(n, bool), 1.0)
    want = D.decimate(planes[0], planes[1], planes[3], planes[2], np.ones(n, bool), 1.0)
    _same_integers(got, want, k)
    assert got["cells"] == 50 and got["singletons"] == 0 and got["largest_cell"] == k
    rep = want["rep"]
    # d = 0 and the weights are 1: sums of k equal terms, times 1 / k: exact
    for name, plane in (("pos", planes[0]), ("cov", planes[3]), ("sh", planes[2])):
        assert got[name].tobytes() == np.ascontiguousarray(plane[rep]).tobytes(), name
    assert np.array_equal(got["color"] & 0xFFFFFF, planes[1][rep] & 0xFFFFFF)
    # k opaque copies carry k times the mass of one: alpha' = min(1, k / 1) = 1
    assert (got["alpha"] == 1.0).all() and ((got["color"] >> 24) == 255).all() and (want["alpha"] == 1.0).all()


def test_the_uniform_fallback(driver):
    planes, rows = _copies(3, 0, seed=8)
    pos = planes[0] + (np.random.default_rng(9).random(planes[0].shape).astype(F) * F(0.5))  # apart, inside their cells' neighbourhood
    planes = (pos.astype(F), planes[1], planes[2], planes[3])
    n = rows.size
    got = D.play(driver, planes, np.ones(n, bool), 8.0)
    want = D.decimate(planes[0], planes[1], planes[3], planes[2], np.ones(n, bool), 8.0)
    _same_integers(got, want)
    assert not want["mass"].any() and (want["members"] > 1).all()  # every opacity byte is 0: no mass anywhere
    dev = _deviations(got, want, 8.0)
    for key in ("pos", "cov", "sh"):
        assert dev[key] <= BOUND[key], (key, dev[key])
    assert (got["alpha"] == 0.0).all() and ((got["color"] >> 24) == 0).all()  # max alpha_i = 0
    # the plain mean of the members
    j = want["map"].astype(np.int64)
    mean = np.stack([np.bincount(j, weights=planes[0][:, a].astype(np.float64)) for a in range(3)], axis=1) / want["members"][:, None]
    assert np.abs(got["pos"] - mean).max() <= 8.0 * BOUND["pos"]


@pytest.mark.parametrize("target", [1, 2, 37, 500, 2999, 10 ** 6])
def test_the_bisection_agrees_with_the_restatement(driver, target):
    planes = D.random_planes(3000, 10)
    kept = np.random.default_rng(10).random(3000) < 0.8
    edge, cells = D.play_edge(driver, planes, kept, target)
    want_edge, want_cells = D.find_edge(planes[0], kept, target)
    assert (edge.tobytes(), cells) == (want_edge.tobytes(), want_cells)
    assert 1 <= cells <= target and cells == D.assign(planes[0], kept, edge)[3].size
    if target == 1:
        assert cells == 1


def test_the_bisection_at_its_edges(driver):
    planes = D.random_planes(100, 11)
    same = (np.tile(planes[0][:1], (100, 1)), planes[1], planes[2], planes[3])
    assert D.play_edge(driver, same, np.ones(100, bool), 5) == D.find_edge(same[0], np.ones(100, bool), 5) == (F(1), 1)  # extent 0
    assert D.play_edge(driver, planes, np.zeros(100, bool), 5) == D.find_edge(planes[0], np.zeros(100, bool), 5) == (F(0), 0)  # nobody
    assert [D.cell_ok(c) for c in (0.0, -1.0, float("nan"), float("inf"), 1e-39, 2e-39, 1.0, 3e38)] == [False, False, False, False, False, False, True, True]


# ---- 3. the visual check's fixture, on the CPU oracle first ----------------------------------------------------------------------------
def test_a_twice_stored_model_decimates_to_its_single_copy_on_the_oracle(driver):
    """Every Gaussian twice at half the opacity mass, a tiny cell: the float32 rules give the single copy back to a rounding, and
    the oracle's frame of the result lies within spec section 8's framebuffer tolerance of the single copy's.  This is the
    confirmation tests/test_gpu_decimate.py's visual check rests on."""
    import oracle
    from tests import common
    from tests.model_ops import H, W
    from wgpu_3dgs_viewer_app_amd import camera

    single, twice, rows, cell = D.twice_stored()
    n = single[0].shape[0]
    lo, hi = single[0].min(axis=0), single[0].max(axis=0)
    assert float((hi - lo).max()) / float(cell) < 32767  # no cells joined at the clamp
    got = D.play(driver, twice, np.ones(2 * n, bool), cell)
    assert (got["cells"], got["singletons"], got["largest_cell"]) == (n, 0, 2) and (got["members"] == 2).all()
    first = rows[np.sort(np.unique(rows, return_index=True)[1])]  # dst order: ascending representative
    assert got["pos"].tobytes() == single[0][first].tobytes() and np.array_equal(got["color"], single[1][first])
    dev_cov = np.abs(got["cov"] - single[3][first]).max() / np.abs(single[3]).max()
    dev_sh = np.abs(got["sh"] - single[2][first]).max()
    print("cov", dev_cov, "sh", dev_sh)
    assert dev_cov <= 4 * 2.0 ** -24 and dev_sh <= 4 * 2.0 ** -24 * max(1.0, float(np.abs(single[2]).max()))
    worst = 0.0
    for pose in (5, 6, 7):
        f = common.oracle_frame(camera.orbit_pose(pose), W, H)
        fa, fb = oracle.new_framebuffer(f), oracle.new_framebuffer(f)
        oracle.render_model(f, *single, fa)
        oracle.render_model(f, *got["planes"], fb)
        assert fa[..., :3].max() > 0
        worst = max(worst, float(np.abs(fa - fb).max()))
    print("frame L-inf", worst)
    assert worst <= 1e-3  # spec section 8
