"""Model neighbours (gsx_model_neighbors, gsx_model_select_neighbors; spec §18) without a device: the entry points and the structs in
the header, the library, the bindings and the facades; the cell function of csrc/neighbors_math.h — played by
tests/neighbors_driver.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers and run as a child
process — over generated pairs and against the numpy restatement tests/neighbors_ref.py; and the restatement's grid version against
its brute-force definition, with the expectations the GPU tests rely on (lattice, coincident points)."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import neighbors_ref as N
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCTIONS = ("gsx_neighbor_desc_default", "gsx_model_neighbors", "gsx_model_select_neighbors")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^#define GSX_NEIGHBOR_MAX_COUNT 4095u", hdr, re.M) and _lib.GSX_NEIGHBOR_MAX_COUNT == 4095 == N.MAX_COUNT
    assert re.search(r"typedef struct gsx_neighbor_desc \{ uint32_t filter; uint32_t flags; float radius; uint32_t max_count; uint32_t grid_bits; "
                     r"uint32_t reserved; \} gsx_neighbor_desc;", hdr)
    assert re.search(r"typedef struct gsx_neighbor_stats_t \{ uint64_t count; uint64_t n_nonfinite; uint32_t grid_bits; uint32_t reserved; \} "
                     r"gsx_neighbor_stats_t;", hdr)
    assert re.search(r"typedef struct gsx_neighbor_select_desc \{\s*uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t max_count;[^}]*"
                     r"float radius; uint32_t count_lo; uint32_t count_hi; uint32_t grid_bits; uint32_t reserved\[2\];\s*\} gsx_neighbor_select_desc;", hdr)
    assert re.search(r"^void gsx_neighbor_desc_default\(gsx_neighbor_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_neighbors\(gsx_viewer\* v, const char\* key, const gsx_neighbor_desc\* desc, uint32_t\* out_counts, "
                     r"uint64_t\* out_hist, gsx_neighbor_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_neighbors\(gsx_viewer\* v, const char\* key, const gsx_neighbor_select_desc\* desc, "
                     r"uint64_t\* out_hit, uint64_t\* out_selected\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    assert (N.SET, N.ADD, N.REMOVE) == (_lib.GSX_SELECTION_SET, _lib.GSX_SELECTION_ADD, _lib.GSX_SELECTION_REMOVE)


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.NeighborDesc) == 24
    assert offsets(_lib.NeighborDesc) == {"filter": 0, "flags": 4, "radius": 8, "max_count": 12, "grid_bits": 16, "reserved": 20}
    assert C.sizeof(_lib.NeighborStats) == 24
    assert offsets(_lib.NeighborStats) == {"count": 0, "n_nonfinite": 8, "grid_bits": 16, "reserved": 20}
    assert C.sizeof(_lib.NeighborSelectDesc) == 40
    assert offsets(_lib.NeighborSelectDesc) == {"filter": 0, "flags": 4, "selection_op": 8, "max_count": 12, "radius": 16, "count_lo": 20,
                                                "count_hi": 24, "grid_bits": 28, "reserved": 32}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_neighbors.cpp")
    assert "static_assert(sizeof(gsx_neighbor_desc) == 24 && sizeof(gsx_neighbor_stats_t) == 24 && sizeof(gsx_neighbor_select_desc) == 40" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[1:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_neighbor_desc", "gsx_neighbor_stats_t", "gsx_neighbor_select_desc"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub const GSX_NEIGHBOR_MAX_COUNT: u32 = 4095;" in rust_sys
    for method in ("neighbors", "select_neighbors"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.NeighborDesc(7, 7, 7.0, 7, 7, 7)
    L.gsx_neighbor_desc_default(C.byref(d))
    assert (d.filter, d.flags, d.radius, d.max_count, d.grid_bits, d.reserved) == (0, 0, 1.0, 4095, 0, 0)
    L.gsx_neighbor_desc_default(None)
    # without a device: a status code and a message, not a crash
    counts, hist, stats = (C.c_uint32 * 4)(), (C.c_uint64 * 4096)(), _lib.NeighborStats()
    sd = _lib.NeighborSelectDesc(0, 0, 0, 4, 1.0, 0, 3, 0)
    assert L.gsx_model_neighbors(None, b"a", C.byref(d), counts, hist, C.byref(stats)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_neighbors" in L.gsx_last_error_string()
    assert L.gsx_model_select_neighbors(None, b"a", C.byref(sd), None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_neighbors" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("neighbors", "select_neighbors"))


def test_the_cell_function_has_one_copy_and_the_build_lists_the_sources():
    kernels, api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_neighbors.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_neighbors.cpp")
    math_h, driver = _read("wgpu_3dgs_viewer_app_amd", "csrc", "neighbors_math.h"), _read("tests", "neighbors_driver.cpp")
    for text in (kernels, api, driver):
        assert '#include "neighbors_math.h"' in text and "inline uint32_t nb_cell(" not in text
    assert math_h.count("inline uint32_t nb_cell(") == 1
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_neighbors.hip" in makefile and "gsx_api_neighbors.cpp" in makefile and "-ffp-contract=off" in makefile


# ---- 2. csrc/neighbors_math.h: the driver ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("neighbors") / "neighbors_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "neighbors_driver.cpp"), "-o", exe])
    return exe


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def _fx(x):
    return f"{int(np.array([x], F).view(np.uint32)[0]):x}"


RADII = [1e-4, 1e-3, 0.01, 0.1, 0.25, 1.0, 7.3, 100.0, 1e3]


def test_pairs_within_the_radius_lie_in_adjacent_cells(driver):
    """at least 10^6 pairs with d2 <= r2, radii from 1e-4 to 1e3 (and the extremes a call accepts): cells differ by at most 1 per
    axis and never decrease with the coordinate, whatever the origin below both"""
    radii = RADII + [4e-23, 1e-19, 1e19]  # r2 a denormal, r2 near the smallest normal, r2 near the largest float32
    out = _play(driver, "".join(f"grid {_fx(r)}\npairs {k + 1} 400000\n" for k, r in enumerate(radii)))
    rows = [ln for ln in out if ln[0] == "pairs"]
    assert len(rows) == len(radii)
    near = exact = clamped = 0
    for r, ln in zip(radii, rows):
        generated, n_near, n_exact, n_clamped, violations = (int(w) for w in ln[1:])
        assert violations == 0, (r, ln)
        assert n_near > generated // 4 and n_exact > 1000 and n_clamped > 1000, (r, ln)  # every kind of pair is there
        near, exact, clamped = near + n_near, exact + n_exact, clamped + n_clamped
    assert near >= 10 ** 6


def test_radius_check_and_grid_agree_with_the_restatement(driver):
    radii = RADII + [0.0, -1.0, float("nan"), float("inf"), 1e-23, 3e-23, 4e-23, 1e-19, 1.8e19, 1.9e19, 3e38]
    out = _play(driver, "".join(f"grid {_fx(r)}\n" for r in radii))
    for r, ln in zip(radii, out):
        ok = N.radius_ok(r)
        assert ln[1] == str(int(ok)), r
        if ok:
            r2, h, inv_h = N.grid_of(r)
            assert ln[2:] == [_fx(r2), _fx(h), _fx(inv_h)], r
            assert float(h) > float(F(r)) * 1.03 and np.isfinite(inv_h) and inv_h > 0
    assert [N.radius_ok(r) for r in (1e-23, 4e-23, 1.8e19, 1.9e19)] == [False, True, True, False]
    out = _play(driver, "auto 0 1 255 256 257 65536 65537 10000000 16777216 16777217 4294967295\n")
    assert [int(w) for w in out[0][1:]] == [N.auto_bits(n) for n in (0, 1, 255, 256, 257, 65536, 65537, 10000000, 16777216, 16777217, 4294967295)]
    assert (N.auto_bits(1), N.auto_bits(257), N.auto_bits(10 ** 7), N.auto_bits(2 ** 32)) == (8, 9, 24, 24)


@pytest.mark.parametrize("r", [0.25, 0.12, 1e-3, 100.0])
def test_cells_and_buckets_of_a_fixed_input_agree_with_the_restatement(driver, r):
    pos = np.concatenate([N.lattice(r, 5), N.special_scene(300)[0]])
    pos = pos[np.isfinite(pos).all(axis=1)]
    origin = pos.min(axis=0)
    _, _, inv_h = N.grid_of(r)
    want_c = np.stack([N.cells(pos[:, k], origin[k], inv_h) for k in range(3)], axis=1)
    for bits in (1, 4, 10, 24):
        text = f"grid {_fx(r)}\ncells {bits:x} {' '.join(_fx(o) for o in origin)} {' '.join(_fx(x) for x in pos.reshape(-1))}\n"
        got = np.array(_play(driver, text)[1][1:], np.int64).reshape(-1, 4)
        assert np.array_equal(got[:, :3], want_c), (r, bits)
        assert np.array_equal(got[:, 3], N.buckets(want_c[:, 0], want_c[:, 1], want_c[:, 2], bits)), (r, bits)
        assert got[:, 3].max() < (1 << bits)
    assert want_c.min() == 0 and want_c.max() == N.MAX_CELL  # the origin's cell, and the clamp (3e38)


# ---- 3. the restatement: grid against brute, and what the GPU tests expect of brute -----------------------------------------------------
def test_grid_equals_brute_on_a_random_scene():
    rng = np.random.default_rng(1)
    n = 5000
    pos = rng.standard_normal((n, 3)).astype(F)
    part = rng.random(n) < 0.8
    for r, cap in ((0.25, N.MAX_COUNT), (0.3, 8), (0.05, 1)):
        want = N.brute(pos, part, r, cap)
        assert np.array_equal(N.grid(pos, part, r, cap), want), r
        assert not want[~part].any() and want.max() == min(cap, want.max())
    assert 1 <= np.median(N.brute(pos, part, 0.25)[part]) <= 8  # (a median count of a few: the GPU tests' regime)


def test_grid_equals_brute_on_the_engineered_sets():
    pos, r = N.special_scene()
    part = N.participates(pos)
    want = N.brute(pos, part, r)
    assert np.array_equal(N.grid(pos, part, r), want)
    assert part.sum() == pos.shape[0] - 3 and want[10] == want[11] == 1 and not want[12:20].any()  # far pair; lone far points; non-finite
    assert (want[20:31] >= 10).all()
    lat = N.lattice()
    every = np.ones(lat.shape[0], bool)
    assert np.array_equal(N.grid(lat, every, 0.25), N.brute(lat, every, 0.25))
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    assert np.array_equal(N.grid(same, np.ones(300, bool), 0.5, 7), N.brute(same, np.ones(300, bool), 0.5, 7))


def test_brute_on_the_lattice_and_on_coincident_points():
    """what tests/test_gpu_neighbors.py expects of the device holds for the definition"""
    lat = N.lattice()
    every = np.ones(lat.shape[0], bool)
    counts = N.brute(lat, every, 0.25)
    k = np.rint(lat / F(0.25)).astype(int)
    assert np.array_equal(k.astype(F) * F(0.25), lat) and k.min() == -4 and k.max() == 4  # exact multiples, both signs
    on_faces = (np.abs(k) == 4).sum(axis=1)
    assert np.array_equal(counts, 6 - on_faces) and (counts[on_faces == 0] == 6).all()  # interior: the six at d2 == r2
    assert not N.brute(lat, every, np.nextafter(F(0.25), F(0))).any()
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    for cap in (1, 7, 299, 4095):
        c = N.brute(same, np.ones(300, bool), 0.5, cap)
        assert (c == min(299, cap)).all()
        h = N.hist(c, np.ones(300, bool), cap)
        assert h[min(299, cap)] == 300 and h.sum() == 300 and h.size == cap + 1
