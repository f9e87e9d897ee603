"""Model clusters (gsx_model_clusters, gsx_model_select_clusters; spec §19) without a device: the entry points and the structs in the
header, the library, the bindings and the facades; the union-find of csrc/clusters_math.h — played by tests/clusters_driver.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process, on 16 threads — against the
numpy restatement tests/clusters_ref.py; and the restatement's expectations on the engineered sets the GPU tests use."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import clusters_ref as K
from tests import neighbors_ref as N
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCTIONS = ("gsx_cluster_desc_default", "gsx_model_clusters", "gsx_model_select_clusters")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^#define GSX_CLUSTER_NONE 0xFFFFFFFFu", hdr, re.M) and _lib.GSX_CLUSTER_NONE == 0xFFFFFFFF == K.NONE
    for name, value in (("BY_SIZE", 0), ("LARGEST", 1), ("SEEDED", 2)):
        assert re.search(rf"^#define GSX_CLUSTER_{name} {value}u", hdr, re.M) and getattr(_lib, "GSX_CLUSTER_" + name) == value == getattr(K, name)
    assert re.search(r"typedef struct gsx_cluster_desc \{ uint32_t filter; uint32_t flags; float radius; uint32_t grid_bits; uint32_t reserved\[2\]; \} "
                     r"gsx_cluster_desc;", hdr)
    assert re.search(r"typedef struct gsx_cluster_stats_t \{\s*uint64_t count; uint64_t n_nonfinite; uint64_t n_clusters; uint64_t largest_size; "
                     r"uint32_t largest_label; uint32_t grid_bits;\s*\} gsx_cluster_stats_t;", hdr)
    assert re.search(r"typedef struct gsx_cluster_select_desc \{\s*uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t mode;[^}]*"
                     r"float radius; uint32_t size_lo; uint32_t size_hi; uint32_t grid_bits; uint32_t reserved\[2\];\s*\} gsx_cluster_select_desc;", hdr)
    assert re.search(r"^void gsx_cluster_desc_default\(gsx_cluster_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_clusters\(gsx_viewer\* v, const char\* key, const gsx_cluster_desc\* desc, uint32_t\* out_labels, "
                     r"uint32_t\* out_sizes, gsx_cluster_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_clusters\(gsx_viewer\* v, const char\* key, const gsx_cluster_select_desc\* desc, "
                     r"uint64_t\* out_hit, uint64_t\* out_selected\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    assert (K.SET, K.ADD, K.REMOVE) == (_lib.GSX_SELECTION_SET, _lib.GSX_SELECTION_ADD, _lib.GSX_SELECTION_REMOVE)


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.ClusterDesc) == 24
    assert offsets(_lib.ClusterDesc) == {"filter": 0, "flags": 4, "radius": 8, "grid_bits": 12, "reserved": 16}
    assert C.sizeof(_lib.ClusterStats) == 40
    assert offsets(_lib.ClusterStats) == {"count": 0, "n_nonfinite": 8, "n_clusters": 16, "largest_size": 24, "largest_label": 32, "grid_bits": 36}
    assert C.sizeof(_lib.ClusterSelectDesc) == 40
    assert offsets(_lib.ClusterSelectDesc) == {"filter": 0, "flags": 4, "selection_op": 8, "mode": 12, "radius": 16, "size_lo": 20, "size_hi": 24,
                                               "grid_bits": 28, "reserved": 32}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_clusters.cpp")
    assert "static_assert(sizeof(gsx_cluster_desc) == 24 && sizeof(gsx_cluster_stats_t) == 40 && sizeof(gsx_cluster_select_desc) == 40" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    for fn in FUNCTIONS[1:]:
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_cluster_desc", "gsx_cluster_stats_t", "gsx_cluster_select_desc"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub const GSX_CLUSTER_NONE: u32 = 0xFFFF_FFFF;" in rust_sys and "pub const GSX_CLUSTER_SEEDED: u32 = 2;" in rust_sys
    for method in ("clusters", "select_clusters"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    d = _lib.ClusterDesc(7, 7, 7.0, 7, (C.c_uint32 * 2)(7, 7))
    L.gsx_cluster_desc_default(C.byref(d))
    assert (d.filter, d.flags, d.radius, d.grid_bits, tuple(d.reserved)) == (0, 0, 1.0, 0, (0, 0))
    L.gsx_cluster_desc_default(None)
    # without a device: a status code and a message, not a crash
    labels, sizes, stats = (C.c_uint32 * 4)(), (C.c_uint32 * 4)(), _lib.ClusterStats()
    sd = _lib.ClusterSelectDesc(0, 0, 0, K.LARGEST, 1.0, 0, 0, 0)
    assert L.gsx_model_clusters(None, b"a", C.byref(d), labels, sizes, C.byref(stats)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_clusters" in L.gsx_last_error_string()
    assert L.gsx_model_select_clusters(None, b"a", C.byref(sd), None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_clusters" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("clusters", "select_clusters"))


def test_find_and_union_have_one_copy_and_the_build_lists_the_sources():
    kernels, api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_clusters.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_clusters.cpp")
    math_h, driver = _read("wgpu_3dgs_viewer_app_amd", "csrc", "clusters_math.h"), _read("tests", "clusters_driver.cpp")
    for text in (kernels, api, driver):
        assert '#include "clusters_math.h"' in text and "cl_find(P&" not in text and "cl_union(P&" not in text
    assert math_h.count("inline uint32_t cl_find(P& p") == 1 and math_h.count("inline void cl_union(P& p") == 1
    assert "cl_union(" in kernels and "cl_find(" in kernels and "cl_union(" in driver
    # the grid is section 18's: its passes are called, its kernels and its cell function are not restated
    assert "enqueue_grid(" in api and "enqueue_grid(" in _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_neighbors.cpp")
    assert '#include "neighbors_math.h"' in kernels and "inline uint32_t nb_cell(" not in kernels
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_clusters.hip" in makefile and "gsx_api_clusters.cpp" in makefile and "-ffp-contract=off" in makefile


# ---- 2. csrc/clusters_math.h: the driver, 16 threads ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("clusters") / "clusters_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "clusters_driver.cpp"), "-o", exe])
    return exe


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def test_threads_on_random_edge_lists_agree_with_the_restatement(driver):
    """the labels 16 threads leave are the restatement's, whatever the order of their compare-and-swaps"""
    rng = np.random.default_rng(3)
    text, want = "", []
    for n, m in ((1, 0), (2, 1), (50, 20), (1000, 400), (1000, 3000), (20000, 15000), (20000, 40000)):
        e = rng.integers(0, n, (m, 2))
        text += f"edges {n} {' '.join(str(x) for x in e.reshape(-1))}\n"
        want.append(K.components(n, np.ones(n, bool), e[:, 0], e[:, 1])[0])
    out = _play(driver, text)
    assert len(out) == len(want)
    for ln, labels in zip(out, want):
        assert ln[0] == "edges" and ln[1] == "0"  # parent[i] <= i, no cycle, roots = the driver's own breadth-first search
        assert np.array_equal(np.array(ln[2:], np.int64), labels.astype(np.int64))
    # the driver's own lists, larger
    out = _play(driver, "random 1 100000 50000\nrandom 2 100000 200000\nrandom 3 300000 299999\n")
    assert [ln[:2] for ln in out] == [["random", "0"]] * 3 and int(out[0][2]) > 50000 > int(out[1][2]) > 1


def test_threads_on_a_shuffled_chain_and_a_star(driver):
    out = _play(driver, "chain 1 65536\nchain 2 65536\nstar 65537 0\nstar 65537 65536\nstar 65537 30000\nchain 3 1\n")
    assert out[0] == out[1] == ["chain", "0", "1", "65537"]  # 65 536 edges: one cluster, its root the smallest index
    assert out[2] == out[3] == out[4] == ["star", "0", "1", "65537"]
    assert out[5] == ["chain", "0", "1", "2"]


# ---- 3. the restatement on the engineered sets of tests/test_gpu_clusters.py -----------------------------------------------------------
def test_restatement_on_a_random_scene_against_the_neighbour_counts():
    rng = np.random.default_rng(1)
    n = 3000
    pos = rng.standard_normal((n, 3)).astype(F)
    part = rng.random(n) < 0.8
    c = K.clusters(pos, part, 0.2)
    counts = N.brute(pos, part, 0.2)
    assert np.array_equal(c.sizes == 1, part & (counts == 0))  # a singleton has no neighbour
    assert (c.labels[~part] == K.NONE).all() and not c.sizes[~part].any()
    assert (c.labels[part] <= np.nonzero(part)[0]).all() and c.count == part.sum()
    roots = np.nonzero(c.labels == np.arange(n))[0]
    assert c.n_clusters == roots.size and c.sizes[roots].sum() == c.count and c.largest_size == c.sizes.max() > 2
    ei, ej = K.edges(pos, part, 0.2)
    assert ei.size == counts.sum() // 2 and np.array_equal(c.labels[ei], c.labels[ej])
    gi, gj = K.grid_edges(pos, part, 0.2)  # the sorted-cell version finds the same pairs
    assert np.array_equal(np.unique(gi * n + gj), np.unique(ei * n + ej)) and gi.size == ei.size
    assert np.array_equal(c.sizes[part], np.bincount(c.labels[part], minlength=n)[c.labels[part]])
    # the hit sets
    assert K.hits(c, K.BY_SIZE, 1, n).sum() == c.count and K.hits(c, K.LARGEST).sum() == c.largest_size
    assert np.array_equal(K.hits(c, K.BY_SIZE, 1, 1), c.sizes == 1)
    seeds = np.zeros(n, bool)
    seeds[[int(c.largest_label), int(np.nonzero(~part)[0][0])]] = True  # one in the largest cluster, one that does not participate
    assert np.array_equal(K.hits(c, K.SEEDED, seeds=seeds), K.hits(c, K.LARGEST)) and not K.hits(c, K.SEEDED).any()


def test_restatement_on_the_chain():
    pos, k = K.chain()
    every = np.ones(4096, bool)
    assert np.array_equal(pos[:, 0], (k * 0.5).astype(F)) and sorted(k) == list(range(4096))
    one = K.clusters(pos, every, 0.5)
    assert (one.n_clusters, one.largest_size, one.largest_label) == (1, 4096, 0) and not one.labels.any()
    apart = K.clusters(pos, every, np.nextafter(F(0.5), F(0)))
    assert apart.n_clusters == 4096 and np.array_equal(apart.labels, np.arange(4096)) and (apart.sizes == 1).all() and apart.largest_label == 0
    pos2, k2 = K.chain(split=True)
    two = K.clusters(pos2, every, 0.5)
    low, high = np.nonzero(k2 < 2048)[0], np.nonzero(k2 >= 2048)[0]
    assert two.n_clusters == 2 and (two.sizes == 2048).all() and two.largest_label == 0
    assert (two.labels[low] == low.min()).all() and (two.labels[high] == high.min()).all()
    far, kf = K.chain(70000, 12)  # exact in float32, and past the cell clamp: 35 000 / (0.5 * 33 / 32) > 32 767 cells
    assert np.array_equal(far[:, 0].astype(np.float64), kf * 0.5) and far[:, 0].max() / N.grid_of(0.5)[1] > N.MAX_CELL + 2


def test_restatement_on_lattice_coincident_special_and_bridge():
    lat = N.lattice()
    every = np.ones(lat.shape[0], bool)
    c = K.clusters(lat, every, 0.25)
    assert (c.n_clusters, c.largest_size, c.largest_label) == (1, 729, 0)
    assert K.clusters(lat, every, np.nextafter(F(0.25), F(0))).n_clusters == 729
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    c = K.clusters(same, np.ones(300, bool), 0.5)
    assert (c.n_clusters, c.largest_size) == (1, 300) and not c.labels.any()
    pos, r = N.special_scene(3000)
    part = N.participates(pos)
    c = K.clusters(pos, part, r)
    assert c.labels[10] == c.labels[11] == 10 and c.sizes[10] == c.sizes[11] == 2            # the coincident far pair
    assert np.array_equal(c.labels[12:17], np.arange(12, 17)) and (c.sizes[12:17] == 1).all()  # lone far points
    assert (c.labels[17:20] == K.NONE).all() and not c.sizes[17:20].any() and c.count == 2997
    assert (c.labels[20:31] == c.labels[20]).all() and c.sizes[20] >= 11
    # a bridge: the filter decides connectivity, not only membership
    pos, at = K.bridge()
    every = np.ones(55, bool)
    c = K.clusters(pos, every, 0.25)
    assert (c.n_clusters, c.largest_size) == (1, 55)
    c = K.clusters(pos, every & (np.arange(55) != at), 0.25)
    assert c.n_clusters == 2 and sorted(set(c.sizes.tolist())) == [0, 27] and c.labels[at] == K.NONE
    assert c.largest_label == c.labels[c.labels != K.NONE].min()  # a tie: the smallest label
