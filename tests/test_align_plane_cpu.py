"""Point-to-plane registration (gsx_model_normals_keep / _kept / _reset, gsx_model_align_plane_step; spec §27) without a device: the
entry points and the structs in the header, the library, the bindings and the facades; the sums of k_nearest_align_plane and the
solve of csrc/align_plane_math.h — played by tests/align_plane_driver.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers and run as a child process — against the numpy restatement tests/align_plane_ref.py: the sums within
the derived bound of a reordered float64 sum, the solve against numpy's eigh and a pseudo-inverse at the same rank."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import align_plane_ref as P
from tests import nearest_ref as R
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCTIONS = ("gsx_model_normals_keep", "gsx_model_normals_kept", "gsx_model_normals_reset", "gsx_model_align_plane_step")
# The driver's solve against numpy (test_solve_against_numpy), measured on this file's fixtures (the corner's three seeds, the lattice,
# the sphere, the cylinder).  The worst absolute deviations were: eigenvalues 1.98e-15 of the largest (corner1); x 9.71e-17 (corner1,
# |x| 2.6e-2); pos 1.11e-16 (corner1); quat 4.86e-17 (corner1).  Asserted: 16 x the worst, the margin test_normals_cpu.py documents.
SOLVE_EIG, SOLVE_X, SOLVE_POS, SOLVE_QUAT = 16 * 1.98e-15, 16 * 9.71e-17, 16 * 1.11e-16, 16 * 4.86e-17


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"typedef struct gsx_normals_kept_t \{\s*uint32_t present; uint32_t k; uint32_t orient; uint32_t filter;[^}]*float toward\[3\]; "
                     r"uint32_t reserved;\s*uint64_t count; uint64_t n_fitted;[^}]*\} gsx_normals_kept_t; /\* 48 B \*/", hdr)
    assert re.search(r"typedef struct gsx_align_plane_desc \{\s*gsx_nearest_desc nearest;\s*uint32_t flags; float max_variation; uint32_t reserved\[2\];"
                     r"[^}]*\} gsx_align_plane_desc; /\* 96 B \*/", hdr)
    step = re.search(r"typedef struct gsx_align_plane_step_t \{(.*?)\} gsx_align_plane_step_t; /\* 568 B \*/", hdr, re.S).group(1)
    fields = re.findall(r"(double|float|uint64_t|uint32_t|gsx_nearest_stats_t) (\w+)", re.sub(r"/\*.*?\*/", "", step))
    assert [f for _, f in fields] == ["pos", "quat", "normal_matrix", "rhs", "eigenvalues", "centre", "rms_before", "rms_plane_before", "n_pairs",
                                      "n_unfitted", "xform_next", "rank", "degenerate", "nearest"]
    assert re.search(r"^gsx_status gsx_model_normals_keep\(gsx_viewer\* v, const char\* key, const gsx_normals_desc\* desc, gsx_normals_stats_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_normals_kept\(gsx_viewer\* v, const char\* key, gsx_normals_kept_t\* out, float\* out_normal /\*[^/]*\*/,\s*"
                     r"float\* out_variation /\*[^/]*\*/\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_normals_reset\(gsx_viewer\* v, const char\* key\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_align_plane_step\(gsx_viewer\* v, const char\* src_key, const char\* dst_key, const gsx_align_plane_desc\* desc,\s*"
                     r"gsx_align_plane_step_t\* out\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    spec = _read("spec", "RENDER_SPEC.md")
    assert "§27" in hdr and "## 27. Point-to-plane registration [BUILD-SPEC]" in spec
    s27 = spec.split("## 27. Point-to-plane registration [BUILD-SPEC]")[1]
    for word in ("symmetric", "source-normal", "robust weights", "scale", "select_normals", "depth map", "sharded", "fuzz", "sign of"):
        assert word in s27, word
    # the neighbouring structs keep their sizes: nothing was added to them
    assert (C.sizeof(_lib.NormalsDesc), C.sizeof(_lib.AlignDesc), C.sizeof(_lib.AlignStep), C.sizeof(_lib.NearestDesc)) == (48, 88, 272, 80)


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.NormalsKept) == 48
    assert offsets(_lib.NormalsKept) == {"present": 0, "k": 4, "orient": 8, "filter": 12, "toward": 16, "reserved": 28, "count": 32, "n_fitted": 40}
    assert C.sizeof(_lib.AlignPlaneDesc) == 96 and offsets(_lib.AlignPlaneDesc) == {"nearest": 0, "flags": 80, "max_variation": 84, "reserved": 88}
    assert C.sizeof(_lib.AlignPlaneStep) == 568
    assert offsets(_lib.AlignPlaneStep) == {"pos": 0, "quat": 24, "normal_matrix": 56, "rhs": 224, "eigenvalues": 272, "centre": 320, "rms_before": 344,
                                            "rms_plane_before": 352, "n_pairs": 360, "n_unfitted": 368, "xform_next": 376, "rank": 424, "degenerate": 428,
                                            "nearest": 432}
    assert "static_assert(sizeof(gsx_align_plane_desc) == 96 && sizeof(gsx_align_plane_step_t) == 568" in _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_nearest.cpp")
    assert "static_assert(sizeof(gsx_normals_kept_t) == 48" in _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_normals.cpp")


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_normals_kept_t", "gsx_align_plane_desc", "gsx_align_plane_step_t"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub normal_matrix: [f64; 21]" in rust_sys
    for method in ("keep_normals", "kept_normals", "reset_normals", "align_plane_step"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    # without a device: a status code and a message, not a crash
    nd = _lib.NormalsDesc()
    L.gsx_normals_desc_default(C.byref(nd))
    assert L.gsx_model_normals_keep(None, b"a", C.byref(nd), C.byref(_lib.NormalsStats())) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_normals_keep" in L.gsx_last_error_string()
    assert L.gsx_model_normals_kept(None, b"a", C.byref(_lib.NormalsKept()), None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_normals_kept" in L.gsx_last_error_string()
    assert L.gsx_model_normals_reset(None, b"a") == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_normals_reset" in L.gsx_last_error_string()
    d = _lib.NearestDesc()
    L.gsx_nearest_desc_default(C.byref(d))
    desc = _lib.AlignPlaneDesc(d, 0, 0.0, (C.c_uint32 * 2)(0, 0))
    assert L.gsx_model_align_plane_step(None, b"a", b"b", C.byref(desc), C.byref(_lib.AlignPlaneStep())) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_align_plane_step" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("keep_normals", "kept_normals", "reset_normals", "align_plane_step", "align"))


def test_the_rules_have_one_copy_and_the_build_lists_the_sources():
    kernels, api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_nearest.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_nearest.cpp")
    plane_h, align_h, driver = (_read("wgpu_3dgs_viewer_app_amd", "csrc", "align_plane_math.h"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "align_math.h"),
                                _read("tests", "align_plane_driver.cpp"))
    for text in (api, driver):
        assert '#include "align_plane_math.h"' in text
        for rule in ("inline AlignPlaneDelta align_plane_solve(", "inline double align_plane_centre(", "inline void align_jacobi("):
            assert rule not in text
    assert plane_h.count("inline AlignPlaneDelta align_plane_solve(") == 1 and plane_h.count("inline double align_plane_centre(") == 1
    body = plane_h.split("#pragma once")[1]
    assert "hip" not in body.lower() and '#include "align_math.h"' in body and "align_jacobi<6>(" in body
    # the rotation's arithmetic has one copy: align_math.h's, which its own 4x4 solve calls too
    assert align_h.count("inline void align_jacobi(") == 1 and "align_jacobi<4>(" in align_h and "theta" not in body and align_h.count("const double theta") == 1
    assert "kAlignPlaneRank = kAlignGap" in plane_h
    # the search and the normals are reused, not copied: one run_nearest, one run_normals, one place where a plane is adopted
    normals_api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_normals.cpp")
    assert api.count("gsx_status run_nearest(") == 1 and api.count("run_nearest(v, src, dst") == 4
    assert normals_api.count("gsx_status run_normals(") == 1 and normals_api.count("gsx_status normals_call(") == 1 and normals_api.count("normals_call(v, ") == 2
    assert "__global__ __launch_bounds__(256) void k_nearest_align_plane(" in kernels and "kAlignPlanePartialDoubles" in kernels
    # the plane step's partials are its own: the workspace of the three older calls is what it was
    assert "constexpr uint32_t kNearestPartialDoubles = 16;" in _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_internal.h")
    state = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_state.h")
    assert state.count("inline void drop_normals(Model* m)") == 1
    # dropped where the visibility planes are dropped, but for the visibility's own reset
    for name in ("gsx_api.cpp", "gsx_api_import.cpp", "gsx_api_transform.cpp", "gsx_api_visibility.cpp"):
        text = _read("wgpu_3dgs_viewer_app_amd", "csrc", name)
        assert text.count("drop_normals(m);") == (0 if name == "gsx_api_visibility.cpp" else text.count("drop_visibility(m);")), name
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_nearest.hip" in makefile and "$(wildcard *.h)" in makefile and "-ffp-contract=off" in makefile


# ---- 2. the driver ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_plane") / "align_plane_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "align_plane_driver.cpp"), "-o", exe])
    return exe


def _hex(a):
    return " ".join(f"{w:x}" for w in np.ascontiguousarray(a, F).reshape(-1).view(np.uint32))


def _f64(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)


def _parse_solve(w):
    assert w[0] == "solve"
    d = _f64(w[3:25])
    return dict(rank=int(w[1]), degenerate=bool(int(w[2])), pos=d[0:3], quat=d[3:7], eigenvalues=d[7:13], centre=d[13:16], x=d[16:22],
                xform_next=np.array([int(x, 16) for x in w[25:37]], np.uint32).view(F).reshape(3, 4))


def play_step(driver, q, t, n, variation, max_variation=0.0, xform=P.IDENTITY):
    """(sums, solve) of the driver over the found pairs' rows"""
    q, t, n = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (q, t, n))
    rows = np.concatenate([q, t, n, np.ascontiguousarray(variation, F).reshape(-1, 1)], axis=1) if len(q) else np.zeros((0, 10), F)
    text = f"step {_hex(F(max_variation))} {_hex(xform)} {len(rows):x} {_hex(rows)}".rstrip() + "\n"
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    a, b = [ln.split() for ln in r.stdout.splitlines()]
    assert a[0] == "sums"
    d = _f64(a[3:])
    sums = dict(n_pairs=int(a[1]), n_unfitted=int(a[2]), sum_q=d[0:3], centre=d[3:6], A21=d[6:27], b=d[27:33], sum_e2=d[33], sum_d2=d[34],
                rms_before=d[35], rms_plane_before=d[36], raw=a)
    return sums, _parse_solve(b)


def _driver_step(driver, src, xform, targets, normals, variation):
    q = R.map_points(xform, src)
    index, _ = P.nearest(q, targets)
    return play_step(driver, q, targets[index], normals[index], variation[index], xform=xform)


def assert_sums_within_bound(got, ref):
    """The reference takes every term as the code under test does, in float64 from the same float32 values, and sums them exactly
    (math.fsum); the code under test adds the same m terms in some order.  So |got - ref| <= (m + 4) 2^-53 sum|term| (align_plane_ref
    .bound: m - 1 roundings of partial sums that sum|term| bounds, and slack for the second order and the reference's own rounding),
    with sum|term| from the reference.  Derived, not measured."""
    m = ref["n_pairs"]
    assert got["n_pairs"] == m and got["n_unfitted"] == ref["n_unfitted"]
    assert np.array_equal(got["centre"], ref["centre"])  # (sum q is within the bound, and the fixtures' quotients do not sit on a float32 tie)
    for key in ("A21", "b", "sum_e2", "sum_d2"):
        err, lim = np.abs(np.asarray(got[key]) - np.asarray(ref[key])), P.bound(m, ref["mag"][key])
        assert np.all(err <= lim), (key, err, lim)
    if "sum_q" in got:
        assert np.all(np.abs(got["sum_q"] - ref["sum_q"]) <= P.bound(m, ref["mag"]["sum_q"]))
    for key, s in (("rms_before", "sum_d2"), ("rms_plane_before", "sum_e2")):  # sqrt(s / m): half the sum's relative bound, and two roundings
        lim = ref[key] * (0.5 * (m + 4) * 2.0 ** -53 * ref["mag"][s] / ref[s] + 2.0 ** -51) if ref[s] else 0.0
        assert abs(got[key] - ref[key]) <= lim, key


@pytest.fixture(scope="module")
def fixtures():
    """name -> (source, targets, normals, variation), made once and not changed"""
    out = {}
    for seed in range(3):
        targets, src, truth = P.corner(seed)
        nrm, var = P.fitted_normals(targets)
        out[f"corner{seed}"] = (src, targets, nrm, var, truth)
    pos, nrm, var = P.lattice()
    out["lattice"] = (P.lattice_source(pos), pos, nrm, var, None)
    for name, f in (("sphere", P.sphere()), ("cylinder", P.cylinder())):
        out[name] = (f[3], f[0], f[1], f[2], None)
    return out


def test_sums_against_the_reference(driver, fixtures):
    for name, (src, targets, nrm, var, _) in fixtures.items():
        index, _ = P.nearest(src, targets)
        got, _ = play_step(driver, src, targets[index], nrm[index], var[index])
        ref = P.sums(src, targets[index], nrm[index], var[index])
        assert ref["n_pairs"] == len(src), name
        assert_sums_within_bound(got, ref)


def solve_deviation(got, ref):
    """(eigenvalues over the largest, x, pos, quat) absolute deviations and |x| of the reference"""
    return (np.abs(got["eigenvalues"] - ref["eigenvalues"]).max() / ref["eigenvalues"][0], np.abs(got["x"] - ref["x"]).max(),
            np.abs(got["pos"] - ref["pos"]).max(), np.abs(got["quat"] - ref["quat"]).max(), np.abs(ref["x"]).max())


def test_solve_against_numpy(driver, fixtures):
    ranks = dict(corner0=6, corner1=6, corner2=6, lattice=3, sphere=3, cylinder=4)
    for name, (src, targets, nrm, var, _) in fixtures.items():
        s, got = _driver_step(driver, src, P.IDENTITY, targets, nrm, var)
        assert got["rank"] == ranks[name] and not got["degenerate"], name  # exact
        ref = P.solve(s["A21"], s["b"], s["centre"], rank=got["rank"])
        assert ref["rank"] == P.solve(s["A21"], s["b"], s["centre"])["rank"]  # numpy's eigenvalues count the same
        eig, x, pos, quat, size = solve_deviation(got, ref)
        print(f"{name}: eig {eig:.2e} x {x:.2e} pos {pos:.2e} quat {quat:.2e} |x| {size:.2e}")
        assert eig <= SOLVE_EIG and x <= SOLVE_X and pos <= SOLVE_POS and quat <= SOLVE_QUAT, name
        assert np.all(np.diff(got["eigenvalues"]) <= 0) and np.array_equal(got["centre"], s["centre"])
        assert abs(np.linalg.norm(got["quat"]) - 1) <= 4e-16 and got["quat"][3] >= 0
        want = P.compose34(P.matrix34(dict(R=R.quat_rows(got["quat"]), pos=got["pos"])), P.IDENTITY).astype(F)
        assert np.array_equal(got["xform_next"].view(np.uint32), want.view(np.uint32))  # composed in double, rounded once


def test_the_sliding_plane(driver, fixtures):
    """A floor against a floor: the pairs determine the lift and the two tilts, and the step moves along nothing else"""
    src, targets, nrm, var, _ = fixtures["lattice"]
    x, s, d = P.plane_step_numpy(src, P.IDENTITY, targets, nrm, var)  # numpy
    assert d["rank"] == 3 and s["n_pairs"] == 800 and abs(d["eigenvalues"][0] - 800) < 1e-9 and np.all(np.abs(d["eigenvalues"][3:]) < 1e-12)
    assert np.abs(d["pos"] - [0, 0, -0.05]).max() <= SOLVE_POS + 1e-9 and np.abs(d["quat"] - [0, 0, 0, 1]).max() <= 1e-15
    # (1e-9: the lift is fl32(0.05), 7.5e-10 from 0.05)
    s, got = _driver_step(driver, src, P.IDENTITY, targets, nrm, var)  # the library's header
    assert got["rank"] == 3 and np.all(got["eigenvalues"][3:] == 0.0)
    assert got["x"][2] == 0.0 and got["x"][3] == 0.0 and got["x"][4] == 0.0  # exactly: no turn in the plane, no slide along it
    assert np.abs(got["pos"] - [0, 0, -float(F(0.05))]).max() <= SOLVE_POS and np.abs(got["pos"][:2]).max() <= 1e-15
    assert np.abs(got["quat"] - [0, 0, 0, 1]).max() <= 1e-15


def _error(xform, truth):
    return float(np.abs(np.asarray(xform, np.float64) - truth).max())


def test_four_plane_steps_beat_twelve_point_steps(driver, fixtures):
    for seed in range(3):
        src, targets, nrm, var, truth = fixtures[f"corner{seed}"]
        x = P.IDENTITY
        for _ in range(4):
            x = _driver_step(driver, src, x, targets, nrm, var)[1]["xform_next"]
        y = P.IDENTITY
        for _ in range(12):
            y = P.point_step_numpy(src, y, targets)
        print(f"seed {seed}: plane {_error(x, truth):.2e} point {_error(y, truth):.2e}")
        assert _error(x, truth) < _error(y, truth)


def test_degenerate_inputs(driver, fixtures):
    src, targets, nrm, var, _ = fixtures["corner0"]
    index, _ = P.nearest(src, targets)
    t, n, v = targets[index], nrm[index], var[index]
    xf = F([[1, 0, 0, 0.5], [0, 1, 0, 0.25], [0, 0, 1, -1]])
    for m in (0, 1, 2):
        s, got = play_step(driver, src[:m], t[:m], n[:m], v[:m], xform=xf)
        assert s["n_pairs"] == m and got["degenerate"] and np.array_equal(got["pos"], [0, 0, 0]) and np.array_equal(got["quat"], [0, 0, 0, 1])
        assert np.array_equal(got["xform_next"], xf)
        assert_sums_within_bound(s, P.sums(src[:m], t[:m], n[:m], v[:m]))
    assert got["rank"] == 2  # (two pairs span two directions; fewer than 3 pairs is degenerate whatever the rank)
    s, got = play_step(driver, src, t, np.zeros_like(n), np.full(len(src), np.inf, F))  # nobody fitted
    assert (s["n_pairs"], s["n_unfitted"]) == (0, len(src)) and got["degenerate"] and got["rank"] == 0 and not s["A21"].any()
    cut = float(np.median(v))
    s, got = play_step(driver, src, t, n, v, max_variation=cut)
    ref = P.sums(src, t, n, v, max_variation=cut)
    assert 0 < ref["n_unfitted"] < len(src) and ref["n_unfitted"] == int((v > F(cut)).sum())
    assert_sums_within_bound(s, ref)
    some = v.copy()
    some[::7] = np.inf  # unfitted rows among the fitted
    s, _ = play_step(driver, src, t, n, some)
    assert_sums_within_bound(s, P.sums(src, t, n, some))
    # the sign of a normal changes nothing: J and e both change sign, every term is a product of two of them
    flipped = n.copy()
    flipped[::3] *= F(-1)
    a, ga = play_step(driver, src, t, n, v)
    b, gb = play_step(driver, src, t, flipped, v)
    assert a["raw"] == b["raw"] and np.array_equal(ga["xform_next"], gb["xform_next"]) and np.array_equal(ga["pos"], gb["pos"])
