"""The model plane (gsx_model_fit_plane, gsx_model_select_plane, gsx_plane_level; spec §28) without a device: the entry points and the
structs in the header, the library, the bindings and the facades; one copy of every rule; csrc/plane_math.h — played by
tests/plane_driver.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process —
against the numpy restatement tests/plane_ref.py: the hash and the sampled indices equal, the candidates bit for bit (the reference
takes the same IEEE operations in the same order; the triple's quotient is one division and one rounding on both sides), the counts
equal, the moments within the derived bound of a reordered float64 sum, the solve against numpy's eigh; gsx_plane_level; and the
issue's experiment: three successive fits peel the three faces of a noisy corner."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import plane_ref as PR
from wgpu_3dgs_viewer_app_amd import _lib
from wgpu_3dgs_viewer_app_amd.viewer import plane_level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCTIONS = ("gsx_plane_fit_desc_default", "gsx_plane_select_desc_default", "gsx_model_fit_plane", "gsx_model_select_plane", "gsx_plane_level")
# The driver's solve against numpy's eigh (test_solve_against_numpy), measured on this file's fixtures: the inliers of the winning
# candidate and of the once-refined plane of the corner's three seeds in both sample modes, and of the tilted lattice, each with three
# sign rules.  The worst deviations were: normal 0 and offset 0 (the same float32 bits on every fixture), eigenvalues 7.73e-16 of the
# largest.  Asserted: 16 x the worst, the margin test_normals_cpu.py documents — for the normal and the offset that is 0: the float32
# bits of the two solvers' planes are equal on these fixtures, and the test says so.
SOLVE_NORMAL, SOLVE_OFFSET, SOLVE_EIG = 16 * 0.0, 16 * 0.0, 16 * 7.73e-16
# gsx_plane_level: the rotated unit normal against up / |up|, in units of 2^-52 (an ulp of a component near 1): asserted 4, measured
# below that on every case of test_level.
LEVEL_ULPS = 4


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- 1. header, layout, exports ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"typedef struct gsx_plane_t \{ float normal\[3\]; float offset; \} gsx_plane_t; /\* 16 B", hdr)
    for name, value in (("GSX_PLANE_MAX_CANDIDATES", "1024u"), ("GSX_PLANE_SAMPLE_TRIPLES", "0u"), ("GSX_PLANE_SAMPLE_NORMALS", "1u"), ("GSX_PLANE_SAMPLE_CALLER", "2u"),
                        ("GSX_PLANE_MAX_REFINE", "8u"), ("GSX_PLANE_NONE", "0xFFFFFFFFu")):
        assert re.search(rf"^#define {name}\s+{value}", hdr, re.M), name
    desc = re.search(r"typedef struct gsx_plane_fit_desc \{(.*?)\} gsx_plane_fit_desc; /\* 64 B \*/", hdr, re.S).group(1)
    fields = [f for _, f in re.findall(r"(float|uint64_t|uint32_t) (\w+)", re.sub(r"/\*.*?\*/", "", desc, flags=re.S))]
    assert fields == ["filter", "flags", "sample", "n_candidates", "seed", "tolerance", "min_cos", "refine_iters", "orient", "toward", "reserved"]
    fit = re.search(r"typedef struct gsx_plane_fit_t \{(.*?)\} gsx_plane_fit_t; /\* 208 B \*/", hdr, re.S).group(1)
    fields = [f for _, f in re.findall(r"(double|float|uint64_t|uint32_t|gsx_plane_t) (\w+)", re.sub(r"/\*.*?\*/", "", fit, flags=re.S))]
    assert fields == ["plane", "candidate", "winner", "n_valid", "count", "n_nonfinite", "candidate_inliers", "n_inliers", "centroid", "refine_done",
                      "eigenvalues", "rms", "sums", "degenerate", "reserved"]
    sel = re.search(r"typedef struct gsx_plane_select_desc \{(.*?)\} gsx_plane_select_desc; /\* 48 B \*/", hdr, re.S).group(1)
    fields = [f for _, f in re.findall(r"(float|uint32_t|gsx_plane_t) (\w+)", sel)]
    assert fields == ["plane", "lo", "hi", "min_cos", "filter", "selection_op", "reserved"]
    assert re.search(r"^gsx_status gsx_model_fit_plane\(gsx_viewer\* v, const char\* key, const gsx_plane_fit_desc\* desc, const gsx_plane_t\* candidates[^;]*"
                     r"gsx_plane_t\* out_candidates[^;]*uint32_t\* out_counts[^;]*gsx_plane_fit_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_plane\(gsx_viewer\* v, const char\* key, const gsx_plane_select_desc\* desc, uint64_t\* out_hit, "
                     r"uint64_t\* out_selected\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_plane_level\(const gsx_plane_t\* plane, const float up\[3\], float quat_xyzw\[4\], float pos\[3\]\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays
    spec = _read("spec", "RENDER_SPEC.md")
    assert "§28" in hdr and "## 28. Model plane [BUILD-SPEC]" in spec
    s28 = spec.split("## 28. Model plane [BUILD-SPEC]")[1]
    for word in ("splitmix64", "inclusive", "NOT normalised", "ties", "antiparallel", "SELECTED", "World-space", "Several planes", "opacity", "Cylinders",
                 "sharded", "fuzz"):
        assert word in s28, word
    design = _read("DESIGN.md")
    assert "### Model plane" in design
    for word in ("k_plane_score", "VGPR", "scratch", "World-space planes", "cylinders"):
        assert word in design.split("### Model plane")[1], word
    for recipe in ("Level a capture", "Remove the floor", "Peel the next plane"):
        assert recipe in hdr and recipe in _read("README.md"), recipe
    assert "gsx_model_fit_plane" in _read("INTEGRATION.md") and "r29_bench_plane.txt" in _read("profiles", "README.md")
    # the neighbouring structs keep their sizes: nothing was added to them
    assert (C.sizeof(_lib.NormalsDesc), C.sizeof(_lib.NormalsSelectDesc), C.sizeof(_lib.AlignPlaneDesc), C.sizeof(_lib.AlignPlaneStep)) == (48, 80, 96, 568)


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.Plane) == 16 and offsets(_lib.Plane) == {"normal": 0, "offset": 12}
    assert C.sizeof(_lib.PlaneFitDesc) == 64
    assert offsets(_lib.PlaneFitDesc) == {"filter": 0, "flags": 4, "sample": 8, "n_candidates": 12, "seed": 16, "tolerance": 24, "min_cos": 28,
                                          "refine_iters": 32, "orient": 36, "toward": 40, "reserved": 52}
    assert C.sizeof(_lib.PlaneFit) == 208
    assert offsets(_lib.PlaneFit) == {"plane": 0, "candidate": 16, "winner": 32, "n_valid": 36, "count": 40, "n_nonfinite": 48, "candidate_inliers": 56,
                                      "n_inliers": 64, "centroid": 72, "refine_done": 84, "eigenvalues": 88, "rms": 112, "sums": 120, "degenerate": 200,
                                      "reserved": 204}
    assert C.sizeof(_lib.PlaneSelectDesc) == 48
    assert offsets(_lib.PlaneSelectDesc) == {"plane": 0, "lo": 16, "hi": 20, "min_cos": 24, "filter": 28, "selection_op": 32, "reserved": 36}
    assert ("static_assert(sizeof(gsx_plane_t) == 16 && sizeof(gsx_plane_fit_desc) == 64 && sizeof(gsx_plane_fit_t) == 208 && sizeof(gsx_plane_select_desc) == 48"
            in _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_plane.cpp"))
    assert (_lib.GSX_PLANE_SAMPLE_TRIPLES, _lib.GSX_PLANE_SAMPLE_NORMALS, _lib.GSX_PLANE_SAMPLE_CALLER) == (PR.TRIPLES, PR.NORMALS, PR.CALLER) == (0, 1, 2)
    assert (_lib.GSX_PLANE_MAX_CANDIDATES, _lib.GSX_PLANE_MAX_REFINE, _lib.GSX_PLANE_NONE) == (1024, 8, PR.NONE)


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCTIONS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_plane_t", "gsx_plane_fit_desc", "gsx_plane_fit_t", "gsx_plane_select_desc"):
        assert "pub struct " + s + " " in rust_sys
    assert "pub sums: [f64; 10]" in rust_sys and "pub const GSX_PLANE_MAX_CANDIDATES: u32 = 1024;" in rust_sys
    for method in ("fit_plane", "select_plane", "plane_level"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    # the defaults
    d = _lib.PlaneFitDesc()
    L.gsx_plane_fit_desc_default(C.byref(d))
    assert (d.filter, d.flags, d.sample, d.n_candidates, d.seed, d.tolerance, d.min_cos, d.refine_iters, d.orient) == (0, 0, 0, 256, 0, 0.0, 0.0, 2, 0)
    assert list(d.toward) == [0, 0, 0] and list(d.reserved) == [0, 0, 0]
    s = _lib.PlaneSelectDesc()
    L.gsx_plane_select_desc_default(C.byref(s))
    assert (list(s.plane.normal), s.plane.offset, s.lo, s.hi, s.min_cos, s.filter, s.selection_op, list(s.reserved)) == ([0, 0, 1], 0, 0, 0, 0, 0, 0, [0, 0, 0])
    L.gsx_plane_fit_desc_default(None)
    L.gsx_plane_select_desc_default(None)
    # without a device: a status code and a message, not a crash
    assert L.gsx_model_fit_plane(None, b"a", C.byref(d), None, None, None, C.byref(_lib.PlaneFit())) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_fit_plane" in L.gsx_last_error_string()
    assert L.gsx_model_select_plane(None, b"a", C.byref(s), None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_plane" in L.gsx_last_error_string()
    assert L.gsx_plane_level(None, None, None, None) == _lib.GSX_ERR_INVALID_ARG and b"gsx_plane_level" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("fit_plane", "select_plane")) and callable(plane_level)


def test_the_rules_have_one_copy_and_the_build_lists_the_sources():
    kernels, api, header, driver = (_read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_plane.hip"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_plane.cpp"),
                                    _read("wgpu_3dgs_viewer_app_amd", "csrc", "plane_math.h"), _read("tests", "plane_driver.cpp"))
    rules = ("inline uint64_t pl_mix(", "inline uint32_t pl_probe(", "inline float pl_residual(", "inline bool pl_inlier(", "inline bool pl_in_range(",
             "inline bool pl_facing(", "inline bool pl_cos_ok(", "inline Plane pl_from_normal(", "inline bool pl_from_triple(", "inline bool pl_caller_ok(", "inline uint32_t pl_winner(",
             "inline PlaneFit pl_solve(", "inline bool pl_level(", "inline float pl_centre(")
    for text in (kernels, api, driver):
        assert '#include "plane_math.h"' in text
        for rule in rules:
            assert rule not in text, rule
        assert "0x9E3779B97F4A7C15" not in text and "fabsf(" not in text
    for rule in rules:
        assert header.count(rule) == 1, rule
    body = header.split("#pragma once")[1]
    assert "hip" not in body.lower() and '#include "normals_math.h"' in body and "ex_rotate<double, 0, 1>" in body and "kExportSweeps" in body
    assert "nm_flip(" in body and "nm_is_fitted(" in body  # section 26's sign and "fitted", not copies
    # the score, the moments and the select all call the one residual and the one inlier rule
    score = kernels.split("void k_plane_score(")[1].split("__global__")[0]
    moments = kernels.split("void k_plane_moments(")[1].split("__global__")[0]
    select = kernels.split("void k_plane_select(")[1].split("namespace {")[0]
    assert "pl_inlier(pl_residual(" in score and "pl_cos_ok(" in score and "nm_is_fitted(" in score  # (pl_facing's two halves, the first once a Gaussian)
    assert "pl_residual(" in moments and "pl_inlier(" in moments and "pl_facing(" in moments and "pl_centre(" in moments
    assert "pl_in_range(pl_residual(" in select and "pl_facing(" in select and "select_write(" in select and "select_store_partial(" in select
    assert "launch_select_finish(" in kernels and "combine_terms(" in kernels and "atomicAdd(&job.counts[j], cnt)" in kernels
    # no float atomics: the only atomic adds are on uint32 words
    assert "atomicAdd(job.sums" not in kernels and "atomicAdd(job.partials" not in kernels
    # the folds are wave_reduce.h's, one copy, which the align passes call too
    reduce_h, nearest = _read("wgpu_3dgs_viewer_app_amd", "csrc", "wave_reduce.h"), _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_nearest.hip")
    assert reduce_h.count("inline DoubleTerms<T> combine_terms(") == 1 and "inline DoubleTerms<T> combine_terms(" not in nearest and "combine_terms(p)" in nearest
    assert "model_filter(m, desc->filter" in api and "neighbor_model(v, fn, key, &m)" in api and "select_begin(" in api and "select_end(m)" in api
    makefile = _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")
    assert "kernels_plane.hip" in makefile and "gsx_api_plane.cpp" in makefile and "$(wildcard *.h)" in makefile and "-ffp-contract=off" in makefile
    # these calls stay out of the model session's fuzz
    assert "fit_plane" not in _read("tests", "test_gpu_model_fuzz.py") and "select_plane" not in _read("tests", "model_shadow.py")


# ---- 2. the driver ------------------------------------------------------------------------------------------------------------------
def build_driver(directory) -> str:
    exe = str(directory / "plane_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "plane_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("plane"))


def _hex(a):
    return " ".join(f"{w:x}" for w in np.ascontiguousarray(a, F).reshape(-1).view(np.uint32))


def _hex64(a):
    return " ".join(f"{w:x}" for w in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def _f32(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(F)


def _f64(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)


def _run(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def _rows(pos, part, normals=None, variation=None):
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    n = len(pos)
    rows = np.zeros((n, 8), np.uint32)
    rows[:, 0:3] = pos.view(np.uint32)
    rows[:, 3] = np.asarray(part, bool)
    rows[:, 4:7] = (np.zeros((n, 3), F) if normals is None else np.ascontiguousarray(normals, F)).view(np.uint32)
    rows[:, 7] = (np.full(n, np.inf, F) if variation is None else np.ascontiguousarray(variation, F)).view(np.uint32)
    return " ".join(f"{w:x}" for w in rows.reshape(-1))


def play_fit(driver, pos, part, sample, H, seed, tolerance, min_cos=0.0, normals=None, variation=None, given=None):
    """dict(valid, slots, planes, counts, winner) of the driver's candidates and scores"""
    text = f"fit {sample:x} {seed:x} {H:x} {_hex(F(tolerance))} {_hex(F(min_cos))} {len(pos):x} {_rows(pos, part, normals, variation)}".rstrip()
    if sample == PR.CALLER:
        text += " " + _hex(given)
    out = _run(driver, text + "\n")
    assert len(out) == H + 1 and all(ln[0] == "cand" for ln in out[:H]) and out[H][0] == "winner"
    return dict(valid=np.array([int(ln[1]) for ln in out[:H]], bool), slots=np.array([[int(x, 16) for x in ln[2:5]] for ln in out[:H]], np.int64),
                planes=np.stack([_f32(ln[5:9]) for ln in out[:H]]), counts=np.array([int(ln[9], 16) for ln in out[:H]], np.uint32), winner=int(out[H][1], 16))


def play_moments(driver, plane, pos, part, tolerance, min_cos=0.0, normals=None, variation=None):
    out = _run(driver, f"moments {_hex(plane)} {_hex(F(tolerance))} {_hex(F(min_cos))} {len(pos):x} {_rows(pos, part, normals, variation)}".rstrip() + "\n")
    d = _f64(out[0][1:])
    return dict(count=int(d[0]), sum_p=d[1:4], sum_r2=float(d[4]), scatter=d[5:11])


def play_solve(driver, count, sum_p, scatter, toward=None):
    """dict(ok, plane, centre, eigenvalues) of pl_solve"""
    t = F([0, 0, 0]) if toward is None else F(toward)
    out = _run(driver, f"solve {0 if toward is None else 1:x} {_hex(t)} {_hex64(np.concatenate([[float(count)], sum_p, scatter]))}\n")[0]
    assert out[0] == "solve"
    return dict(ok=bool(int(out[1])), plane=_f32(out[2:6]), centre=_f32(out[6:9]), eigenvalues=_f64(out[9:12]))


def play_level(driver, plane, up):
    out = _run(driver, f"level {_hex(plane)} {_hex(up)}\n")[0]
    d = _f64(out[2:])
    return bool(int(out[1])), d[:4], d[4:]


def assert_moments_within_bound(got, ref):
    """The reference takes every term as the code under test does, in float64 from the same float32 values, and sums them exactly
    (math.fsum); the code under test adds the same m terms in some order: |got - ref| <= (m + 4) 2^-53 sum|term| (align_plane_ref.bound,
    whose argument — m - 1 roundings of partial sums that sum|term| bounds, and slack for the second order and the reference's own
    rounding — carries over unchanged: it uses nothing about the terms but that both sides hold the same ones).  Derived, not measured.
    The centre is compared through sum p: it is a function of it."""
    m = ref["count"]
    assert got["count"] == m
    for key in ("sum_p", "scatter"):
        if key in got:
            err, lim = np.abs(np.asarray(got[key]) - np.asarray(ref[key])), PR.bound(m, ref["mag"][key])
            assert np.all(err <= lim), (key, err, lim)
    if "sum_r2" in got:
        assert abs(got["sum_r2"] - ref["sum_r2"]) <= PR.bound(m, ref["mag"]["sum_r2"])


@pytest.fixture(scope="module")
def corners():
    """seed -> (pos, normals, variation), made once and not changed"""
    return {seed: PR.corner(seed) for seed in range(3)}


def test_mix_and_the_probe(driver):
    cases = [(0, 0, 0, 0), (7, 1023, 2, 63), (2 ** 64 - 1, 5, 1, 9), (0x0123456789ABCDEF, 300, 0, 31)]
    out = _run(driver, "".join(f"mix {s:x} {h:x} {k:x} {t:x}\n" for s, h, k, t in cases))
    assert [int(ln[1], 16) for ln in out] == [PR.mix(*c) for c in cases]
    assert PR.mix(0, 0, 0, 0) == 0xE220A8397B1DCDAF  # the first output of splitmix64 seeded with 0 (the published test vector)
    # different counters give different draws
    assert len({PR.mix(3, h, s, t) for h in range(8) for s in range(3) for t in range(64)}) == 8 * 3 * 64


def test_candidates_and_counts_against_the_reference(driver, corners):
    pos, nrm, var = corners[0]
    n = len(pos)
    rng = np.random.default_rng(11)
    third = np.arange(n) % 3 == 0
    holes = pos.copy()
    holes[5, 0], holes[77, 2] = np.nan, np.inf
    some_var = var.copy()
    some_var[::5] = np.inf
    given = np.concatenate([rng.normal(size=(6, 3)), rng.random((6, 1))], axis=1).astype(F)
    given[1, :3], given[3, 3], given[4, 0] = 0, np.nan, np.inf
    cases = [dict(sample=PR.TRIPLES, H=64, seed=7, part=PR.participants(pos)), dict(sample=PR.TRIPLES, H=65, seed=8, part=PR.participants(holes, third), pos=holes),
             dict(sample=PR.NORMALS, H=64, seed=7, part=PR.participants(pos), variation=some_var),
             dict(sample=PR.NORMALS, H=33, seed=2 ** 63 + 5, part=PR.participants(pos, third), min_cos=0.9, variation=some_var),
             dict(sample=PR.CALLER, H=6, seed=0, part=PR.participants(pos), given=given),
             dict(sample=PR.TRIPLES, H=16, seed=1, part=np.arange(n) < 2),    # two participants: no triple
             dict(sample=PR.TRIPLES, H=16, seed=1, part=np.zeros(n, bool))]  # none
    for case in cases:
        p, part, v = case.get("pos", pos), case["part"], case.get("variation", var)
        got = play_fit(driver, p, part, case["sample"], case["H"], case["seed"], 0.006, case.get("min_cos", 0.0), nrm, v, case.get("given"))
        planes, valid, slots = PR.candidates(p, part, case["sample"], case["H"], case["seed"], nrm, v, case.get("given"))
        cnt = PR.counts(planes, valid, p, part, 0.006, case.get("min_cos", 0.0), nrm, v)
        assert np.array_equal(got["valid"], valid) and np.array_equal(got["slots"], slots & 0xFFFFFFFF), case["sample"]
        assert got["planes"].tobytes() == planes.tobytes()  # bit for bit: the same IEEE operations in the same order on both sides
        assert np.array_equal(got["counts"], cnt) and got["winner"] == PR.winner(cnt, valid)
    assert not valid.any() and got["winner"] == PR.NONE and not cnt.any()
    # coincident and collinear triples are invalid, not NaN planes
    assert PR.from_triple([0, 0, 0], [1, 1, 1], [2, 2, 2]) is None and PR.from_triple([1, 2, 3], [1, 2, 3], [0, 0, 1]) is None


def _fit_inputs(corners):
    """(name, pos, plane, inlier mask): the winning candidates and the refined planes whose inliers the solve is tested on"""
    out = []
    for seed, (pos, nrm, var) in corners.items():
        for sample in (PR.TRIPLES, PR.NORMALS):
            f = PR.fit(pos, PR.participants(pos), sample, 256, 7, 0.006, refine_iters=1, normals=nrm, variation=var)
            for name, plane in (("candidate", f["candidate"]), ("refined", f["plane"])):
                out.append((f"corner{seed}-{sample}-{name}", pos, plane, PR.inliers(plane, pos, PR.participants(pos), 0.006)))
    pos, normal = PR.tilted_lattice()
    plane = np.concatenate([normal, [normal @ pos[0].astype(np.float64)]]).astype(F)
    out.append(("lattice", pos, plane, PR.inliers(plane, pos, PR.participants(pos), 1e-4)))
    return out


def test_moments_against_the_reference(driver, corners):
    for name, pos, plane, inl in _fit_inputs(corners):
        ref = PR.moments(plane, pos, inl)
        tol = 1e-4 if name == "lattice" else 0.006
        got = play_moments(driver, plane, pos, PR.participants(pos), tol)
        assert ref["count"] == int(inl.sum()) >= 900, name
        assert_moments_within_bound(got, ref)
        assert np.array_equal(F(got["sum_p"] / got["count"]), ref["centre"]), name  # (the fixtures' quotients do not sit on a float32 tie)


def solve_deviation(got, ref):
    """(normal, offset, eigenvalues over the largest) absolute deviations"""
    return (float(np.abs(got["plane"][:3].astype(np.float64) - ref["plane"][:3]).max()), float(abs(float(got["plane"][3]) - float(ref["plane"][3]))),
            float(np.abs(got["eigenvalues"] - ref["eigenvalues"]).max() / ref["eigenvalues"][0]))


def test_solve_against_numpy(driver, corners):
    worst = np.zeros(3)
    for name, pos, plane, inl in _fit_inputs(corners):
        mom = PR.moments(plane, pos, inl)
        for toward in (None, (0.5, 0.5, 0.5), (-3.0, -2.0, -5.0)):
            got = play_solve(driver, mom["count"], mom["sum_p"], mom["scatter"], toward)
            ref = PR.solve(mom, toward)
            assert got["ok"] and ref is not None, name
            dev = solve_deviation(got, ref)
            worst = np.maximum(worst, dev)
            assert dev[0] <= SOLVE_NORMAL and dev[1] <= SOLVE_OFFSET and dev[2] <= SOLVE_EIG, (name, dev)
            assert np.array_equal(got["centre"], mom["centre"]) and np.all(np.diff(got["eigenvalues"]) <= 0) and got["eigenvalues"][2] >= 0
            assert abs(float(np.linalg.norm(got["plane"][:3].astype(np.float64))) - 1) <= 2.0 ** -23
            n64, c64 = got["plane"][:3].astype(np.float64), got["centre"].astype(np.float64)
            assert got["plane"][3] == F((n64[0] * c64[0] + n64[1] * c64[1]) + n64[2] * c64[2])  # the offset from the float32 normal and centre
            if toward is not None:
                assert n64 @ (np.asarray(F(toward), np.float64) - c64) > 0
            else:
                assert got["plane"][:3][np.flatnonzero(got["plane"][:3])[0]] > 0
    print(f"worst: normal {worst[0]:.2e} offset {worst[1]:.2e} eig {worst[2]:.2e}")
    # no plane: fewer than three points, points that coincide
    assert not play_solve(driver, 2, [1.0, 1.0, 1.0], [1.0, 0, 0, 1.0, 0, 0])["ok"]
    none = play_solve(driver, 5, [1.0, 1.0, 1.0], np.zeros(6))
    assert not none["ok"] and not none["plane"].any()
    assert PR.solve(dict(count=5, scatter=np.zeros(6), centre=F([0, 0, 0]))) is None


# ---- 3. gsx_plane_level -----------------------------------------------------------------------------------------------------------------
def test_level(driver):
    rng = np.random.default_rng(3)
    cases = [((0, 0, 1, 0.5), (0, 0, 1)), ((0, 0, 2, 0.5), (0, 0, 3)),  # the identity: parallel already
             ((0, 0, -1, 0.25), (0, 0, 1)), ((-1, 0, 0, 1), (2, 0, 0)), ((0, -3, 0, 1), (0, 1, 0)), ((1, 1, 1, 2), (-1, -1, -1)),  # antiparallel
             ((1, 0, 0, 1), (0, 0, 1)), ((0.6, 0, 0.8, -1), (0, 1, 0))]
    cases += [(tuple(rng.normal(size=3)) + (float(rng.normal()),), tuple(rng.normal(size=3))) for _ in range(24)]
    for plane, up in cases:
        plane, up = F(plane), F(up)
        ok, q, pos = play_level(driver, plane, up)
        assert ok
        a = plane[:3].astype(np.float64) / np.linalg.norm(plane[:3].astype(np.float64))
        b = up.astype(np.float64) / np.linalg.norm(up.astype(np.float64))
        Rm = PR.quat_rows(q)
        assert np.abs(Rm @ a - b).max() <= LEVEL_ULPS * 2.0 ** -52, (plane, up, np.abs(Rm @ a - b).max() / 2.0 ** -52)
        assert q[3] >= 0 and abs(np.linalg.norm(q) - 1) <= 4e-16
        h = float(plane[3]) / np.linalg.norm(plane[:3].astype(np.float64))
        assert np.abs(pos + h * b).max() <= 2.0 ** -52 * abs(h)
        # a point of the plane lands at height 0 along up
        p = a * h
        assert abs((Rm @ p + pos) @ b) <= 8 * 2.0 ** -52 * max(1.0, abs(h))
        rq, rpos = PR.level(plane, up)
        assert np.abs(q - rq).max() <= 4e-16 and np.abs(pos - rpos).max() <= 4e-16 * max(1.0, abs(h))
        # the C ABI rounds the same numbers to float32
        cq, cpos = plane_level(plane, up)
        assert np.array_equal(cq, q.astype(F)) and np.array_equal(cpos, pos.astype(F))
    ok, q, _ = play_level(driver, F([0, 0, 1, 0.5]), F([0, 0, 1]))
    assert np.array_equal(q, [0, 0, 0, 1])  # the identity exactly
    ok, q, _ = play_level(driver, F([0, 0, -1, 0]), F([0, 0, 1]))
    assert np.array_equal(q, [0, 1, 0, 0])  # antiparallel: the half turn about e x n, e the x axis (the first of the smallest)
    for plane, up in (((0, 0, 0, 1), (0, 0, 1)), ((0, 0, 1, 1), (0, 0, 0)), ((np.nan, 0, 1, 1), (0, 0, 1)), ((0, 0, 1, np.inf), (0, 0, 1)), ((0, 0, 1, 1), (0, np.inf, 1))):
        assert not play_level(driver, F(plane), F(up))[0]
        with pytest.raises(Exception, match="gsx_plane_level"):
            plane_level(plane, up)


# ---- 4. the peel ---------------------------------------------------------------------------------------------------------------------------
def face_counts(seed, n=3000):
    """how many of align_plane_ref.corner_points(n, seed)'s points lie on each face (its own draws, replayed)"""
    rng = np.random.default_rng(seed)
    rng.random((n, 3))
    return np.bincount(rng.integers(0, 3, n), minlength=3)


def assert_peel(planes, n_inliers, seed):
    """three planes, one per axis: |n . axis| > 0.999 (the experiment's worst case is 0.99996) and at least 85 % of that face's points"""
    faces = face_counts(seed)
    axes = [int(np.argmax(np.abs(p[:3]))) for p in planes]
    assert sorted(axes) == [0, 1, 2], axes
    for plane, count, axis in zip(planes, n_inliers, axes):
        n = plane[:3].astype(np.float64)
        assert abs(n[axis]) / np.linalg.norm(n) > 0.999 and count >= 0.85 * faces[axis], (seed, axis, n, count, faces[axis])


@pytest.mark.parametrize("sample", [PR.TRIPLES, PR.NORMALS])
def test_three_fits_peel_the_corner(driver, corners, sample):
    for seed, (pos, nrm, var) in corners.items():
        part = PR.participants(pos)
        planes, n_inliers = [], []
        for call in range(3):
            ref = PR.fit(pos, part, sample, 256, 7, 0.006, refine_iters=2, normals=nrm, variation=var)
            got = play_fit(driver, pos, part, sample, 256, 7, 0.006, normals=nrm, variation=var)  # the header's candidates and scores
            assert got["planes"].tobytes() == ref["candidates"].tobytes() and np.array_equal(got["counts"], ref["counts"]) and got["winner"] == ref["winner"]
            assert not ref["degenerate"] and ref["n_inliers"] >= ref["candidate_inliers"] == int(ref["counts"][ref["winner"]])
            inl = PR.inliers(ref["plane"], pos, part, 0.006)
            assert int(inl.sum()) == ref["n_inliers"]
            planes.append(ref["plane"])
            n_inliers.append(ref["n_inliers"])
            part = part & ~inl
        assert_peel(planes, n_inliers, seed)


def test_the_stop_rule_fixture(corners):
    """Corner seed 2, NORMALS, 256 candidates, seed 7, tolerance 0.006: the first refine round raises the winner's 1024 inliers to 1036,
    the second would lower them to 1035: the call stops with the first round's plane."""
    pos, nrm, var = corners[2]
    f = PR.fit(pos, PR.participants(pos), PR.NORMALS, 256, 7, 0.006, refine_iters=4, normals=nrm, variation=var)
    assert (f["candidate_inliers"], f["history"], f["n_inliers"], f["refine_done"]) == (1024, [1036, 1035], 1036, 1)
    assert math.isclose(f["rms"], math.sqrt(f["sum_r2"] / 1036))
