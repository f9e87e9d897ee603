"""Model properties (gsx_model_property_values, gsx_model_histogram, gsx_model_select_range; spec §17) without a device: the entry
points, the enum, the flags and the structs in the header, the library, the bindings and the facades; and the arithmetic of
csrc/property_math.h — played by tests/property_driver.cpp, a stand-alone program built with the address and undefined-behaviour
sanitizers and run as a child process — against the numpy restatement tests/property_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import property_ref as P
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
NAMES = ("POS_X", "POS_Y", "POS_Z", "RED", "GREEN", "BLUE", "OPACITY", "HUE", "SATURATION", "VALUE", "SCALE_MAX", "SCALE_MID", "SCALE_MIN", "COUNT")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points_enum_flags_and_structs():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^gsx_status gsx_model_property_values\(gsx_viewer\* v, const char\* key, uint32_t property, uint32_t flags, float\* out, "
                     r"uint64_t n\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_histogram\(gsx_viewer\* v, const char\* key, const gsx_histogram_desc\* desc, uint64_t\* out_bins, "
                     r"gsx_histogram_t\* out\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_select_range\(gsx_viewer\* v, const char\* key, const gsx_select_desc\* desc, uint64_t\* out_hit, "
                     r"uint64_t\* out_selected\);", hdr, re.M)
    for value, name in enumerate(NAMES):
        assert re.search(rf"\bGSX_PROP_{name} = {value}\b", hdr) and getattr(_lib, "GSX_PROP_" + name) == value == getattr(P, name)
    for name, value in (("GSX_PROP_WORLD", 1), ("GSX_HIST_AUTO_RANGE", 4), ("GSX_HIST_MAX_BINS", 4096)):
        assert re.search(rf"^#define {name}\s+{value}u\b", hdr, re.M) and getattr(_lib, name) == value
    assert (P.WORLD, P.AUTO_RANGE, P.MAX_BINS) == (_lib.GSX_PROP_WORLD, _lib.GSX_HIST_AUTO_RANGE, _lib.GSX_HIST_MAX_BINS)
    assert (P.SET, P.ADD, P.REMOVE) == (_lib.GSX_SELECTION_SET, _lib.GSX_SELECTION_ADD, _lib.GSX_SELECTION_REMOVE)
    assert re.search(r"GSX_SELECTION_SET = 0, GSX_SELECTION_ADD = 1, GSX_SELECTION_REMOVE = 2", hdr)
    assert re.search(r"typedef struct gsx_histogram_desc \{ uint32_t property; uint32_t flags; uint32_t filter; uint32_t bins; float lo; float hi; \}", hdr)
    assert re.search(r"typedef struct gsx_histogram_t \{ uint64_t count; uint64_t below; uint64_t above; uint64_t n_nonfinite; float lo; float hi; "
                     r"float min; float max; \}", hdr)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # additive: the version stays


def test_ctypes_mirrors_have_the_header_layout():
    offsets = lambda s: {f: getattr(s, f).offset for f, _ in s._fields_}  # noqa: E731
    assert C.sizeof(_lib.HistogramDesc) == 24
    assert offsets(_lib.HistogramDesc) == {"property": 0, "flags": 4, "filter": 8, "bins": 12, "lo": 16, "hi": 20}
    # four 64-bit counts and four floats: 48 bytes
    assert C.sizeof(_lib.Histogram) == 48
    assert offsets(_lib.Histogram) == {"count": 0, "below": 8, "above": 16, "n_nonfinite": 24, "lo": 32, "hi": 36, "min": 40, "max": 44}
    assert C.sizeof(_lib.SelectDesc) == 40
    assert offsets(_lib.SelectDesc) == {"property": 0, "flags": 4, "filter": 8, "selection_op": 12, "lo": 16, "hi": 20, "bins": 24, "bin_lo": 28,
                                        "bin_hi": 32, "reserved": 36}
    api = _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_property.cpp")
    assert "sizeof(gsx_histogram_desc) == 24 && sizeof(gsx_histogram_t) == 48 && sizeof(gsx_select_desc) == 40" in api


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in ("gsx_model_property_values", "gsx_model_histogram", "gsx_model_select_range"):
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp
    for s in ("gsx_histogram_desc", "gsx_histogram_t", "gsx_select_desc"):
        assert "pub struct " + s in rust_sys
    assert "pub enum gsx_property" in rust_sys
    assert all(f"pub const {n}: u32" in rust_sys for n in ("GSX_PROP_WORLD", "GSX_HIST_AUTO_RANGE", "GSX_HIST_MAX_BINS", "GSX_PROP_COUNT"))
    for method in ("property_values", "histogram", "select_range"):
        assert f"pub fn {method}(" in rust and re.search(rf"\b{method}\(", hpp)
    # without a device: a status code and a message, not a crash
    out, bins, hist = (C.c_float * 4)(), (C.c_uint64 * 4)(), _lib.Histogram()
    hd, sd = _lib.HistogramDesc(0, 0, 0, 4, 0.0, 1.0), _lib.SelectDesc(0, 0, 0, 0, 0.0, 1.0, 0, 0, 0, 0)
    assert L.gsx_model_property_values(None, b"a", 0, 0, out, 4) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_property_values" in L.gsx_last_error_string()
    assert L.gsx_model_histogram(None, b"a", C.byref(hd), bins, C.byref(hist)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_histogram" in L.gsx_last_error_string()
    assert L.gsx_model_select_range(None, b"a", C.byref(sd), None, None) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_select_range" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert all(callable(getattr(MultiModelViewerModel, m)) for m in ("property_values", "histogram", "select_range"))


def test_the_bin_recipe_is_restated_not_shared():
    """bounds_math.h is left as it is (its device code stays what it is): property_math.h states the recipe again and does not
    include it."""
    math_h = _read("wgpu_3dgs_viewer_app_amd", "csrc", "property_math.h")
    assert '#include "bounds_math.h"' not in math_h and '#include "export_math.h"' in math_h
    assert "kPropMaxBins = GSX_HIST_MAX_BINS" in math_h


# ---- csrc/property_math.h against the numpy restatement ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("property") / "property_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "property_driver.cpp"), "-o", exe])
    return exe


def _hex(a):
    return " ".join(f"{int(w):x}" for w in np.asarray(a).reshape(-1))


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def _fx(x):
    return f"{int(P.bits(np.array([x], F))[0]):x}"


#: ranges: ordinary, negative to positive, lo == hi, a few ulps, a width that underflows (denormals), huge (hi - lo overflows), zeros
RANGES = [(0.0, 1.0), (-3.25, 7.5), (2.5, 2.5), (1.0, float(P.next_up(F(1.0), 3))), (0.0, 1e-42), (-1e-44, 1e-44), (-3e38, 3e38),
          (1e-3, 1.0 + 1e-3), (-0.0, 0.0), (1000.0, 1000.5)]


def _probe_values(r):
    """every edge, one ulp either side of it, the ends, beyond them, the middles, and the values nothing counts"""
    edges = r.edge(np.arange(r.bins + 1))
    near = np.concatenate([edges, [P.next_up(e, 1) for e in edges[:: max(1, r.bins // 64)]], [P.next_up(e, -1) for e in edges[:: max(1, r.bins // 64)]],
                           [P.next_up(edges[-1], 1), P.next_up(edges[0], -1), P.next_up(edges[-1], -1), P.next_up(edges[0], 1)]]).astype(F)
    with np.errstate(all="ignore"):
        mids = (edges[:-1] * F(0.5) + edges[1:] * F(0.5)).astype(F)[:: max(1, r.bins // 32)]
    rng = np.random.default_rng(r.bins)
    rand = (F(r.lo) + rng.random(64).astype(F) * F(min(float(r.hi) - float(r.lo), 3e38))).astype(F)
    return np.concatenate([near, mids, rand, np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.4e38, -3.4e38], F)]).astype(F)


@pytest.mark.parametrize("bins", P.BIN_COUNTS)
@pytest.mark.parametrize("lo_hi", RANGES, ids=lambda r: f"{r[0]:g}..{r[1]:g}")
def test_driver_bins_agree_with_the_restatement(driver, lo_hi, bins):
    r = P.Range(*lo_hi, bins)
    v = _probe_values(r)
    out = _play(driver, f"range {_fx(r.lo)} {_fx(r.hi)} {bins}\nclassify {_hex(P.bits(v))}\nhit 0 0 0 {_hex(P.bits(v))}\n"
                        f"hit 1 {bins // 3} {bins // 2} {_hex(P.bits(v))}\nminmax {_hex(P.bits(v))}\n")
    assert out[0] == ["live", str(int(r.live))]
    edges = np.array([int(w, 16) for w in out[1][1:]], np.uint32)
    assert np.array_equal(edges, P.bits(r.edge(np.arange(bins + 1))))
    assert edges[0] == P.bits(r.lo)[()] and edges[-1] == P.bits(r.hi)[()]  # edge(0) = lo and edge(bins) = hi exactly
    cls = np.array(out[2][1:], np.int64)
    want = P.classify(r, v)
    assert np.array_equal(cls, want)
    inside = cls >= 0
    if r.live:  # every value lies between the edges of its bin
        assert np.all(r.edge(cls[inside]) <= v[inside]) and np.all(v[inside] <= r.edge(cls[inside] + 1))
    else:
        assert np.all(cls[inside] == 0)  # zero, too small or not finite: bin 0
    assert np.array_equal(np.array(out[3][1:], np.int64) == 1, P.hits(v, np.ones(v.size, bool), r.lo, r.hi))
    assert np.array_equal(np.array(out[4][1:], np.int64) == 1, P.hits(v, np.ones(v.size, bool), r.lo, r.hi, bins, bins // 3, bins // 2))
    fin = v[P.finite(v)]
    mn, mx = P.min_max(fin)
    assert out[5][1:] == [str(fin.size), _fx(mn), _fx(mx)]
    assert P.bits(mn)[()] == 0xFF7FC99E and P.bits(mx)[()] == 0x7F7FC99E  # (+-3.4e38)


SWEEPS = [(1.0, 2.0), (0.5, float(P.next_up(F(0.5), 5000))), (-1e-40, 1e-40), (0.0, float(P.next_up(F(0.0), 70000))), (8.0, 8.0),
          (16777216.0, 16777216.0 + 4096 * 2)]


@pytest.mark.parametrize("bins", P.BIN_COUNTS)
def test_every_value_of_a_range_lies_between_the_edges_of_its_bin(driver, bins):
    """exhaustive: every float32 of the range, its bin's edges enclose it and the bins never decrease"""
    text = "".join(f"range {_fx(lo)} {_fx(hi)} {bins}\nsweep\n" for lo, hi in SWEEPS)
    out = [ln for ln in _play(driver, text) if ln[0] == "sweep"]
    assert len(out) == len(SWEEPS)
    for (lo, hi), ln in zip(SWEEPS, out):
        want = int(P.key(np.array([hi], F))[0]) - int(P.key(np.array([lo], F))[0]) + 1
        assert (int(ln[1]), int(ln[2])) == (want, 0), (lo, hi, ln)
    assert int(out[0][1]) == (1 << 23) + 1  # all of [1, 2]


def test_the_single_bin_hit_sets_partition_the_in_range_set(driver):
    bins, lo, hi = 16, F(-1.5), F(2.25)
    rng = np.random.default_rng(5)
    r = P.Range(lo, hi, bins)
    v = np.concatenate([(rng.random(3000).astype(F) * F(5) - F(2)).astype(F), r.edge(np.arange(bins + 1)), np.array([np.nan, np.inf, -np.inf], F)]).astype(F)
    text = f"range {_fx(lo)} {_fx(hi)} {bins}\nhit 0 0 0 {_hex(P.bits(v))}\n" + "".join(f"hit 1 {b} {b} {_hex(P.bits(v))}\n" for b in range(bins))
    out = _play(driver, text)[2:]
    in_range = np.array(out[0][1:], np.int64)
    per_bin = np.array([ln[1:] for ln in out[1:]], np.int64)
    assert np.array_equal(per_bin.sum(axis=0), in_range)  # each in-range value in exactly one bin, the others in none
    assert in_range.sum() == int((P.finite(v) & (v >= lo) & (v <= hi)).sum())
    want = P.histogram(v, np.ones(v.size, bool), bins, lo, hi)
    assert np.array_equal(per_bin.sum(axis=1).astype(np.uint64), want["bins"])  # a bin's hit count is the histogram's bin
    assert want["count"] - want["below"] - want["above"] == int(want["bins"].sum()) and want["n_nonfinite"] == 3


def test_driver_values_agree_with_the_restatement(driver):
    rng = np.random.default_rng(11)
    n = 300
    pos = (rng.standard_normal((n, 3)) * 10).astype(F)
    pos[:6] = np.array([[np.nan, 1, 2], [np.inf, 0, 0], [-0.0, 0.0, -np.inf], [1e38, 1e38, 1e38], [1e-45, -1e-45, 0], [3, 4, 5]], F)
    color = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    color[:8] = [0, 0xFFFFFFFF, 0xFF0000FF, 0x0000FF00, 0x00FF0000, 0x80808080, 0x01010101, 0x7F80FF00]  # greys, primaries, ties of the max
    elems = np.concatenate([P.bits(pos), color[:, None]], axis=1)
    R = np.array([0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6], F)
    s, t = np.array([1.5, -2.0, 0.25], F), np.array([10.0, -20.0, 0.125], F)
    text = f"xform {_hex(P.bits(np.concatenate([R, s, t])))}\n"
    text += "".join(f"pc {p} 0 {_hex(elems)}\n" for p in range(10)) + "".join(f"pc {p} 1 {_hex(elems)}\n" for p in range(3))
    out = _play(driver, text)
    got = [np.array([int(w, 16) for w in ln[1:]], np.uint32) for ln in out]
    for p in range(10):
        assert np.array_equal(got[p], P.bits(P.values_pc(p, pos, color))), p
    for p in range(3):
        assert np.array_equal(got[10 + p], P.bits(P.values_pc(p, pos, color, (R, s, t)))), p
    assert np.array_equal(got[0], P.bits(pos[:, 0]))  # stored bits, NaN payloads and -0 included
    hue, sat, val = (P.from_bits(got[p]) for p in (7, 8, 9))
    assert np.all((hue >= 0) & (hue < 1)) and np.all((sat >= 0) & (sat <= 1)) and np.all((val >= 0) & (val <= 1))
    assert hue[0] == 0 and sat[0] == 0 and val[0] == 0 and val[1] == 1 and sat[1] == 0


def test_driver_scales_of_plain_covariances(driver):
    """the scales are ex_solve's (the yardstick is gsx_model_export, on the device): here the cases with a known answer"""
    cov = np.array([[4, 0, 0, 9, 0, 1], [1, 0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 0], [0.25, 0, 0, 0, 0, 16], [np.inf, 0, 0, 4, 0, 9], [np.nan, 0, 0, 4, 0, -1]], F)
    out = _play(driver, "".join(f"scale {p} {_hex(P.bits(cov))}\n" for p in (10, 11, 12)))
    mx, mid, mn = (P.from_bits(np.array([int(w, 16) for w in ln[1:]], np.uint32)) for ln in out)
    assert np.array_equal(mx[:4], F([3, 1, 0, 4])) and np.array_equal(mid[:4], F([2, 1, 0, 0.5])) and np.array_equal(mn[:4], F([1, 1, 0, 0]))
    # a non-finite entry: no solve, the roots of the diagonal in place (spec §14)
    assert np.isinf(mx[4]) and mid[4] == 2 and mn[4] == 3
    assert mx[5] == 0 and mid[5] == 2 and mn[5] == 0


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 1025])
@pytest.mark.parametrize("op", [P.SET, P.ADD, P.REMOVE])
def test_driver_selection_op_agrees_with_the_restatement(driver, op, n):
    rng = np.random.default_rng(n * 3 + op)
    old, hit = rng.random(n) < 0.5, rng.random(n) < 0.3
    out = _play(driver, f"op {op} {n} {_hex(P.words(old, True))} | {_hex(P.words(hit, True))}\n")  # garbage in the tails
    got = np.array([int(w, 16) for w in out[0][1:]], np.uint32)
    assert np.array_equal(got, P.words(P.apply_op(op, old, hit)))  # ... and the tail bits written 0
