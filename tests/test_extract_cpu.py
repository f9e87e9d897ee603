"""Model extract (gsx_model_extract, spec §12) without a device: the two entry points, the flags and the struct in the header, the
library, the bindings and the facades; and the word arithmetic of csrc/extract_math.h — played by tests/extract_driver.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process — against the numpy
restatement tests/extract_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import extract_ref as X
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points_flags_and_struct():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^void gsx_extract_desc_default\(gsx_extract_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_extract\(gsx_viewer\* v, const char\* src_key, const char\* dst_key,\s*"
                     r"const gsx_extract_desc\* desc, uint64_t\* out_count\);", hdr, re.M)
    for name, value in (("GSX_EXTRACT_INVERT", 1), ("GSX_EXTRACT_DROP_EDITS", 2)):
        assert re.search(rf"^#define {name}\s+{value}u\b", hdr, re.M) and getattr(_lib, name) == value
    assert re.search(r"typedef struct gsx_extract_desc \{ uint32_t filter; uint32_t flags; \} gsx_extract_desc;", hdr)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3
    assert (X.MASKED, X.SKIP_HIDDEN, X.SELECTED) == (_lib.GSX_BOUNDS_MASKED, _lib.GSX_BOUNDS_SKIP_HIDDEN, _lib.GSX_BOUNDS_SELECTED)
    assert (X.INVERT, X.DROP_EDITS) == (_lib.GSX_EXTRACT_INVERT, _lib.GSX_EXTRACT_DROP_EDITS)


def test_ctypes_mirror_has_the_header_layout():
    assert C.sizeof(_lib.ExtractDesc) == 8
    assert {f: getattr(_lib.ExtractDesc, f).offset for f, _ in _lib.ExtractDesc._fields_} == {"filter": 0, "flags": 4}


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys = _read("rust", "gsx-sys", "src", "lib.rs")
    for fn in ("gsx_extract_desc_default", "gsx_model_extract"):
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    assert "pub struct gsx_extract_desc" in rust_sys
    assert all(f"pub const {n}: u32" in rust_sys for n in ("GSX_EXTRACT_INVERT", "GSX_EXTRACT_DROP_EDITS"))
    assert "pub fn extract(" in _read("rust", "gsx", "src", "lib.rs") and "sys::gsx_model_extract(" in _read("rust", "gsx", "src", "lib.rs")
    assert re.search(r"uint64_t extract\(", _read("include", "gsx.hpp")) and "gsx_model_extract(" in _read("include", "gsx.hpp")
    d = _lib.ExtractDesc(7, 3)
    L.gsx_extract_desc_default(C.byref(d))
    assert (d.filter, d.flags) == (0, 0)
    # without a device: a status code and a message, not a crash
    count = C.c_uint64(99)
    assert L.gsx_model_extract(None, b"a", b"b", C.byref(d), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_extract" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert callable(MultiModelViewerModel.extract)


def test_the_shared_constants_agree_with_the_restatement():
    math_h = _read("wgpu_3dgs_viewer_app_amd", "csrc", "extract_math.h")
    assert re.search(rf"kExtractGroup = {X.GROUP};", math_h) and re.search(rf"kExtractScanPass = {X.SCAN_PASS};", math_h)


# ---- csrc/extract_math.h against the numpy restatement ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("extract") / "extract_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "extract_driver.cpp"), "-o", exe])
    return exe


def _hex(words):
    return " ".join(f"{int(w):x}" for w in words)


def _play(driver, n, filter_bits, invert, mask_words=None, sel_words=None, edited_words=None, edit_flags=None):
    text = f"n {n}\nfilter {filter_bits}\ninvert {int(invert)}\n"
    if mask_words is not None:
        text += f"mask {_hex(mask_words)}\n"
    if sel_words is not None:
        text += f"sel {_hex(sel_words)}\n"
    if edited_words is not None:
        text += f"edited {_hex(edited_words)}\nflags {' '.join(str(int(f)) for f in edit_flags)}\n"
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report, or a destination written twice / never)
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    got = np.array(lines["kept"], np.int64)
    assert int(lines["count"][0]) == got.size
    return got


def _planes(n, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random(n) < 0.6
    sel = rng.random(n) < 0.4
    flags = rng.choice(np.uint32([0, 1, 2, 3, 5, 7]), n)  # 3 and 7 hide; 2 (HIDDEN without ENABLED) does not
    edited = (flags & X.EDIT_ENABLED) != 0  # the `edited` plane is set where the stored flag has ENABLED
    return mask, sel, flags, edited


SIZES = [1, 31, 32, 33, 63, 64, 65, 4097]


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "invert"])
@pytest.mark.parametrize("filter_bits", range(8))
@pytest.mark.parametrize("n", SIZES)
def test_driver_agrees_with_the_restatement(driver, n, filter_bits, invert):
    mask, sel, flags, edited = _planes(n, 100 + n)
    flg = X.INVERT if invert else 0
    want = X.kept(n, filter_bits, flg, mask, sel, flags)
    # garbage above n in the last words of every bit plane
    got = _play(driver, n, filter_bits, invert, X.words(mask, True), X.words(sel, True), X.words(edited, True), flags)
    assert np.array_equal(got, want)
    # ... and clean tails give the same
    assert np.array_equal(_play(driver, n, filter_bits, invert, X.words(mask), X.words(sel), X.words(edited), flags), want)
    if filter_bits == 0:
        assert got.size == (0 if invert else n)
    # absent planes: a null mask gives all, a null selection gives none, no edit records hide nothing
    got_absent = _play(driver, n, filter_bits, invert)
    want_absent = X.kept(n, filter_bits, flg)
    assert np.array_equal(got_absent, want_absent)
    none = bool(filter_bits & X.SELECTED)
    assert got_absent.size == (n if none == invert else 0)


def test_patterns_across_words_and_groups(driver):
    n = 4097
    for name, mask in (("only bit 0", np.arange(n) == 0), ("only bit n - 1", np.arange(n) == n - 1), ("alternating", np.arange(n) % 2 == 1),
                       ("a clear word beside a set word", (np.arange(n) // 32) % 2 == 0), ("all clear", np.zeros(n, bool))):
        for invert in (False, True):
            got = _play(driver, n, X.MASKED, invert, X.words(mask, True))
            assert np.array_equal(got, np.nonzero(~mask if invert else mask)[0]), (name, invert)


# ---- the workspace of the kept-set pass (extract_ws_layout) ----
LAYOUTS = [[0], [1], [32], [33], [1024], [1025], [263169], [1, 0, 1025], [1024] * 16]


@pytest.mark.parametrize("sizes", LAYOUTS, ids=lambda s: "x".join(map(str, s)) if len(s) < 4 else f"{s[0]}x{len(s)}")
def test_workspace_layout(driver, sizes):
    r = subprocess.run([driver], input="layout " + " ".join(map(str, sizes)) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0][0] == "size" and [ln[0] for ln in lines[1:]] == [f"source{s}" for s in range(len(sizes))]
    size = int(lines[0][1])
    regions = [("totals", 0, 8 * len(sizes))]  # (name, start, bytes needed)
    for s, (n, ln) in enumerate(zip(sizes, lines[1:])):
        bases, partials, keep = map(int, ln[1:])
        groups = -(-n // X.GROUP)
        regions += [(f"bases{s}", bases, 4 * groups), (f"partials{s}", partials, 4 * groups), (f"keep{s}", keep, 4 * (-(-n // 32)))]
    regions.sort(key=lambda reg: reg[1])
    for (name, start, need), nxt in zip(regions, regions[1:] + [("end", size, 0)]):
        assert start % 128 == 0, name  # whole 128-byte lines
        assert start + need <= nxt[1], (name, nxt[0])  # as large as its kernel needs, disjoint from the next, inside the workspace
    if len(sizes) == 1:  # the total and the bases are one copy to the host
        assert dict((name, start) for name, start, _ in regions)["bases0"] == 128
