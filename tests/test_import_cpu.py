"""PLY import (gsx_model_import_ply, gsx_model_upload_ply_rows, spec §15) without a device: the entry points and the struct in the
header, the library, the bindings and the facades; and the arithmetic of csrc/import_math.h — played by tests/import_driver.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process — against the numpy
yardstick of tests/import_ref.py, bit for bit, and against the library's host reader gsx_ply_read_gaussians."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import import_ref as R
from wgpu_3dgs_viewer_app_amd import _lib, ply, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points_and_struct():
    hdr = _read("include", "gsx.h")
    assert re.search(r"typedef struct gsx_import_desc \{ uint32_t flags; uint32_t reserved; uint64_t staging_bytes; \} gsx_import_desc;", hdr)
    assert re.search(r"^void gsx_import_desc_default\(gsx_import_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_upload_ply_rows\(gsx_viewer\* v, const char\* key, uint64_t start, const void\* rows, uint64_t n,\s+"
                     r"const gsx_ply_header\* header, const gsx_import_desc\* desc\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_import_ply\(gsx_viewer\* v, const char\* key, const void\* data, uint64_t size, gsx_sh_kind sh,\s+"
                     r"gsx_cov3d_kind cov3d, const gsx_import_desc\* desc, uint64_t\* out_count\);", hdr, re.M)
    assert hdr.index("gsx_model_export_ply(") < hdr.index("gsx_import_desc_default(") < hdr.index("GSX_EDIT_ENABLED")  # after the export block
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3


def test_ctypes_mirror_has_the_header_layout():
    assert C.sizeof(_lib.ImportDesc) == 16
    assert {f: getattr(_lib.ImportDesc, f).offset for f, _ in _lib.ImportDesc._fields_} == {"flags": 0, "reserved": 4, "staging_bytes": 8}


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs")
    for fn in ("gsx_import_desc_default", "gsx_model_upload_ply_rows", "gsx_model_import_ply"):
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    assert "pub struct gsx_import_desc" in rust_sys
    assert "pub fn import_ply(" in rust and "sys::gsx_model_import_ply(" in rust
    assert "pub fn update_range_ply<Q>(" in rust and "sys::gsx_model_upload_ply_rows(" in rust
    hpp = _read("include", "gsx.hpp")
    assert re.search(r"uint64_t import_ply\(", hpp) and "gsx_model_import_ply(" in hpp
    assert re.search(r"void update_range_ply\(", hpp) and "gsx_model_upload_ply_rows(" in hpp
    d = _lib.ImportDesc(7, 5, 123)
    L.gsx_import_desc_default(C.byref(d))
    assert (d.flags, d.reserved, d.staging_bytes) == (0, 0, 0)
    # without a device: a status code and a message, not a crash
    count, h = C.c_uint64(99), _lib.PlyHeader()
    assert L.gsx_model_import_ply(None, b"a", b"ply\n", 4, 0, 0, C.byref(d), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_import_ply" in L.gsx_last_error_string()
    assert L.gsx_model_upload_ply_rows(None, b"a", 0, None, 0, C.byref(h), C.byref(d)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_upload_ply_rows" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import GaussiansBuffer, MultiModelViewer

    assert callable(MultiModelViewer.import_ply) and callable(GaussiansBuffer.update_range_ply)


def test_the_kernel_and_the_driver_share_the_header():
    kernel = _read("wgpu_3dgs_viewer_app_amd", "csrc", "kernels_import.hip")
    assert '#include "import_math.h"' in kernel and '#include "import_math.h"' in _read("tests", "import_driver.cpp")
    assert "im_row_to_gaussian(" in kernel and "store_gaussian(" in kernel
    # the write side is k_convert's, not a copy of it: one definition of each store function
    src = "".join(_read("wgpu_3dgs_viewer_app_amd", "csrc", n) for n in sorted(os.listdir(CSRC)) if n.endswith((".h", ".hip", ".cpp")))
    for fn in ("store_cov", "store_sh", "store_aos_geometry", "ddot3", "store_gaussian"):
        assert len(re.findall(r"__device__ inline \w+ " + fn + r"\(", src)) == 1, fn
    math_h = _read("wgpu_3dgs_viewer_app_amd", "csrc", "import_math.h")
    assert "hip/" not in math_h and "expf" not in math_h.replace("float32 expf", "")  # no libm float32 exponential in §15


# ---- csrc/import_math.h against the yardstick ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("import") / "import_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "import_driver.cpp"), "-o", exe])
    return exe


def _run(driver, text, answers):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[:4000]  # (stderr: a sanitizer report)
    lines = r.stdout.splitlines()
    assert len(lines) == answers
    return lines


def _play(driver, layout, v, mode="r"):
    """the driver's records of the values v written as rows of `layout`"""
    stride, offsets = R.layout_header(layout)
    rows = R.ply_rows(layout, v)
    text = f"h {stride} " + " ".join(str(o) for o in offsets) + "\n" + "".join(f"{mode} {row.tobytes().hex()}\n" for row in rows)
    lines = _run(driver, text, rows.shape[0])
    assert all(ln[0] == mode for ln in lines)
    words = np.array([[int(t, 16) for t in ln.split()[1:]] for ln in lines], np.uint32).reshape(-1, 56)
    return np.frombuffer(words.tobytes(), scene.GAUSSIAN_DTYPE)


def _same_or_both_nan(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def test_the_generator_respects_its_bands():
    v = R.rows(20000, 1)
    assert not R.in_bands(v).any()
    assert R.scale_band_distance(v[:, 55:58]).min() >= R.SCALE_BAND and R.alpha_band_distance(v[:, 54]).min() >= R.ALPHA_BAND
    assert np.array_equal(v, R.rows(20000, 1)) and not np.array_equal(v[:100], R.rows(100, 2))  # seeded
    # the bands are not vacuous: a value on a midpoint is inside the first, alpha * 255 = 127.5 inside the second
    assert R.alpha_band_distance(F(0.0)) < R.ALPHA_BAND and R.scale_band_distance(F(0.0)) >= R.SCALE_BAND
    # (the clamp of the colour is exercised at both ends)
    g = R.records(v)
    assert (g["color"][:, :3] == 0).any() and (g["color"][:, :3] == 255).any() and (g["color"][:, 3] > 0).any()


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_records_are_the_yardsticks_bit_for_bit(driver, name):
    layout = R.LAYOUTS[name]()
    v = R.rows(1500, 20 + len(name))
    want = R.records(R.dropped(layout, v))
    stride, offsets = R.layout_header(layout)
    assert {"canonical": (248, True), "reordered": (268, True), "leading_uchar": (249, False), "short_rest": (164, True)}[name] == (
        stride, all(o % 4 == 0 for o in offsets if o >= 0))
    if name == "short_rest":
        # f_rest[ch * 15 + c] from 24 on is absent: channel 1 from coefficient 9 on, all of channel 2
        assert not want["sh"][:, :, 2].any() and not want["sh"][:, 9:, 1].any() and want["sh"][:, :, 0].all() and want["sh"][:, :9, 1].all()
    assert _play(driver, layout, v).tobytes() == want.tobytes()
    assert _play(driver, layout, v[:200], "b").tobytes() == want[:200].tobytes()  # the byte fetch of the same rows


def test_specials(driver):
    v = R.specials()
    want = R.records(v)
    got = _play(driver, R.canonical_layout(), v)
    for field in ("pos", "sh", "color"):  # carried bits, and bytes
        assert got[field].tobytes() == want[field].tobytes(), field
    assert _same_or_both_nan(got["rot"], want["rot"]) and _same_or_both_nan(got["scale"], want["scale"])
    # the table says what it means to
    inf = F(np.inf)
    assert want["scale"][0, 0] == inf and want["scale"][1, 0] == 0 and np.isnan(want["scale"][2, 0]) and want["scale"][3, 0] == inf and want["scale"][4, 0] == 0
    assert list(want["color"][15:22, 3]) == [255, 0, 0, 255, 0, 128, 128]  # opacity +inf, -inf, NaN, 100, -100, 0, -0
    ident = np.array([0, 0, 0, 1], F)
    assert np.array_equal(want["rot"][22], ident) and np.array_equal(want["rot"][23], ident) and np.array_equal(want["rot"][26], ident)
    assert np.isfinite(want["rot"][24]).all() and abs(np.linalg.norm(want["rot"][24].astype(np.float64)) - 1) < 1e-6  # a subnormal sum of squares
    assert all(np.array_equal(want["rot"][27 + k], ident) for k in range(4))  # a NaN component: len is NaN
    assert list(want["color"][35:40, 0]) == [0, 255, 0, 255, 0]  # f_dc NaN, 1e30, -1e30, inf, -inf
    assert np.isnan(want["pos"][50, 0]) and want["pos"][51, 0] == inf


def test_against_the_host_reader(driver):
    """pos, rot, sh and the rgb bytes are the host reader's bits; scale is within 1 float32 ulp of its expf, the alpha byte within 1."""
    for name in R.LAYOUTS:
        layout = R.LAYOUTS[name]()
        v = R.rows(3000, 31)
        data = R.ply_bytes(layout, v)
        host = ply.Gaussians.read_ply(data).gaussians
        got = _play(driver, layout, v)
        for field in ("pos", "rot", "sh"):
            assert got[field].tobytes() == host[field].tobytes(), (name, field)
        assert np.array_equal(got["color"][:, :3], host["color"][:, :3]), name
        ulp = np.abs(got["scale"].view(np.int32).astype(np.int64) - host["scale"].view(np.int32).astype(np.int64))
        alpha = np.abs(got["color"][:, 3].astype(np.int64) - host["color"][:, 3].astype(np.int64))
        print(f"{name}: scale differs on {int((ulp > 0).sum())} of {ulp.size} (worst {int(ulp.max())} ulp), alpha on {int((alpha > 0).sum())}")
        assert ulp.max() <= 1 and alpha.max() <= 1


def test_header_validation(driver):
    stride, offsets = R.layout_header(R.canonical_layout())

    def verdict(is_ascii, vb, offs):
        ln = _run(driver, f"c {is_ascii} {vb} " + " ".join(str(o) for o in offs) + "\n", 1)[0].split()
        return int(ln[1]), int(ln[2])

    assert verdict(0, stride, offsets) == (0, -1)
    assert verdict(0, 249, [o + 1 for o in offsets]) == (0, -1)  # unaligned offsets are legal
    assert verdict(0, 1024, offsets) == (0, -1)
    assert verdict(1, 62, list(range(62)))[0] == 1                # ascii: unsupported
    assert verdict(0, 1025, offsets)[0] == 1                      # a stride above 1024: unsupported
    assert verdict(0, 0, offsets)[0] == 2                         # stride 0
    past = list(offsets)
    past[61] = stride - 3                                         # the last byte of rot_3 would lie past the row
    assert verdict(0, stride, past) == (2, 61)
    past[61] = stride
    assert verdict(0, stride, past) == (2, 61)
    neg = list(offsets)
    neg[10] = -2                                                  # neither -1 nor an offset
    assert verdict(0, stride, neg) == (2, 10)
    neg[10] = -1                                                  # f_rest_1 absent: fine
    assert verdict(0, stride, neg) == (0, -1)
    for req in R.REQUIRED:
        lacks = list(offsets)
        lacks[req] = -1
        assert verdict(0, stride, lacks) == (2, req)
    assert verdict(0, stride, [2 ** 31 - 1 if k == 5 else o for k, o in enumerate(offsets)]) == (2, 5)
