"""Model transform (gsx_model_apply_transform, spec §21) without a device: the entry points in the header, the library, the bindings
and the facades; and the rules of csrc/transform_math.h — the mode of a transform, its validity, the position formula with its
pivot rule — played by tests/transform_driver.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers
and run as a child process, against the numpy restatement tests/transform_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import transform_ref as T
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- facades --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^gsx_status gsx_model_apply_transform\(gsx_viewer\* v, const char\* key, const gsx_transform_desc\* desc, "
                     r"uint64_t\* out_count /\* nullable \*/\);", hdr, re.M)
    assert re.search(r"^void gsx_transform_desc_default\(gsx_transform_desc\* d\);", hdr, re.M)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # (additive: the version stays)


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for name in ("gsx_model_apply_transform", "gsx_transform_desc_default"):
        assert hasattr(L, name) and name in _lib.EXPORTS
        assert f"pub fn {name}(" in rust_sys
    assert re.search(r"pub fn gsx_model_apply_transform\(v: \*mut gsx_viewer, key: \*const c_char, desc: \*const gsx_transform_desc, "
                     r"out_count: \*mut u64\) -> gsx_status;", rust_sys)
    assert re.search(r"pub struct gsx_transform_desc \{\s*pub filter: u32, pub flags: u32, pub pos: \[f32; 3\], pub quat: \[f32; 4\], "
                     r"pub scale: \[f32; 3\], pub pivot: \[f32; 3\], pub reserved: u32,\s*\}", rust_sys)
    assert "pub fn apply_transform(" in rust and "sys::gsx_model_apply_transform(" in rust
    assert re.search(r"uint64_t apply_transform\(", hpp) and "gsx_model_apply_transform(" in hpp
    # without a device: a status code and a message, not a crash
    desc, count = _lib.TransformDesc(), C.c_uint64(99)
    L.gsx_transform_desc_default(C.byref(desc))
    assert L.gsx_model_apply_transform(None, b"a", C.byref(desc), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_apply_transform" in L.gsx_last_error_string()
    L.gsx_transform_desc_default(None)  # (a null desc is ignored)
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert callable(MultiModelViewerModel.apply_transform)


def test_the_desc_is_64_bytes_and_the_default_is_the_identity():
    assert C.sizeof(_lib.TransformDesc) == 64
    desc = _lib.TransformDesc()
    C.memset(C.byref(desc), 0xAB, 64)
    _lib.load().gsx_transform_desc_default(C.byref(desc))
    want = np.zeros(16, np.uint32)
    want[2:15] = np.float32([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]).view(np.uint32)  # pos 0, quat (0, 0, 0, 1), scale 1, pivot 0
    assert bytes(desc) == want.tobytes()
    assert (desc.filter, desc.flags, desc.reserved) == (0, 0, 0)
    assert T.mode(desc.pos[:], desc.quat[:], desc.scale[:]) == T.IDENTITY


# ---- csrc/transform_math.h against the numpy restatement ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("transform") / "transform_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "transform_driver.cpp"), "-o", exe])
    return exe


def _hex(floats):
    return " ".join(f"{int(b):08x}" for b in np.asarray(floats, np.float32).reshape(-1).view(np.uint32))


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report)
    return [ln.split() for ln in r.stdout.splitlines()]


def test_the_driver_sees_the_same_desc(driver):
    assert _play(driver, "desc\n") == [["desc", "64", "0", "4", "8", "20", "36", "48", "60"]]
    f = _lib.TransformDesc
    assert [getattr(f, k).offset for k in ("filter", "flags", "pos", "quat", "scale", "pivot", "reserved")] == [0, 4, 8, 20, 36, 48, 60]


def test_mode_classification(driver):
    one_up = np.nextafter(np.float32(1), np.float32(2))
    z, o = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    cases = [  # pos, quat, scale -> mode, the rotation is the identity
        (z, [0, 0, 0, 1], o, T.IDENTITY, 1), (z, [0, 0, 0, -1], o, T.IDENTITY, 1), ([-0.0, 0.0, -0.0], [-0.0, 0.0, -0.0, 1], o, T.IDENTITY, 1),
        ([0.5, 0, 0], [0, 0, 0, 1], o, T.TRANSLATE, 1), ([0, 0, 1e-30], [-0.0, 0, 0, -1], o, T.TRANSLATE, 1),
        (z, [0, 0, 0, 1], [2, 1, 1], T.NO_ROTATION, 1), (z, [0, 0, 0, -1], [1, -1, 1], T.NO_ROTATION, 1), ([1, 2, 3], [0, 0, 0, 1], [1, one_up, 1], T.NO_ROTATION, 1),
        # the identity only after normalisation: NOT the identity rotation as float32 values
        (z, [0, 0, 0, 2], o, T.FULL, 0), (z, [0, 0, 0, one_up], o, T.FULL, 0), (z, [0, 0, 0, 0.5], o, T.FULL, 0),
        (z, [1e-30, 0, 0, 1], o, T.FULL, 0), (z, [1, 0, 0, 0], o, T.FULL, 0), ([1, 0, 0], [0.5, 0.5, 0.5, 0.5], [2, 2, 2], T.FULL, 0),
    ]
    out = _play(driver, "".join(f"mode {_hex(p)} {_hex(q)} {_hex(s)}\n" for p, q, s, _, _ in cases))
    assert len(out) == 2 * len(cases)
    for k, (p, q, s, mode, rot) in enumerate(cases):
        assert (out[2 * k], out[2 * k + 1]) == (["mode", str(mode)], ["rot", str(rot)]), (p, q, s)
        assert T.mode(p, q, s) == mode and T.rotation_is_identity(q) == bool(rot)
    # What moves positions and covariances is the matrix of the quaternion AS GIVEN.  For (0, 0, 0, 2) that matrix happens to be the
    # identity (w enters only through products with x, y, z), yet the mode is full: the planes are rewritten, the SH through the
    # matrices of the normalised quaternion.  For (0, 0, 1, 1) — a quarter turn about z once normalised — it is no rotation at all.
    assert np.array_equal(T.quat_rows([0, 0, 0, 2]), np.eye(3, dtype=np.float32))
    assert np.array_equal(T.quat_rows([0, 0, 0, -1]), np.eye(3, dtype=np.float32))
    assert np.array_equal(T.quat_rows([0, 0, 1, 1]), np.float32([[-1, -2, 0], [2, -1, 0], [0, 0, 1]]))


def test_validity(driver):
    z, o, q1 = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 0, 0, 1]
    cases = [  # pos, quat, scale, pivot -> valid, the pivot is zero
        (z, q1, o, z, 1, 1), (z, q1, o, [-0.0, 0.0, -0.0], 1, 1), (z, q1, o, [0, 1e-45, 0], 1, 0), ([1, 2, 3], [1, 2, 3, 4], [1, -1, 0], [5, 6, 7], 1, 0),
        (z, q1, o, [np.nan, 0, 0], 0, 0), (z, q1, o, [0, np.inf, 0], 0, 0), (z, q1, o, [0, 0, -np.inf], 0, 0),
        ([np.inf, 0, 0], q1, o, z, 0, 1), ([0, np.nan, 0], q1, o, z, 0, 1), (z, [0, np.nan, 0, 1], o, z, 0, 1), (z, [0, 0, 0, np.inf], o, z, 0, 1),
        (z, q1, [1, np.nan, 1], z, 0, 1), (z, q1, [1, 1, -np.inf], z, 0, 1), (z, [0, 0, 0, 0], o, z, 0, 1), (z, [-0.0, 0, 0, -0.0], o, z, 0, 1),
        (z, [1e-30, 0, 0, 0], o, z, 1, 1),  # tiny but not zero: its float64 norm is a number
    ]
    out = _play(driver, "".join(f"valid {_hex(p)} {_hex(q)} {_hex(s)} {_hex(c)}\n" for p, q, s, c, _, _ in cases))
    assert len(out) == 2 * len(cases)
    for k, (p, q, s, c, valid, zero) in enumerate(cases):
        assert (out[2 * k], out[2 * k + 1]) == (["valid", str(valid)], ["pivot0", str(zero)]), (p, q, s, c)
        assert T.is_valid(p, q, s, c) == bool(valid)


def _positions(driver, points, pos, quat, scale, pivot):
    text = f"xf {_hex(T.quat_rows(quat))} {_hex(scale)} {_hex(pos)} {_hex(pivot)}\n" + "".join(f"p {_hex(p)}\n" for p in points)
    out = _play(driver, text)
    assert len(out) == len(points) and all(ln[0] == "o" for ln in out)
    return np.array([[int(h, 16) for h in ln[1:]] for ln in out], np.uint32).view(np.float32)


@pytest.mark.parametrize("pivot", [(0.0, 0.0, 0.0), (0.7, -1.9, 0.3), (-0.0, 0.0, 0.0)], ids=["pivot0", "pivot", "pivot-0"])
def test_position_formula_bit_for_bit(driver, pivot):
    rng = np.random.default_rng(21)
    q = rng.normal(size=4)
    quat, pos, scale = (q / np.linalg.norm(q)).astype(np.float32), np.float32([0.3, -0.2, 0.5]), np.float32([1.3, -0.7, 0.9])
    points = (rng.normal(size=(1000, 3)) * 3).astype(np.float32)
    points[5] = [np.inf, 0.5, -0.25]  # a non-finite coordinate goes through the same formula
    points[6] = [0.1, np.nan, 0.2]
    points[7] = [-np.inf, np.inf, 1e38]
    points[8] = [3e38, 3e38, -3e38]  # (overflows on the way)
    got = _positions(driver, points, pos, quat, scale, pivot)
    want = T.position(points, pos, quat, scale, pivot)
    assert got.tobytes() == want.tobytes()
    assert np.isfinite(want[9:]).all() and not np.isfinite(want[5:9]).all(axis=1).any()
    without = T.position(points, pos, quat, scale)
    if any(pivot):  # (the pivot matters)
        assert np.abs(want[9:].astype(np.float64) - without[9:]).max() > 0.1
    else:  # a pivot of -0 is the zero pivot
        assert want.tobytes() == without.tobytes()


def test_signed_zeros(driver):
    """Without a pivot nothing is added to the sum of the products: a result of -0 stays -0 (with the pivot's final + c it cannot:
    x + c is +0 only for x = -c).  Under a pure mirror the rows are single products, the other two being zeros of either sign."""
    ident, z3, one = np.float32([0, 0, 0, 1]), np.zeros(3, np.float32), np.ones(3, np.float32)
    points = np.float32([[0.0, -0.0, 1.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-1.0, 0.0, -0.0]])
    for pos, quat, scale, pivot in ((np.float32([-0.0, -0.0, -0.0]), ident, np.float32([1, -1, 1]), z3), (z3, np.float32([0, 0, 0, -1]), np.float32([-1, -1, -1]), z3),
                                    (np.float32([-0.0, 0.0, -0.0]), np.float32([1, 0, 0, 0]), one, z3), (z3, ident, np.float32([2, 2, 2]), np.float32([1.0, 0.0, 0.0]))):
        got = _positions(driver, points, pos, quat, scale, pivot)
        want = T.position(points, pos, quat, scale, pivot)
        assert got.tobytes() == want.tobytes(), (pos, quat, scale, pivot)
    # and a -0 does arise: p = (-0, -0, -0) under t = -0 and scale 1 keeps every sign
    keep = T.position(points[1:2], np.float32([-0.0, -0.0, -0.0]), ident, one)
    assert np.signbit(keep).all() and np.signbit(_positions(driver, points[1:2], np.float32([-0.0, -0.0, -0.0]), ident, one, z3)).all()
