"""Model merge (gsx_model_merge, spec §13) without a device: the entry point in the header, the library, the bindings and the
facades; and the arithmetic of csrc/merge_math.h — the SH rotation matrices, the joint word of the `edited` plane, the identity
test — played by tests/merge_driver.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers and run as
a child process, against the numpy restatement tests/merge_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import extract_ref as X
from tests import merge_ref as R
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_point():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^gsx_status gsx_model_merge\(gsx_viewer\* v, const char\* const\* src_keys, uint32_t n_src, const char\* dst_key,\s*"
                     r"const gsx_extract_desc\* desc, uint64_t\* out_counts /\* n_src entries, nullable \*/, uint64_t\* out_total\);", hdr, re.M)
    assert re.search(rf"^#define GSX_MERGE_MAX_SOURCES {R.MAX_SOURCES}u\b", hdr, re.M) and _lib.GSX_MERGE_MAX_SOURCES == R.MAX_SOURCES
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3  # (as the extract left it)
    assert re.search(rf"kMergeMaxSources = {R.MAX_SOURCES};", _read("wgpu_3dgs_viewer_app_amd", "csrc", "merge_math.h"))


def test_entry_point_is_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys = _read("rust", "gsx-sys", "src", "lib.rs")
    assert hasattr(L, "gsx_model_merge") and "gsx_model_merge" in _lib.EXPORTS
    assert re.search(r"pub fn gsx_model_merge\(v: \*mut gsx_viewer, src_keys: \*const \*const c_char, n_src: u32,", rust_sys)
    assert f"pub const GSX_MERGE_MAX_SOURCES: u32 = {R.MAX_SOURCES};" in rust_sys
    assert "pub fn merge(" in _read("rust", "gsx", "src", "lib.rs") and "sys::gsx_model_merge(" in _read("rust", "gsx", "src", "lib.rs")
    assert re.search(r"uint64_t merge\(", _read("include", "gsx.hpp")) and "gsx_model_merge(" in _read("include", "gsx.hpp")
    # without a device: a status code and a message, not a crash
    keys = (C.c_char_p * 1)(b"a")
    desc, total = _lib.ExtractDesc(0, 0), C.c_uint64(99)
    assert L.gsx_model_merge(None, keys, 1, b"b", C.byref(desc), None, C.byref(total)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_merge" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewer

    assert callable(MultiModelViewer.merge)


# ---- csrc/merge_math.h against the numpy restatement ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merge") / "merge_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "merge_driver.cpp"), "-o", exe])
    return exe


def _hex(floats):
    return " ".join(f"{int(b):08x}" for b in np.asarray(floats, np.float32).view(np.uint32))


def _play(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # (stderr: a sanitizer report or a failed self-check)
    return [ln.split() for ln in r.stdout.splitlines()]


def _quats():
    rng = np.random.default_rng(11)
    qs = [np.float32([0, 0, 0, 1]), np.float32([0, 0, 0, -1]), np.float32([1, 0, 0, 0]), np.float32([0, np.sqrt(0.5), 0, np.sqrt(0.5)]),
          np.float32([0.5, 0.5, 0.5, 0.5]), np.float32([0.3, -0.2, 0.1, 2.5])]  # (the last: far from unit length)
    for _ in range(4):
        q = rng.normal(size=4)
        qs.append((q / np.linalg.norm(q)).astype(np.float32))
    return qs


def test_sh_matrices_agree_with_the_least_squares_fit(driver):
    qs = _quats()
    out = _play(driver, "".join(f"quat {_hex(q)}\n" for q in qs))
    assert len(out) == 4 * len(qs)
    for k, q in enumerate(qs):
        M, Mf, ortho, prop = out[4 * k:4 * k + 4]
        assert (M[0], Mf[0], ortho[0], prop[0]) == ("M", "Mf", "ortho", "prop")
        got = np.array(M[1:], np.float64)
        want = R.flat_matrices(R.sh_matrices(q))
        assert got.shape == want.shape == (83,)
        assert np.abs(got - want).max() <= 1e-12, (q, np.abs(got - want).max())
        assert np.array_equal(np.array(Mf[1:], np.float32), got.astype(np.float32))  # what the kernel gets: the float64 entries, rounded once
        assert float(ortho[1]) <= 1e-12 and float(prop[1]) <= 1e-12, (q, ortho, prop)
    # the identity rotation gives identity matrices, whichever sign the quaternion has
    for k in (0, 1):
        got = np.array(out[4 * k][1:], np.float64)
        assert np.abs(got - R.flat_matrices([np.eye(3), np.eye(5), np.eye(7)])).max() <= 1e-14


def test_the_restatement_has_the_defining_property():
    """merge_ref against spec_f64.sh_color itself, at directions the fit did not see and with all 45 coefficients at once"""
    from oracle import spec_f64

    assert hasattr(_lib.load(), "gsx_model_merge")  # (the restatement is checked for the call it restates)
    rng = np.random.default_rng(5)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sh = rng.normal(size=(64, 15, 3))
    (_, rotated, _), _ = R.bake(np.zeros((64, 3)), sh.reshape(64, 45), np.zeros((64, 6)), (0, 0, 0), q, (1, 1, 1))
    Rm = R.quat_rows_f32(q)  # (a float64 unit quaternion rounded to float32: a rotation to 1e-7, which the tolerance allows for)
    a = spec_f64.sh_color(d @ Rm.T, rotated.reshape(64, 15, 3), 3)
    b = spec_f64.sh_color(d, sh, 3)
    assert np.abs(a - b).max() <= 2e-5


def test_composition(driver):
    qs = _quats()[3:]
    out = _play(driver, "".join(f"comp {_hex(a)} {_hex(b)}\n" for a in qs for b in qs))
    assert len(out) == len(qs) ** 2
    assert all(ln[0] == "comp" and float(ln[1]) <= 1e-12 for ln in out), out


@pytest.mark.parametrize("count1", [1, 31, 33, 70])
@pytest.mark.parametrize("off", [0, 1, 31, 32, 33])
def test_joint_words(driver, off, count1):
    out = dict((ln[0], ln[1:]) for ln in _play(driver, f"joint {off} {off} {count1} {off * 100 + count1}\n"))
    bits = np.array([c == "1" for c in (out["bits"][0] if out["bits"] else "")], bool)
    assert bits.size == off + count1 and (bits.any() or bits.size < 3)
    assert np.array_equal(np.array([int(w, 16) for w in out["words"]], np.uint32), X.words(bits))
    assert int(out["shared"][0]) == int(off % 32 != 0)


def test_identity_predicate(driver):
    one_up = np.nextafter(np.float32(1), np.float32(2))
    z, o = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    cases = [  # pos, quat, scale -> identity, valid
        (z, [0, 0, 0, 1], o, 1, 1), (z, [0, 0, 0, -1], o, 1, 1), ([-0.0, 0.0, -0.0], [-0.0, 0, 0, 1], o, 1, 1),
        (z, [0, 0, 0, one_up], o, 0, 1), (z, [0, 0, 0, 2], o, 0, 1), (z, [1e-30, 0, 0, 1], o, 0, 1),
        ([0, 1e-30, 0], [0, 0, 0, 1], o, 0, 1), (z, [0, 0, 0, 1], [1, one_up, 1], 0, 1), (z, [0, 0, 0, 1], [1, -1, 1], 0, 1),
        (z, [0, 0, 0, 0], o, 0, 0), (z, [0, np.nan, 0, 1], o, 0, 0), ([np.inf, 0, 0], [0, 0, 0, 1], o, 0, 0), (z, [0, 0, 0, 1], [1, np.nan, 1], 0, 0),
        (z, [1e-30, 0, 0, 0], o, 0, 1),  # tiny but not zero: its float64 norm is a number
    ]
    out = _play(driver, "".join(f"ident {_hex(p)} {_hex(q)} {_hex(s)}\n" for p, q, s, _, _ in cases))
    assert len(out) == 2 * len(cases)
    for k, (p, q, s, ident, valid) in enumerate(cases):
        assert (out[2 * k], out[2 * k + 1]) == (["ident", str(ident)], ["valid", str(valid)]), (p, q, s)
        assert R.is_identity(p, q, s) == bool(ident)
