"""Model export (gsx_model_export, gsx_model_export_ply, spec §14) without a device: the entry points, constants and struct in the
header, the library, the bindings and the facades; and the arithmetic of csrc/export_math.h — played by tests/export_driver.cpp, a
stand-alone program built with the address and undefined-behaviour sanitizers and run as a child process — against the float64
yardstick and the canonical-form checks of tests/export_ref.py and against the library's own PLY writer."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import export_ref as X
from wgpu_3dgs_viewer_app_amd import _lib, ply, query, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points_constants_and_struct():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^void gsx_export_desc_default\(gsx_export_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_export\(gsx_viewer\* v, const char\* key, const gsx_export_desc\* desc, void\* out, "
                     r"uint64_t capacity_bytes, uint64_t\* out_count\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_export_ply\(gsx_viewer\* v, const char\* key, const gsx_export_desc\* desc, void\* out, "
                     r"uint64_t capacity, uint64_t\* out_size\);", hdr, re.M)
    for name, value in (("GSX_EXPORT_GAUSSIANS", 0), ("GSX_EXPORT_PLY_VERTICES", 1), ("GSX_EXPORT_BAKE_EDITS", 4)):
        assert re.search(rf"^#define {name}\s+{value}u\b", hdr, re.M) and getattr(_lib, name) == value
    assert re.search(r"typedef struct gsx_export_desc \{ uint32_t filter; uint32_t flags; uint32_t format; uint32_t reserved; "
                     r"uint64_t staging_bytes; \} gsx_export_desc;", hdr)
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3
    # the bake flag is neither of extract's flags
    assert _lib.GSX_EXPORT_BAKE_EDITS & (_lib.GSX_EXTRACT_INVERT | _lib.GSX_EXTRACT_DROP_EDITS) == 0


def test_ctypes_mirror_has_the_header_layout():
    assert C.sizeof(_lib.ExportDesc) == 24
    assert {f: getattr(_lib.ExportDesc, f).offset for f, _ in _lib.ExportDesc._fields_} == {
        "filter": 0, "flags": 4, "format": 8, "reserved": 12, "staging_bytes": 16}
    assert scene.GAUSSIAN_DTYPE.itemsize == 4 * X.GAUSSIAN_WORDS


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs")
    for fn in ("gsx_export_desc_default", "gsx_model_export", "gsx_model_export_ply"):
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys)
    assert "pub struct gsx_export_desc" in rust_sys
    assert all(f"pub const {n}: u32" in rust_sys for n in ("GSX_EXPORT_GAUSSIANS", "GSX_EXPORT_PLY_VERTICES", "GSX_EXPORT_BAKE_EDITS"))
    assert "pub fn export(" in rust and "sys::gsx_model_export(" in rust and "pub fn export_ply(" in rust and "sys::gsx_model_export_ply(" in rust
    hpp = _read("include", "gsx.hpp")
    assert re.search(r"std::vector<gsx_gaussian> export_gaussians\(", hpp) and "gsx_model_export(" in hpp
    assert re.search(r"std::vector<uint8_t> export_ply\(", hpp) and "gsx_model_export_ply(" in hpp
    d = _lib.ExportDesc(7, 5, 1, 9, 123)
    L.gsx_export_desc_default(C.byref(d))
    assert (d.filter, d.flags, d.format, d.reserved, d.staging_bytes) == (0, 0, 0, 0, 0)
    # without a device: a status code and a message, not a crash
    count = C.c_uint64(99)
    assert L.gsx_model_export(None, b"a", C.byref(d), None, 0, C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_export" in L.gsx_last_error_string()
    assert L.gsx_model_export_ply(None, b"a", C.byref(d), None, 0, C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_export_ply" in L.gsx_last_error_string()
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert callable(MultiModelViewerModel.export) and callable(MultiModelViewerModel.export_ply)


def test_the_shared_constants_agree_with_the_restatement():
    math_h = _read("wgpu_3dgs_viewer_app_amd", "csrc", "export_math.h")
    assert re.search(rf"kExportGaussianWords = {X.GAUSSIAN_WORDS};", math_h) and re.search(rf"kExportPlyWords = {X.PLY_WORDS};", math_h)
    assert "typedef float ExportReal;" in math_h  # the library solves in float32: the bound below is met there
    # one header writer: gsx_ply_write and gsx_model_export_ply call it
    assert _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_ply.cpp").count('"end_header\\n"') == 1
    assert "end_header" not in _read("wgpu_3dgs_viewer_app_amd", "csrc", "gsx_api_export.cpp")


# ---- csrc/export_math.h against the yardstick ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("export") / "export_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "export_driver.cpp"), "-o", exe])
    return exe


def _play(driver, mode, words):
    """words: (n, k) uint32 requests of one mode -> (n, m) uint32 answers"""
    words = np.ascontiguousarray(words, np.uint32)
    text = "".join(mode + " " + " ".join(f"{int(w):x}" for w in row) + "\n" for row in words)
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[:4000]  # (stderr: a sanitizer report)
    lines = r.stdout.splitlines()
    assert len(lines) == words.shape[0] and all(ln[0] == mode for ln in lines)
    return np.array([[int(t, 16) for t in ln.split()[1:]] for ln in lines], np.uint32)


def _solve(driver, cov, mode="s"):
    out = _play(driver, mode, np.asarray(cov, F).view(np.uint32)).view(F)
    return out[:, :4], out[:, 4:]


@pytest.mark.parametrize("name", X.FIXTURES)
def test_the_covariance_bound_and_the_canonical_form(driver, name):
    """Measured with 4000 Gaussians a family (worst error in units of 2^-24: float32 solve / float64 path): bench 15.0 / 9.3,
    log-uniform 16.4 / 11.5, spheres 14.9 / 10.1, flats 16.8 / 10.3: at most 1.64 of the float64 path, under the factor 4."""
    cov = X.fixture(name, 4000, 7)
    rot, scale = _solve(driver, cov)
    X.check_canonical(rot, scale)
    r64, s64 = X.solve_f64(cov)
    X.check_canonical(r64, s64)
    mine, yard = X.cov_err(cov, rot, scale).max(), X.cov_err(cov, r64, s64).max()
    print(f"{name}: float32 solve {mine * 2 ** 24:.1f}, float64 path {yard * 2 ** 24:.1f} (2^-24), ratio {mine / yard:.2f}")
    assert yard > 0 and mine <= X.FACTOR * yard
    # the float64 variant of the same template is no worse than the yardstick's bound either
    rd, sd = _solve(driver, cov, "d")
    X.check_canonical(rd, sd)
    assert X.cov_err(cov, rd, sd).max() <= X.FACTOR * yard


def test_the_solve_is_the_same_bits_from_run_to_run(driver):
    cov = X.fixture("loguniform", 200, 3)
    a, b = _play(driver, "s", cov.view(np.uint32)), _play(driver, "s", cov.view(np.uint32))
    assert np.array_equal(a, b)


def test_special_cases(driver):
    inf, nan = F(np.inf), F(np.nan)
    rotm = X.upload_cov(X.random_rot(np.random.default_rng(5), 2), np.array([[2.0, 2.0, 0.5], [0.3, 1.5, 1.5]], F))  # two equal eigenvalues
    cases = np.array([
        [0, 0, 0, 0, 0, 0],                      # 0 all zero
        [inf, 0.5, 0.25, 4.0, 0.125, 9.0],       # 1 an overflowed diagonal entry
        [1.0, inf, 0.0, 4.0, 0.0, 0.25],         # 2 an overflowed off-diagonal entry
        [nan, 0.0, 0.0, 4.0, 0.0, 9.0],          # 3 NaN on the diagonal
        [1.0, 0.0, nan, 4.0, 0.0, -9.0],         # 4 NaN off the diagonal, a negative diagonal entry
        [1.0, 1.5, 0.0, 1.0, 0.0, 0.5],          # 5 indefinite: eigenvalues 2.5, 0.5, -0.5
        [9.0, 0.0, 0.0, 4.0, 0.0, 1.0],          # 6 exactly diagonal, descending
        [1.0, 0.0, 0.0, 9.0, 0.0, 4.0],          # 7 exactly diagonal, unsorted
        [2.25, 0.0, 0.0, 2.25, 0.0, 2.25],       # 8 three equal
        list(rotm[0]), list(rotm[1]),            # 9, 10 two equal, rotated
        [1e-30, 0.0, 0.0, 1e-30, 0.0, 1e-38],    # 11 tiny
        [1e30, 1e29, 0.0, 1e30, 0.0, 1e28],      # 12 huge but finite
    ], F)
    rot, scale = _solve(driver, cases)
    ident = np.array([0, 0, 0, 1], F)
    assert np.array_equal(rot[0], ident) and np.array_equal(scale[0], np.zeros(3, F))
    assert np.array_equal(rot[1], ident) and np.array_equal(scale[1], np.array([inf, 2.0, 3.0], F))
    assert np.array_equal(rot[2], ident) and np.array_equal(scale[2], np.array([1.0, 2.0, 0.5], F))
    assert np.array_equal(rot[3], ident) and np.array_equal(scale[3], np.array([0.0, 2.0, 3.0], F))
    assert np.array_equal(rot[4], ident) and np.array_equal(scale[4], np.array([1.0, 2.0, 0.0], F))
    # indefinite: the negative eigenvalue gives scale 0; the other two are sqrt(2.5), sqrt(0.5)
    assert scale[5, 2] == 0 and np.allclose(scale[5, :2], np.sqrt([2.5, 0.5]), rtol=4e-7)
    assert np.array_equal(rot[6], ident) and np.array_equal(scale[6], np.array([3.0, 2.0, 1.0], F))
    assert np.array_equal(scale[7], np.array([3.0, 2.0, 1.0], F))
    assert np.array_equal(rot[8], ident) and np.array_equal(scale[8], np.array([1.5, 1.5, 1.5], F))
    finite = [0, 5, 6, 7, 8, 9, 10, 11, 12]
    X.check_canonical(rot[finite], scale[finite])
    r64, s64 = X.solve_f64(cases[[7, 9, 10, 12]])
    assert X.cov_err(cases[[7, 9, 10, 12]], rot[[7, 9, 10, 12]], scale[[7, 9, 10, 12]]).max() <= X.FACTOR * max(
        X.cov_err(cases[[7, 9, 10, 12]], r64, s64).max(), 2.0 ** -24)
    # (case 5's covariance is not reproduced: its negative part is dropped; case 11 is below float32's squares)
    assert np.allclose(X.upload_cov(rot[5:6], scale[5:6])[0], [1.25, 1.25, 0.0, 1.25, 0.0, 0.5], atol=1e-6)


# ---- row assembly against the library's PLY writer ----
def _row_requests(g, cov, has_sh=True, edits=None):
    n = g.shape[0]
    req = np.zeros((n, 65), np.uint32)
    req[:, 0:6] = np.asarray(cov, F).view(np.uint32)
    req[:, 6:9] = g["pos"].view(np.uint32)
    req[:, 9] = g["color"].astype(np.uint32) @ np.array([1, 1 << 8, 1 << 16, 1 << 24], np.uint32)
    req[:, 10] = 1 if has_sh else 0
    req[:, 11:56] = g["sh"].reshape(n, 45).view(np.uint32)
    if edits is not None:
        req[:, 56] = (edits["flag"] & 1) != 0  # the kernel bakes a record whose flag has ENABLED
        req[:, 57:65] = np.ascontiguousarray(edits).view(np.uint32).reshape(n, 8)
    return req


@pytest.fixture(scope="module")
def known():
    """Gaussians whose covariance is diagonal with distinct descending entries: rot is the identity and scale the diagonal's roots."""
    n = 64
    rng = np.random.default_rng(11)
    g = scene.synthetic_gaussians(n, 11, 3)
    d = np.sort(np.exp(rng.uniform(-8.0, 1.0, size=(n, 3))).astype(F), axis=1)[:, ::-1]
    assert (d[:, 0] > d[:, 1]).all() and (d[:, 1] > d[:, 2]).all()
    cov = np.zeros((n, 6), F)
    cov[:, 0], cov[:, 3], cov[:, 5] = d[:, 0], d[:, 1], d[:, 2]
    g["rot"] = np.array([0, 0, 0, 1], F)
    g["scale"] = np.sqrt(d)
    g["pos"][3] = [np.nan, -np.inf, -0.0]  # carried as bits
    g["color"][:4] = [[0, 255, 1, 0], [255, 0, 254, 255], [128, 127, 3, 1], [17, 200, 99, 254]]
    return g, cov


def test_rows_agree_with_the_host_writer(driver, known):
    g, cov = known
    n = g.shape[0]
    rec = _play(driver, "g", _row_requests(g, cov))
    assert rec.tobytes() == g.tobytes()
    header = f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\n".encode()
    want = ply.Gaussians(g).write_ply_array()
    assert want[: len(header)].tobytes() == header
    want = want[want.size - 248 * n:].view(np.uint32).reshape(n, 62)
    assert np.array_equal(_play(driver, "p", _row_requests(g, cov)), want)
    # an Sh None model: zeros
    z = g.copy()
    z["sh"] = 0
    assert _play(driver, "g", _row_requests(g, cov, has_sh=False)).tobytes() == z.tobytes()
    assert np.array_equal(_play(driver, "p", _row_requests(g, cov, has_sh=False)),
                          ply.Gaussians(z).write_ply_array()[-248 * n:].view(np.uint32).reshape(n, 62))
    # a zero scale writes -inf
    c0 = cov[:1].copy()
    c0[0, 5] = 0
    row = _play(driver, "p", _row_requests(g[:1], c0)).view(F)[0]
    assert row[57] == -np.inf and np.isfinite(row[55:57]).all()


def test_baked_edits_agree_with_the_host_writer(driver, known):
    g, cov = known
    n = g.shape[0]
    rng = np.random.default_rng(12)
    ed = np.zeros(n, query.EDIT_DTYPE)
    ed["flag"] = rng.choice(np.uint32([0, 1, 1, 5, 4, 2]), n)  # disabled records (0, 4, 2) change nothing; nothing here is hidden
    ed["color"] = rng.uniform(0.0, 1.2, size=(n, 3)).astype(F)
    ed["contrast"] = rng.choice(F([0.0, 0.3, -0.2]), n)
    ed["exposure"] = rng.choice(F([0.0, 0.5, -1.0]), n)
    ed["gamma"] = rng.choice(F([1.0, 2.2, 0.45]), n)
    ed["alpha"] = rng.choice(F([1.0, 0.5, 0.0, 3.0]), n)
    want = ply.Gaussians(g).write_ply_array(None, ed)[-248 * n:].view(np.uint32).reshape(n, 62)
    got = _play(driver, "p", _row_requests(g, cov, edits=ed))
    assert np.array_equal(got, want)
    assert (got[:, 6:9] != ply.Gaussians(g).write_ply_array()[-248 * n:].view(np.uint32).reshape(n, 62)[:, 6:9]).any()
    # records: color = floor(255 * clamp(x, 0, 1) + 0.5) of the same edited float colour, everything else as unedited
    rec = _play(driver, "g", _row_requests(g, cov, edits=ed))
    plain = _play(driver, "g", _row_requests(g, cov))
    assert np.array_equal(np.delete(rec, 7, axis=1), np.delete(plain, 7, axis=1))
    fdc, op = want[:, 6:9].view(F).astype(np.float64), want[:, 54].view(F).astype(np.float64)
    on = (ed["flag"] & 1) != 0
    col = rec[:, 7:8].view(np.uint8).astype(np.int64)
    assert np.array_equal(col[~on], g["color"][~on].astype(np.int64))
    # the float colour behind f_dc, to within the float32 roundings of the two conversions: one UNORM8 step at the most
    c = np.clip(fdc * 0.28209479177387814 + 0.5, 0.0, 1.0)
    assert np.abs(col[on, :3] - np.floor(255.0 * c[on] + 0.5)).max() <= 1
    a = np.clip(1.0 / (1.0 + np.exp(-op)), 0.0, 1.0)
    inner = on & (a > 2e-6) & (a < 1 - 2e-6)  # (the PLY side clamps alpha to [1e-6, 1 - 1e-6]; the record does not)
    assert np.abs(col[inner, 3] - np.floor(255.0 * a[inner] + 0.5)).max() <= 1
    assert (col[on & (ed["alpha"] == 0), 3] == 0).all()
