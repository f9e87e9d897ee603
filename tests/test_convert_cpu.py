"""Model convert (gsx_model_pod_kind, gsx_model_convert, gsx_model_set_pod_kind; spec §16) without a device: the entry points and
the struct in the header, the library, the bindings and the facades; that the encoders of csrc/pod_planes.h are written once; and that
the stress values of tests/convert_ref.py reach what they are meant to reach (numpy's binary16 and a numpy statement of snorm8)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from tests import common
from tests import convert_ref as R
from wgpu_3dgs_viewer_app_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
F = np.float32
FUNCS = ("gsx_model_pod_kind", "gsx_convert_desc_default", "gsx_model_convert", "gsx_model_set_pod_kind")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points_and_struct():
    hdr = _read("include", "gsx.h")
    assert re.search(r"^gsx_status gsx_model_pod_kind\(gsx_viewer\* v, const char\* key, gsx_sh_kind\* out_sh, gsx_cov3d_kind\* out_cov3d\);", hdr, re.M)
    assert re.search(r"^typedef struct gsx_convert_desc \{ uint32_t filter; uint32_t flags; uint32_t sh; uint32_t cov3d; \} gsx_convert_desc;", hdr, re.M)
    assert re.search(r"^void gsx_convert_desc_default\(gsx_convert_desc\* d\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_convert\(gsx_viewer\* v, const char\* src_key, const char\* dst_key, const gsx_convert_desc\* desc, "
                     r"uint64_t\* out_count\);", hdr, re.M)
    assert re.search(r"^gsx_status gsx_model_set_pod_kind\(gsx_viewer\* v, const char\* key, gsx_sh_kind sh, gsx_cov3d_kind cov3d\);", hdr, re.M)
    # after the import block, in front of the selection block
    assert hdr.index("gsx_model_import_ply(") < hdr.index("gsx_model_pod_kind(gsx_viewer") < hdr.index("gsx_model_set_pod_kind(gsx_viewer") < hdr.index("GSX_EDIT_ENABLED")
    assert re.search(r"^#define GSX_ABI_VERSION 3u", hdr, re.M) and _lib.GSX_ABI_VERSION == 3
    # gsx_model_merge's comment sends sources of mixed kinds here
    merge_doc = hdr[hdr.index("model merge"):hdr.index("gsx_status gsx_model_merge(")]
    assert "mixed kinds are converted first" in merge_doc and "gsx_model_convert" in merge_doc
    assert "Model convert [BUILD-SPEC]" in _read("spec", "RENDER_SPEC.md")


def test_ctypes_mirror_has_the_header_layout():
    assert C.sizeof(_lib.ConvertDesc) == 16
    assert {f: getattr(_lib.ConvertDesc, f).offset for f, _ in _lib.ConvertDesc._fields_} == {"filter": 0, "flags": 4, "sh": 8, "cov3d": 12}


def test_entry_points_are_exported_bound_and_in_the_facades():
    L = _lib.load()
    rust_sys, rust, hpp = _read("rust", "gsx-sys", "src", "lib.rs"), _read("rust", "gsx", "src", "lib.rs"), _read("include", "gsx.hpp")
    for fn in FUNCS:
        assert hasattr(L, fn) and fn in _lib.EXPORTS
        assert re.search(r"pub fn " + fn + r"\(", rust_sys), fn
    assert "pub struct gsx_convert_desc" in rust_sys
    for fn in ("gsx_model_pod_kind", "gsx_model_convert", "gsx_model_set_pod_kind"):
        assert "sys::" + fn + "(" in rust and fn + "(" in hpp, fn
    assert "pub fn convert(" in rust and "pub fn set_pod_kind(" in rust and "pub fn pod_kind(" in rust
    assert re.search(r"uint64_t convert\(", hpp) and re.search(r"void set_pod_kind\(", hpp) and re.search(r"pod_kind\(\) const", hpp)
    d = _lib.ConvertDesc(7, 3, 2, 1)
    L.gsx_convert_desc_default(C.byref(d))
    assert (d.filter, d.flags, d.sh, d.cov3d) == (0, 0, 0, 0)
    L.gsx_convert_desc_default(None)  # (tolerated, as the other *_default calls)
    from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewerModel

    assert callable(MultiModelViewerModel.convert) and callable(MultiModelViewerModel.set_pod_kind) and isinstance(MultiModelViewerModel.pod_kind, property)


def test_null_viewer_is_an_error_with_the_functions_name():
    L = _lib.load()
    d, count, sh, cov = _lib.ConvertDesc(0, 0, 0, 0), C.c_uint64(99), C.c_int32(), C.c_int32()
    assert L.gsx_model_pod_kind(None, b"a", C.byref(sh), C.byref(cov)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_pod_kind" in L.gsx_last_error_string()
    assert L.gsx_model_convert(None, b"a", b"b", C.byref(d), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_convert" in L.gsx_last_error_string()
    assert L.gsx_model_set_pod_kind(None, b"a", 0, 0) == _lib.GSX_ERR_INVALID_ARG
    assert b"gsx_model_set_pod_kind" in L.gsx_last_error_string()


def test_one_definition_of_each_encoder():
    """The register-level encoders are pod_planes.h's; the new kernel uses them and builds no Half or Norm8 word itself.  (The upload's
    store_sh and k_merge_bake keep the builders they had: adopting the encoders changes k_merge_bake's device code)"""
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".h", ".hip", ".cpp")))
    src = {n: _read("wgpu_3dgs_viewer_app_amd", "csrc", n) for n in names}
    everything = "".join(src.values())
    for fn in ("pod_encode_sh", "pod_encode_cov", "pod_load_sh", "pod_load_cov", "pack_h2", "q_snorm8"):
        defs = [n for n in names if re.search(r"__device__ inline \w+ " + fn + r"\(", src[n])]
        assert len(re.findall(r"__device__ inline \w+ " + fn + r"\(", everything)) == 1, fn
        assert defs[0] != "kernels_convert.hip", fn
    assert [n for n in names if "pod_encode_sh(" in src[n] and "__device__ inline void pod_encode_sh(" in src[n]] == ["pod_planes.h"]
    kernel = src["kernels_convert.hip"]
    assert '#include "pod_planes.h"' in kernel
    for use in ("pod_encode_sh<", "pod_encode_cov<", "pod_load_sh<", "pod_load_cov<", "extract_group_ranks(", "stage_rows_out<"):
        assert use in kernel, use
    code = re.sub(r"//[^\n]*", "", kernel)
    assert "pack_h2(" not in code and "q_snorm8(" not in code and "__float2half" not in code and "__device__ inline" not in code
    # the builders stand where they stood, and nowhere else: store_sh (pod_store.h), k_merge_bake, and now the encoder
    users = sorted(n for n in names if re.search(r"q_snorm8\(s", re.sub(r"//[^\n]*", "", src[n])))
    assert users == ["kernels_merge.hip", "pod_planes.h", "pod_store.h"], users
    # the host side reuses gsx_model_extract's pieces
    api = src["gsx_api_convert.cpp"]
    for use in ("kept_sets(", "model_create(", "ensure_edit_buffers(", "extract_planes(", "launch_extract_scatter(", "launch_convert_kind("):
        assert use in api, use
    assert "launch_convert_kind(" in src["gsx_internal.h"] and "kernels_convert.hip" in _read("wgpu_3dgs_viewer_app_amd", "csrc", "Makefile")


# ---- the stress values are what they are meant to be (numpy's binary16 is IEEE round-to-nearest-even, as pack_h2) ----
def test_stress_values_reach_the_edges_of_both_formats():
    s = R.STRESS
    with np.errstate(over="ignore"):
        h = s.astype(np.float16)
    at = lambda v: h[np.nonzero(s == F(v))[0][0]]  # noqa: E731
    assert at(65504.0) == np.float16(65504.0) and np.isfinite(at(65504.0))       # Half's largest value
    assert np.isposinf(at(65520.0)) and np.isneginf(at(-65520.0))                   # the tie above it rounds to infinity
    assert at(65519.996) == np.float16(65504.0)                                    # the float32 just below the tie does not
    assert 0 < float(at(1e-7)) < 2.0 ** -14 and float(at(-1e-7)) < 0                # Half subnormals
    assert at(2.0 ** -24) == np.float16(2.0 ** -24) and at(2.0 ** -25) == 0 and at(6e-8) == np.float16(2.0 ** -24)  # the smallest, the tie to zero
    assert at(1e-10) == 0
    assert at(1.0 + 2.0 ** -11) == np.float16(1.0) and at(1.0 + 2.0 ** -10 + 2.0 ** -11) == np.float16(1.0 + 2.0 ** -9)  # ties go to even
    neg0 = np.nonzero((s == 0) & np.signbit(s))[0]
    assert neg0.size == 1 and np.signbit(h[neg0[0]]) and R.q_snorm8(s[neg0[0]]) == 0
    # Norm8: clamps, and ties of v * 127 + 0.5
    q = R.q_snorm8(s)
    assert q[s == F(1.5)][0] == 127 and q[s == F(-1.5)][0] == -127 and q[s == F(2.0 ** 20)][0] == 127 and q.min() == -127 and q.max() == 127
    ties = s[np.isin(s, np.array([0.5, 1.5, -0.5, -2.5, 63.5, 126.5, -126.5], F) / F(127))]
    assert ties.size == 7
    frac = (ties.astype(np.float64) * 127 + 0.5) % 1.0
    assert np.all(np.minimum(frac, 1 - frac) < 1e-5)  # each within a float32 rounding of an integer: floor decides by the last bit
    assert -128 not in q


def test_snorm8_decode_then_encode_is_the_identity():
    """Round trips Norm8 -> Single -> Norm8 rest on this: q_snorm8(dq_snorm8(q)) == q for every q an upload stores, [-127, 127];
    -128 is never stored (the clamp's lower end encodes to -127) and would decode to -1 and come back as -127."""
    q = np.arange(-127, 128, dtype=np.int32)
    assert np.array_equal(R.q_snorm8(R.dq_snorm8(q)), q)
    assert R.dq_snorm8(np.array([-128]))[0] == F(-1) and R.q_snorm8(R.dq_snorm8(np.array([-128])))[0] == -127
    # Half -> Single -> Half: decoding is exact, so encoding gives the bits back (all 63488 non-NaN patterns; NaNs stay NaNs)
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = bits.view(np.float16)
    ok = ~np.isnan(h)
    assert np.array_equal(h.astype(F).astype(np.float16).view(np.uint16)[ok], bits[ok]) and np.isnan(h.astype(F).astype(np.float16)[~ok]).all()


def test_stress_pod_places_every_value_and_the_specials():
    g = common.small_scene(1025, 3)
    pos, color, sh, cov = R.stress_pod(g, 3)
    assert pos.shape == (1025, 3) and color.shape == (1025,) and sh.shape == (1025, 45) and cov.shape == (1025, 6)
    assert all(a.dtype == F for a in (pos, sh, cov)) and color.dtype == np.uint32
    for val in R.STRESS[~np.isnan(R.STRESS)]:
        assert (sh.view(np.uint32) == val.view(np.uint32)).any(), val
        assert (cov.view(np.uint32) == val.view(np.uint32)).any(), val
    assert np.isposinf(sh).any() and np.isneginf(sh).any() and np.isposinf(cov).any() and np.isneginf(cov).any()
    assert np.isnan(sh[-1]).any() and np.isnan(cov[-1]).any() and not np.isnan(sh[:-1]).any() and not np.isnan(cov[:-1]).any()
    assert np.isfinite(pos).all() and np.array_equal(R.stress_pod(g, 3)[2].view(np.uint32), sh.view(np.uint32))  # seeded
