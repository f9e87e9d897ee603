"""CPU suite (-m "not gpu"): the C oracle against the committed golden fixtures (float64 spec), oracle
self-consistency, host-side math, and the C-ABI library surface (no compute calls without a GPU)."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
from oracle import spec_f64
from tests import common
from wgpu_3dgs_viewer_app_amd import _lib, camera, scene

from tests import golden_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = golden_util.GOLDEN


@pytest.mark.parametrize("path", GOLDEN, ids=golden_util.IDS)
def test_c_oracle_matches_golden_fixture(path):
    """float32 C restatement vs the float64 spec fixture: quantised pods, mask words, projection fields (after edits) and the
    frame (<= 1e-3 L-inf).  tests/test_gpu_golden.py runs the HIP path against the same float64 arrays."""
    from wgpu_3dgs_viewer_app_amd.mask import MaskOp, pack_program
    from wgpu_3dgs_viewer_app_amd.query import default_edits

    fx = golden_util.Fixture(path)
    fb = None
    lim = None if fx.depth is None else oracle.depth_limits(fx.proj, fx.depth)
    for k in fx.paint_order:
        g = fx.gaussians(k)
        n = g.shape[0]
        pos, color, sh, cov = oracle.convert_pod(g, *fx.pod)
        fx.check_pod(k, pos, color, sh, cov)
        mp, mq, ms = fx.transform(k)
        mask = None
        if fx.mask_expr:
            mask = oracle.mask_evaluate(pos, mp, mq, ms, *pack_program(MaskOp.parse(fx.mask_expr), fx.mask_shapes()))
            tail = np.uint32((1 << (n & 31)) - 1 if n & 31 else 0xFFFFFFFF)
            ref = fx.mask_words(k).copy()
            ref[-1] &= tail
            got = mask.copy()
            got[-1] &= tail
            assert np.array_equal(got, ref), "mask words differ from the float64 spec"
        params = None
        if fx.params:
            params = oracle.SpecParams.default()
            for name, val in fx.params.items():
                setattr(params, name, val)
        f = oracle.frame_setup(fx.view, fx.proj, fx.w, fx.h, mp, mq, ms, size=fx.size, display_mode=fx.display_mode,
                               sh_deg=fx.sh_deg, no_sh0=fx.no_sh0, params=params)
        pr = oracle.project(f, pos, color, None if fx.pod[0] == 3 else sh, cov, mask)
        if fx.selection_words(k) is not None:
            oracle.edit_pass(pr, fx.selection_words(k), default_edits(n), fx.edit_pod(), fx.highlight if fx.highlight is not None else (0, 0, 0, 0))
        fx.check_projection(k, pr)
        idx, nvis = oracle.depth_sort(pr["key"])
        if fb is None:
            fb = oracle.new_framebuffer(f)
        oracle.rasterize(f, pr, idx, nvis, fb, lim=lim)
    fx.check_frame(fb, tight=5e-5)


def test_back_to_front_equals_front_to_back_tiles():
    g = common.small_scene(4000, 5)
    cam = camera.orbit_pose(60)
    f, pr, idx, nvis, fb = common.oracle_model_frame(g, cam, 200, 136, common.odd_transform())
    off, lst = oracle.tile_lists(f, idx, nvis, pr["rect"])
    fb2 = oracle.new_framebuffer(f)
    oracle.composite_tiles(f, pr, off, lst, fb2)
    assert np.abs(fb - fb2).max() <= 2e-6
    # tile lists: every visible splat once per tile of its rect, lists in depth order
    r = pr["rect"][idx[:nvis]].astype(np.int64)
    assert lst.size == int(((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])).sum())
    rank = np.empty(pr["key"].size, np.int64)
    rank[idx[:nvis]] = np.arange(nvis)
    seg = np.repeat(np.arange(off.size - 1), np.diff(off.astype(np.int64)))
    assert np.all(np.diff(rank[lst])[np.diff(seg) == 0] > 0)


def test_depth_sort_is_stable_and_culled_last():
    rng = np.random.default_rng(1)
    key = rng.integers(0, 50, 5000).astype(np.uint32) * np.uint32(0x01010101)
    key[rng.random(5000) < 0.2] = 0xFFFFFFFF
    idx, nvis = oracle.depth_sort(key)
    assert nvis == int((key != 0xFFFFFFFF).sum())
    assert np.array_equal(idx, np.argsort(key, kind="stable").astype(np.uint32))
    assert oracle.depth_sort(np.zeros(0, np.uint32))[1] == 0


def test_empty_and_single_inputs():
    cam = camera.orbit_pose(0)
    f = common.oracle_frame(cam, 64, 48)
    g = common.small_scene(1, 3)[:0]
    pr = oracle.project(f, *oracle.convert(g))
    assert pr["n_visible"] == 0
    fb = oracle.new_framebuffer(f)
    assert oracle.render_model(f, *oracle.convert(g), fb) == 0 and np.all(fb[..., 3] == 1)


def test_spec_params_switch_results():
    g = common.small_scene(1500, 9)
    cam = camera.orbit_pose(12)
    base = common.oracle_model_frame(g, cam, 128, 96)[4]
    sp = oracle.SpecParams.default()
    sp.max_std_dev = 2.0
    f = common.oracle_frame(cam, 128, 96, params=sp)
    pr = oracle.project(f, *oracle.convert(g))
    idx, nvis = oracle.depth_sort(pr["key"])
    fb = oracle.new_framebuffer(f)
    oracle.rasterize(f, pr, idx, nvis, fb)
    assert np.abs(fb - base).max() > 1e-3  # the cutoff is a real, switchable parameter
    ref = spec_f64.render(cam.view(), cam.projection(128 / 96), 128, 96,
                          [dict(zip(("pos", "color", "sh", "cov3d"), oracle.convert(g)))], params=dict(max_std_dev=2.0))
    assert np.abs(fb - ref).max() <= 5e-5


# ---- host-side math restated from the reference's call sites -------------------------------------
def test_glam_camera_conventions():
    cam = camera.CameraOrbitControl()  # app.rs:1188-1199 defaults: target 0, pos -Z, z 0.1..1e4, fov 60 deg
    v, p = cam.view().reshape(4, 4).T, cam.projection(16 / 9).reshape(4, 4).T
    eye = np.array([0, 0, -1, 1.0])
    assert np.allclose(v @ eye, [0, 0, 0, 1], atol=1e-6)  # camera at the view-space origin
    fwd = v @ np.array([0, 0, 0, 1.0])  # the target is 1 unit ahead: RH looks down -Z
    assert np.allclose(fwd[:3], [0, 0, -1], atol=1e-6)
    near, far = p @ np.array([0, 0, -0.1, 1]), p @ np.array([0, 0, -1e4, 1])
    assert abs(near[2] / near[3]) < 1e-6 and abs(far[2] / far[3] - 1) < 1e-4  # NDC depth in [0, 1]
    assert np.isclose(p[1, 1], 1 / np.tan(np.radians(30)), rtol=1e-6) and np.isclose(p[0, 0], p[1, 1] / (16 / 9), rtol=1e-6)
    assert p[3, 2] == -1


def test_euler_zyx_degrees_and_world_center():
    mt = camera.ModelTransform(pos=np.array([1, 2, 3], np.float32), rot=np.array([0, 0, 90], np.float32),
                               scale=np.array([2, 2, 2], np.float32))
    q = mt.quat()  # Rz(90 deg): x -> y
    assert np.allclose(camera.quat_rotate(q, [1, 0, 0]), [0, 1, 0], atol=1e-6)
    assert np.allclose(mt.world_center([1, 0, 0]), [1, 4, 3], atol=1e-5)  # quat * (center * scale) + pos, app.rs:1044
    mt2 = camera.ModelTransform(rot=np.array([30, 40, 50], np.float32))
    rx, ry, rz = [np.radians(a) for a in (30, 40, 50)]

    def R(ax, a):
        c, s = np.cos(a), np.sin(a)
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][ax]
        m[i, i], m[j, j], m[i, j], m[j, i] = c, c, -s, s
        return m

    assert np.allclose(spec_f64.quat_to_mat(mt2.quat()), R(2, rz) @ R(1, ry) @ R(0, rx), atol=1e-6)


def test_model_render_order_far_to_near():
    keys = camera.model_render_order([0, 0, -6], {"near": [0, 0, -2], "far": [0, 0, 5], "mid": [0, 0, 0]})
    assert keys == ["far", "mid", "near"]  # scene.rs:533-558: descending squared distance


def test_scene_generator_is_seeded_and_shardable():
    a = scene.synthetic_gaussians(70000, 1238, 3)
    b = scene.synthetic_gaussians(70000, 1238, 3)
    assert a.tobytes() == b.tobytes()
    c = scene.synthetic_gaussians(70000, 1238, 3, start=65000, count=3000)
    assert c.tobytes() == a[65000:68000].tobytes()
    assert np.allclose(np.linalg.norm(a["rot"], axis=1), 1, atol=1e-5)
    assert a["scale"].min() >= np.exp(-7) * 0.999 and a["scale"].max() <= np.exp(-1) * 1.001
    z = scene.synthetic_gaussians(1000, 1235, 0)
    assert not z["sh"].any()
    assert scene.GAUSSIAN_DTYPE.itemsize == 224 and scene.PLY_DTYPE.itemsize == 248


# ---- the C ABI surface --------------------------------------------------------------------------
def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "gsx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsx_[a-z0-9_]+)\s*\((?!\s*\*)", text)))  # (not the return type of a function-pointer typedef)


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    declared = _declared_symbols()
    assert sorted(_lib.EXPORTS) == declared, "binding and include/gsx.h disagree"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gsx_[a-z0-9_]+)", nm))
    assert set(declared) <= exported
    assert lib.gsx_abi_version() == _lib.GSX_ABI_VERSION
    sp = _lib.SpecParams()
    lib.gsx_spec_params_default(sp)
    assert (sp.max_std_dev, sp.low_pass, sp.alpha_max, sp.alpha_min) == pytest.approx((3.0, 0.3, 1.0, 0.0))
    d = oracle.SpecParams.default()
    assert all(getattr(sp, n) == pytest.approx(getattr(d, n)) for n, _ in _lib.SpecParams._fields_)


def test_render_option_defaults_and_struct_layout():
    """gsx_render_options as the binding sees it: the defaults the header documents, and a struct of ten 4-byte fields (ABI 2:
    frames_in_flight was appended — one frame in flight unless the caller asks for more; ABI 3: slab_shading, on by default).  No GPU needed."""
    import ctypes as C

    from wgpu_3dgs_viewer_app_amd import _lib

    lib = _lib.load()
    o = _lib.RenderOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    lib.gsx_render_options_default(C.byref(o))
    assert C.sizeof(o) == 40 and lib.gsx_abi_version() == 3
    assert (o.progressive, o.first_slab_divisor, o.min_slab, o.growth, o.speculative, o.spec_radius, o.host_verify, o.frames_in_flight, o.slab_shading) == (
        1, 16, 131072, 2, 1, 3, 0, 1, 1)
    assert abs(o.spec_margin - 0.25) < 1e-7
    header = open(os.path.join(ROOT, "include", "gsx.h")).read()
    body = header[header.index("typedef struct gsx_render_options {"):header.index("} gsx_render_options;")]
    assert [ln.split()[1].rstrip(";") for ln in body.splitlines()[1:] if ln.strip().startswith(("uint32_t", "float"))] == [
        f[0] for f in _lib.RenderOptions._fields_]
    rs = open(os.path.join(ROOT, "rust", "gsx-sys", "src", "lib.rs")).read()
    assert "pub frames_in_flight: u32" in rs and "pub slab_shading: u32" in rs and "GSX_ABI_VERSION: u32 = 3" in rs


def test_rust_sys_covers_every_symbol():
    """rust/gsx-sys/src/lib.rs (uncompiled binding source) declares every function include/gsx.h exports, and is
    what tools/gen_rust_sys.py generates from the current header (not a stale copy)."""
    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    declared = set(re.findall(r"^(?:gsx_status|void|uint32_t|uint64_t|const char\*)\s+(gsx_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M))
    assert declared == set(_lib.EXPORTS)
    path = os.path.join(ROOT, "rust", "gsx-sys", "src", "lib.rs")
    rs = open(path).read()
    in_rust = set(re.findall(r"pub fn (gsx_\w+)\(", rs))
    assert in_rust == declared, (declared - in_rust, in_rust - declared)
    before = rs
    subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_rust_sys.py")], check=True, capture_output=True)
    assert open(path).read() == before, "rust/gsx-sys/src/lib.rs is stale: run tools/gen_rust_sys.py"
    # the documents quote the count: it is the header's
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        for quoted in re.findall(r"all\s+\**(\d+)\**\s+(?:functions|symbols)", open(os.path.join(ROOT, doc)).read()):
            assert int(quoted) == len(declared), f"{doc} says {quoted} functions, include/gsx.h declares {len(declared)}"
    facade = open(os.path.join(ROOT, "rust", "gsx", "src", "lib.rs")).read()
    for name in ("MultiModelViewer", "new_with", "update_range", "preprocess", "radix_sorter", "render", "postprocess", "update_camera",
                 "update_model_transform", "update_gaussian_transform", "update_query", "update_selection_highlight",
                 "update_selection_edit_with_pod", "GaussianShDegree", "remove_model", "read_ply", "write_ply", "shard_render_frame"):
        assert name in facade, name


def test_no_cpu_fallback_without_a_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from wgpu_3dgs_viewer_app_amd.viewer import GsxError, MultiModelViewer

    with pytest.raises(GsxError) as e:
        MultiModelViewer()
    assert e.value.status == _lib.GSX_ERR_NO_DEVICE


def test_missing_rccl_is_an_error_code_not_a_crash():
    """a host without librccl gets GSX_ERR_RCCL from the first collective call (the loader's error string used to
    be built from a second dlerror() call = NULL: a segfault).  Own process: the library is looked up once per process."""
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); L.gsx_last_error_string.restype = C.c_char_p; "
            "b = (C.c_uint8 * 128)(); st = L.gsx_comm_unique_id(b); print(st, L.gsx_last_error_string().decode())")
    env = dict(os.environ, GSX_RCCL_LIBRARY="/nonexistent/librccl.so.1")
    r = subprocess.run([sys.executable, "-c", code, os.environ.get("GSX_LIB", _lib.LIB_PATH)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    st, msg = r.stdout.split(" ", 1)
    assert int(st) == _lib.GSX_ERR_RCCL and "librccl not found" in msg and "/nonexistent/librccl.so.1" in msg


def test_new_entry_points_reject_bad_arguments_without_a_device():
    """The round-3 additions of the C ABI (transports, layered shard call, buffer handles, statistics) check their arguments
    before they touch a device: status codes and messages, nothing aborts.  (What they compute is tested under -m gpu.)"""
    import ctypes as C

    L = _lib.load()
    g = C.c_void_p()
    assert L.gsx_comm_group_create(0, 0, C.byref(g)) == _lib.GSX_ERR_INVALID_ARG and b"world" in L.gsx_last_error_string()
    assert L.gsx_comm_group_create(65, 0, C.byref(g)) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_comm_group_create(3, 0, None) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_comm_group_create(3, 250, C.byref(g)) == _lib.GSX_OK and g.value
    assert L.gsx_viewer_comm_init_group(None, g, 0) == _lib.GSX_ERR_INVALID_ARG          # no viewer
    L.gsx_comm_group_destroy(g)
    L.gsx_comm_group_destroy(None)                                                       # a no-op, like free(NULL)
    n = C.c_uint64()
    assert L.gsx_buffer_retain(None) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_buffer_len(None, C.byref(n)) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_buffer_download(None, None, 0) == _lib.GSX_ERR_INVALID_ARG
    L.gsx_buffer_release(None)
    h = C.c_void_p()
    assert L.gsx_model_buffer_retain(None, b"m", 0, C.byref(h)) == _lib.GSX_ERR_INVALID_ARG
    st = _lib.ShardStats()
    assert L.gsx_shard_get_stats(None, C.byref(st), 0) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_shard_set_slot_records(None, b"m", 64) == _lib.GSX_ERR_NOT_FOUND
    assert L.gsx_shard_set_gather_root(None, 0) == _lib.GSX_ERR_INVALID_ARG
    keys = (C.c_char_p * 1)(b"m")
    mx = (C.c_uint32 * 1)(10)
    assert L.gsx_shard_render_frame_keys(None, keys, 1, mx, 1, 0.25, 3) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_shard_render_frame(None, None, 0, 1, 0.25, 3) == _lib.GSX_ERR_INVALID_ARG
    fn = _lib.COMM_FN(lambda *a: 0)
    assert L.gsx_viewer_comm_init_custom(None, 2, 0, fn, fn, None) == _lib.GSX_ERR_INVALID_ARG
    assert C.sizeof(_lib.ShardStats) == 80
    fa, fg = _lib.COMM_A2A_V_FN(lambda *a: 0), _lib.COMM_GATHER_V_FN(lambda *a: 0)
    assert L.gsx_viewer_comm_init_custom_v(None, 2, 0, fa, fg, None) == _lib.GSX_ERR_INVALID_ARG
    e = (C.c_uint32 * 3)(0, 1, 2)
    assert L.gsx_shard_set_band_edges(None, 2, e) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_shard_get_band_edges(None, 2, e) == _lib.GSX_ERR_INVALID_ARG
    assert L.gsx_shard_set_balance(None, 1) == _lib.GSX_ERR_INVALID_ARG
    hdr = open(os.path.join(ROOT, "include", "gsx.h")).read()
    body = hdr[hdr.index("typedef struct gsx_shard_stats {"):hdr.index("} gsx_shard_stats;")]
    fields = re.findall(r"(\w+)\s*(?:,\s*(\w+))?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1])
    assert [x for pair in fields for x in pair if x] == [f[0] for f in _lib.ShardStats._fields_]


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd")
    for path in glob.glob(os.path.join(pkg, "**", "*"), recursive=True):
        if path.endswith((".py", ".hip", ".cpp", ".h")):
            src = open(path).read()
            # comments may cite the oracle; code must not import, link or dlopen it
            assert not re.search(r"^\s*(import oracle|from oracle)", src, flags=re.M), path
            assert "libgsx_oracle" not in src and "#include \"../../oracle" not in src, path


# ---- mask operation grammar (src/app.rs:1660-1783) and oracle evaluation ---------------------------
def test_mask_op_grammar_precedence_and_associativity():
    from wgpu_3dgs_viewer_app_amd.mask import MaskOp, MaskOpError

    assert MaskOp.parse("") is None and MaskOp.parse("   ") is None
    assert MaskOp.parse("0").tree == ("shape", 0)
    # ! > ^ > - > & > |
    assert MaskOp.parse("0 | 1 & 2 - 3 ^ !4").tree == ("|", ("shape", 0), ("&", ("shape", 1), ("-", ("shape", 2), ("^", ("shape", 3), ("not", ("shape", 4))))))
    # left associativity of every binary operator
    assert MaskOp.parse("0 - 1 - 2").tree == ("-", ("-", ("shape", 0), ("shape", 1)), ("shape", 2))
    assert MaskOp.parse("0^1^2").tree == ("^", ("^", ("shape", 0), ("shape", 1)), ("shape", 2))
    assert MaskOp.parse(" ( 0 | 1 ) & !( 2 ) ").tree == ("&", ("|", ("shape", 0), ("shape", 1)), ("not", ("shape", 2)))
    assert MaskOp.parse("!!12").tree == ("not", ("not", ("shape", 12)))
    for bad in ("0 +", "(0", "0 1", "|0", "a", "0 - ", "()"):
        with pytest.raises(MaskOpError):
            MaskOp.parse(bad)
    op = MaskOp.parse("0 - 1")  # cfg5's mask op: box minus ellipsoid
    assert op.validate_shapes(2) is None and op.validate_shapes(1) == 1
    assert op.to_postfix() == [(0, 0), (0, 1), (3, 0)]


def test_mask_oracle_set_algebra():
    from wgpu_3dgs_viewer_app_amd.mask import MaskOp, MaskShape, MaskShapeKind, pack_program

    rng = np.random.default_rng(3)
    pos = rng.uniform(-2, 2, size=(4000, 3)).astype(np.float32)
    box = MaskShape(MaskShapeKind.Box, pos=np.array([0.2, 0, 0], np.float32), scale=np.array([1, 0.5, 1.5], np.float32))
    ell = MaskShape(MaskShapeKind.Ellipsoid, pos=np.zeros(3, np.float32), scale=np.array([1.2, 1.2, 0.8], np.float32),
                    rotation=camera.quat_from_euler_zyx(0.3, 0.2, 0.1))
    ident = ((0, 0, 0), (0, 0, 0, 1), (1, 1, 1))

    def run(expr):
        w = oracle.mask_evaluate(pos, *ident, *pack_program(MaskOp.parse(expr), [box, ell]))
        return ((w[np.arange(4000) >> 5] >> (np.arange(4000) & 31).astype(np.uint32)) & 1).astype(bool)

    a, b = run("0"), run("1")
    q = np.abs((pos - box.pos) / box.scale)
    assert np.array_equal(a, np.all(q <= 1, axis=1))
    assert 100 < b.sum() < 3000
    assert np.array_equal(run("0 | 1"), a | b) and np.array_equal(run("0 & 1"), a & b)
    assert np.array_equal(run("0 - 1"), a & ~b) and np.array_equal(run("0 ^ 1"), a ^ b)
    assert np.array_equal(run("!0"), ~a) and np.array_equal(run("!(0 | 1) | 0&1"), ~(a | b) | (a & b))
    assert run("").all()  # Reset


# ---- PLY I/O (host side of libgsx; src/app.rs:1053-1096, 897-947) ---------------------------------
def _ply_bytes(ply, order=None, ascii_=False):
    names = (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(45)]
             + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])
    flat = np.concatenate([ply["pos"], ply["n"], ply["f_dc"], ply["f_rest"], ply["opacity"][:, None], ply["scale"], ply["rot"]], 1).astype("<f4")
    idx = list(range(62)) if order is None else order
    head = "ply\nformat %s 1.0\ncomment test\nelement vertex %d\n" % ("ascii" if ascii_ else "binary_little_endian", flat.shape[0])
    head += "".join(f"property float {names[i]}\n" for i in idx) + "end_header\n"
    body = flat[:, idx]
    if ascii_:
        return head.encode() + "\n".join(" ".join(repr(float(v)) for v in row) for row in body).encode() + b"\n"
    return head.encode() + np.ascontiguousarray(body).tobytes()


def test_ply_read_matches_gaussian_from_ply_and_round_trips():
    from wgpu_3dgs_viewer_app_amd.ply import Gaussians
    from wgpu_3dgs_viewer_app_amd._lib import GsxError

    ply = scene.synthetic_ply(3000, 77, 3)
    ref = scene.gaussians_from_ply(ply)
    for data in (_ply_bytes(ply), _ply_bytes(ply, order=list(reversed(range(62)))), _ply_bytes(ply[:200], ascii_=True)):
        h = Gaussians.read_ply_header(data)
        n = h.count()
        got = Gaussians.read_ply(data).gaussians
        assert got.shape[0] == n
        r = ref[:n]
        assert np.array_equal(got["pos"], r["pos"]) and np.array_equal(got["sh"], r["sh"])
        np.testing.assert_allclose(got["rot"], r["rot"], atol=2e-7)
        np.testing.assert_allclose(got["scale"], r["scale"], rtol=3e-7)
        assert np.abs(got["color"].astype(int) - r["color"].astype(int)).max() <= 1  # exp / sigmoid last-bit rounding
    # streaming batches like the app's loader (scene.rs:341-380)
    data = _ply_bytes(ply)
    h = Gaussians.read_ply_header(data)
    parts = list(Gaussians.read_ply_gaussians(data, h, start=100, count=1000, batch=256))
    assert [p.shape[0] for p in parts] == [256, 256, 256, 232]
    assert np.array_equal(np.concatenate(parts)["pos"], ref["pos"][100:1100])
    # write -> read round trip, with a mask (write_ply's mask iterator)
    g = Gaussians(ref)
    back = Gaussians.read_ply(g.write_ply()).gaussians
    assert np.array_equal(back["pos"], ref["pos"]) and np.array_equal(back["color"], ref["color"]) and np.array_equal(back["sh"], ref["sh"])
    np.testing.assert_allclose(back["scale"], ref["scale"], rtol=1e-6)
    mask = np.random.default_rng(1).integers(0, 2**32, size=(3000 + 31) // 32, dtype=np.uint32)
    kept = ((mask[np.arange(3000) >> 5] >> (np.arange(3000) & 31).astype(np.uint32)) & 1).astype(bool)
    masked = Gaussians.read_ply(g.write_ply(mask)).gaussians
    assert masked.shape[0] == kept.sum() and np.array_equal(masked["pos"], ref["pos"][kept])
    # errors are gs::Error-style results, not crashes
    for bad in (b"plx\n", b"ply\nformat binary_big_endian 1.0\nelement vertex 1\nend_header\n", data[:400],
                b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nend_header\n0\n"):
        with pytest.raises(GsxError):
            Gaussians.read_ply(bad)
    with pytest.raises(GsxError):
        list(Gaussians.read_ply_gaussians(data[: h.raw.header_bytes + 248 * 10], h))  # truncated body -> Error::Io
    # a PLY without f_rest (SH-0 export) reads zero SH
    no_rest = _ply_bytes(ply[:50], order=[i for i in range(62) if not 9 <= i < 54])
    assert not Gaussians.read_ply(no_rest).gaussians["sh"].any()


def test_ply_large_range_converted_by_several_threads_equals_small_batches():
    """gsx_ply_read_gaussians splits a range of >= 2 x 131072 vertices over host threads: same bytes as the app's 1000-vertex batches."""
    import ctypes as C

    from wgpu_3dgs_viewer_app_amd import scene
    from wgpu_3dgs_viewer_app_amd.ply import Gaussians

    n = 3 * 131072 + 777
    g = scene.synthetic_gaussians(n, 5, 3, 0, n)
    data = Gaussians(g).write_ply_array()
    L = _lib.load()
    h = Gaussians.read_ply_header(data[:4096].tobytes())
    whole, parts = np.zeros(n, g.dtype), np.zeros(n, g.dtype)
    _lib.check(L.gsx_ply_read_gaussians(data.ctypes.data, data.size, C.byref(h.raw), 0, n, whole.ctypes.data))
    for s in range(0, n, 1000):
        m = min(1000, n - s)
        _lib.check(L.gsx_ply_read_gaussians(data.ctypes.data, data.size, C.byref(h.raw), s, m, parts[s:].ctypes.data))
    assert whole.tobytes() == parts.tobytes()
    # and a range that starts in the middle
    mid = np.zeros(2 * 131072 + 5, g.dtype)
    _lib.check(L.gsx_ply_read_gaussians(data.ctypes.data, data.size, C.byref(h.raw), 1234, mid.shape[0], mid.ctypes.data))
    assert mid.tobytes() == parts[1234:1234 + mid.shape[0]].tobytes()


def test_no_raw_stream_calls_in_the_library():
    """csrc/gsx_launch.h: a frame-level entry point may be RECORDING its kernel launches (they leave as a HIP graph when the segment
    closes), so every other stream operation, every host wait for the device and every free of device memory must close the
    segment first — the gsx::op wrappers do.  A raw hipMemcpyAsync / hipEventRecord / hipStreamSynchronize / ... in the library
    would be reordered against launches that are still in a trace; raw hipLaunchKernelGGL would bypass the trace."""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    raw = re.compile(r"(?<![A-Za-z0-9_:])hip(MemcpyAsync|Memcpy|MemsetAsync|Memset|MemsetD32Async|EventRecord|StreamWaitEvent|StreamSynchronize|"
                     r"StreamQuery|EventSynchronize|Free|LaunchKernelGGL|DeviceSynchronize)\(")
    bad = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".cpp", ".hip", ".h")) or name in ("gsx_launch.h", "gsx_graph.cpp"):
            continue
        for ln, line in enumerate(open(os.path.join(csrc, name)), 1):
            code = line.split("//")[0]
            if raw.search(code):
                bad.append(f"{name}:{ln}: {line.strip()}")
    assert not bad, "\n".join(bad)


def test_box_mask_without_division_is_the_same_verdict():
    """k_mask_evaluate decides |d / s| <= 1 as |d| <= mask_box_limit(s) (csrc/gsx_internal.h): correctly rounded float32 division,
    as the oracle and the reference's shader do it, gives the same verdict on, next to and far from the faces — normal, denormal,
    negative, zero, infinite and NaN scales."""
    rng = np.random.default_rng(11)

    def limit(s):  # restatement of mask_box_limit
        out = np.abs(s)
        out = np.where(np.isnan(s) | (s == 0), np.float32(-1), out)
        return np.where(np.isinf(out), np.float32(3.402823466e+38), out).astype(np.float32)

    s = (rng.standard_normal(400000).astype(np.float32) * np.float32(10) ** rng.integers(-44, 38, 400000).astype(np.float32)).astype(np.float32)
    s = np.concatenate([s, np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 2.0 ** -126, 2.0 ** -149, 3.4028235e38], np.float32)])
    lim = limit(s)
    a = np.abs(s)
    with np.errstate(all="ignore"):
        for k in (-3, -1, 0, 1, 3, None):
            d = a.copy() if k is not None else (rng.standard_normal(s.size).astype(np.float32) * np.float32(2) ** rng.integers(-20, 20, s.size).astype(np.float32)).astype(np.float32)
            for _ in range(abs(k or 0)):
                d = np.nextafter(d, np.float32(np.inf) if k > 0 else np.float32(0))
            for sign in (1, -1):
                dd = (d * np.float32(sign)).astype(np.float32)
                want = np.abs(dd / s) <= 1
                got = np.abs(dd) <= lim
                bad = np.flatnonzero(want != got)
                assert bad.size == 0, (k, s[bad[:4]], dd[bad[:4]])


def test_every_environment_switch_is_documented_and_placed():
    """VERDICT r5 housekeeping: every GSX_* variable libgsx reads is a row of DESIGN.md's "Environment switches" table (what it
    selects, why it stays, which test or tool uses it) — and nothing in that table has gone from the sources."""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    read = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".cpp", ".hip", ".h")):
            read |= set(re.findall(r'getenv\("(GSX_[A-Z0-9_]+)"\)', open(os.path.join(csrc, name)).read()))
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = text.index("### Environment switches")
    table = text[start:text.index("\n## ", start) if "\n## " in text[start:] else len(text)]
    rows = set(re.findall(r"^\| `(GSX_[A-Z0-9_]+)` \|", table, re.M))
    assert read - rows == set(), f"read by libgsx, not in DESIGN.md's table: {sorted(read - rows)}"
    assert rows - read == set(), f"in DESIGN.md's table, no longer read by libgsx: {sorted(rows - read)}"
    assert len(read) <= 24, "a new switch needs a reason (VERDICT r5: prune the A/B losers)"
