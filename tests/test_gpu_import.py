"""GPU: gsx_model_import_ply and gsx_model_upload_ply_rows (spec/RENDER_SPEC.md §15; csrc/kernels_import.hip, csrc/gsx_api_import.cpp).
The oracle throughout is a second model of the same pod kinds, filled by gsx_model_upload_range with the records of the numpy
yardstick tests/import_ref.py; the resident planes are compared through gsx_model_download_pod, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import import_ref as R
from tests import model_ops
from tests.model_ops import KIND_IDS, KINDS, frames as _frames, load as _load
from wgpu_3dgs_viewer_app_amd import _lib, ply
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.viewer import CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
IMP, ORA = "imp", "ora"
PLANES = ("pos", "color", "sh", "cov3d")


def _planes(v, key):
    return model_ops.pod(v, key)


def _assert_same_planes(v, a, b, what="", nan_cov=False):
    """the resident planes of models a and b, bit for bit; nan_cov: a covariance value computed from a NaN or an infinity may be any NaN"""
    for name, x, y in zip(PLANES, _planes(v, a), _planes(v, b)):
        assert x.shape == y.shape, (what, name)
        if nan_cov and name == "cov3d":
            assert ((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))).all(), (what, name)
        else:
            assert x.tobytes() == y.tobytes(), (what, name)


def _import_raw(v, key, data, flags=0, reserved=0, staging=0):
    """gsx_model_import_ply through ctypes: (status, count)"""
    buf = np.frombuffer(data, np.uint8)
    desc, count = _lib.ImportDesc(flags, reserved, staging), C.c_uint64(0xDEAD)
    st = v._L.gsx_model_import_ply(v._h, key.encode(), buf.ctypes.data, buf.size, int(v.sh), int(v.cov3d), C.byref(desc), C.byref(count))
    return st, int(count.value)


@pytest.fixture(scope="module")
def rows5000():
    v = R.rows(5000, 81)
    v.setflags(write=False)
    return v, R.records(v)


# ---- 1. the canonical file, in chunks, on every pod kind ------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_canonical_file_in_chunks(rows5000, sh, cov):
    vals, recs = rows5000
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        for n in (2500, 5000):  # staging of 1 byte is raised to 1024 rows: three chunks (the third reuses a buffer, the last partial), five
            data = R.ply_bytes(R.canonical_layout(), vals[:n])
            assert len(data) > 248 * n
            assert v.import_ply(f"{IMP}{n}", data, staging_bytes=1) == n
            assert model_ops.model_len(v, f"{IMP}{n}") == (_lib.GSX_OK, n) and len(v.models[f"{IMP}{n}"].gaussian_buffers.gaussians_buffer) == n
            _load(v, recs[:n], f"{ORA}{n}")
            _assert_same_planes(v, f"{IMP}{n}", f"{ORA}{n}", n)
        # a second import of the same bytes under another key: the same bits
        assert v.import_ply("again", data, staging_bytes=1) == 5000
        _assert_same_planes(v, "again", f"{IMP}5000", "again")
        if (sh, cov) == (ShKind.Norm8, Cov3dKind.Half):  # the default pod: the frames of the oracle model (shade records included)
            want = _frames(v, [f"{ORA}2500"])
            assert want[0][..., :3].max() > 0
            for k, (a, b) in enumerate(zip(_frames(v, [f"{IMP}2500"]), want)):
                assert np.array_equal(a, b), k


# ---- 2. default staging ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2500, 1])
def test_default_staging(rows5000, n):
    vals, recs = rows5000
    with MultiModelViewer() as v:
        assert v.import_ply(IMP, R.ply_bytes(R.canonical_layout(), vals[:n])) == n  # one chunk
        _load(v, recs[:n], ORA)
        _assert_same_planes(v, IMP, ORA, n)


# ---- 3. general layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", [(ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)], ids=["Single-Single", "Norm8-Half"])
@pytest.mark.parametrize("name", ["reordered", "leading_uchar", "short_rest"])
def test_general_layouts(name, sh, cov):
    n = 777  # seven workgroups, the last partial; reordered (stride 268) reads rows in place, the other two through the slab
    layout = R.LAYOUTS[name]()
    vals = R.rows(n, 82)
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        assert v.import_ply(IMP, R.ply_bytes(layout, vals)) == n
        _load(v, R.records(R.dropped(layout, vals)), ORA)
        _assert_same_planes(v, IMP, ORA, name)
        # in chunks too: a chunk of a stride that is no multiple of 16 still starts at an aligned staging buffer
        big = np.concatenate([vals, vals, vals])  # 2331 rows: three chunks of 1024
        assert v.import_ply("big", R.ply_bytes(layout, big), staging_bytes=1) == 3 * n
        _load(v, R.records(R.dropped(layout, big)), "bigora")
        _assert_same_planes(v, "big", "bigora", (name, "chunks"))


# ---- 4. specials -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", [(ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)], ids=["Single-Single", "Norm8-Half"])
def test_specials(sh, cov):
    vals = R.specials()
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        assert v.import_ply(IMP, R.ply_bytes(R.canonical_layout(), vals)) == 67
        _load(v, R.records(vals), ORA)
        # positions, colour bytes and SH are carried or quantised from carried bits: bit patterns, NaN included; a covariance is computed
        _assert_same_planes(v, IMP, ORA, "specials", nan_cov=True)
        pos, color, _, cov3d = _planes(v, IMP)
        assert np.isnan(pos[50, 0]) and pos[51, 0] == np.inf and np.isnan(cov3d[2]).any() and np.isinf(cov3d[0]).any()
        assert list(color[15:22] >> 24) == [255, 0, 0, 255, 0, 128, 128]  # opacity +inf, -inf, NaN, 100, -100, 0, -0
        assert list(color[35:40] & 0xFF) == [0, 255, 0, 255, 0]           # f_dc NaN, 1e30, -1e30, inf, -inf
        if cov == Cov3dKind.Single:  # scale 0 (exp of -inf, of -104) on the x axis: the covariance of rows 1 and 4 has rank 2, finite
            assert np.isfinite(cov3d[[1, 4]]).all()
        # the same rows through the general kernel (a leading uchar)
        assert v.import_ply("general", R.ply_bytes(R.leading_uchar_layout(), vals)) == 67
        _assert_same_planes(v, "general", ORA, "specials, general", nan_cov=True)


# ---- 5. gsx_model_upload_ply_rows ------------------------------------------------------------------------------------------------------
def test_upload_ply_rows_into_the_middle(rows5000):
    vals, recs = rows5000
    n, start, count = 3000, 517, 1301
    sentinel = common.small_scene(n, 83)
    layout = R.canonical_layout()
    data = R.ply_bytes(layout, vals[:count])
    header = ply.Gaussians.read_ply_header(data)
    body = np.frombuffer(data, np.uint8)[header.raw.header_bytes:]
    with MultiModelViewer() as v:
        _load(v, sentinel, IMP)
        _load(v, sentinel, ORA)
        before = [a.copy() for a in _planes(v, IMP)]
        buf = v.models[IMP].gaussian_buffers.gaussians_buffer
        buf.update_range_ply(start, b"", header)  # n = 0: nothing happens
        desc = _lib.ImportDesc(0, 0, 0)
        assert v._L.gsx_model_upload_ply_rows(v._h, IMP.encode(), n, None, 0, C.byref(header.raw), C.byref(desc)) == _lib.GSX_OK
        _assert_same_planes(v, IMP, ORA, "n = 0")
        buf.update_range_ply(start, body, header, staging_bytes=1)  # two chunks
        v.models[ORA].gaussian_buffers.gaussians_buffer.update_range(start, recs[:count])
        _assert_same_planes(v, IMP, ORA, "middle")
        for name, was, now in zip(PLANES, before, _planes(v, IMP)):  # the sentinels on either side are untouched, the range is not
            assert was[:start].tobytes() == now[:start].tobytes() and was[start + count:].tobytes() == now[start + count:].tobytes(), name
            assert was[start:start + count].tobytes() != now[start:start + count].tobytes(), name
        # the range contract of gsx_model_upload_range
        with pytest.raises(GsxError) as e:
            buf.update_range_ply(n - count + 1, body, header)
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG and "exceeds" in str(e.value)
        assert v._L.gsx_model_upload_ply_rows(v._h, b"nope", 0, body.ctypes.data, 1, C.byref(header.raw), C.byref(desc)) == _lib.GSX_ERR_NOT_FOUND
        # two calls that together cover a file equal one import of that file
        assert v.import_ply("whole", data) == count
        v.add_model("halves", count)
        hb = v.models["halves"].gaussian_buffers.gaussians_buffer
        cut = 700
        hb.update_range_ply(cut, body[248 * cut:], header)
        hb.update_range_ply(0, body[:248 * cut], header)
        _assert_same_planes(v, "halves", "whole", "halves")
        # a caller's header is checked before anything is read
        bad = _lib.PlyHeader.from_buffer_copy(header.raw)
        bad.offsets[61] = 246
        assert v._L.gsx_model_upload_ply_rows(v._h, IMP.encode(), 0, body.ctypes.data, 1, C.byref(bad), C.byref(desc)) == _lib.GSX_ERR_INVALID_ARG
        bad.offsets[61] = 244
        bad.vertex_bytes = 1028
        assert v._L.gsx_model_upload_ply_rows(v._h, IMP.encode(), 0, body.ctypes.data, 1, C.byref(bad), C.byref(desc)) == _lib.GSX_ERR_UNSUPPORTED
        assert b"gsx_ply_read_gaussians" in v._L.gsx_last_error_string()
        _assert_same_planes(v, IMP, ORA, "after the refused calls")


# ---- 6. from the device and back -------------------------------------------------------------------------------------------------------
def test_from_the_device_and_back():
    n = 2049
    with MultiModelViewer() as v:  # Single / Single
        _load(v, common.small_scene(n, 84), "src")
        assert v.models["src"].extract("cut", 0) == n
        data = v.models["cut"].export_ply()
        assert v.import_ply(IMP, data) == n
        src, back = _planes(v, "cut"), _planes(v, IMP)
        for name, a, b in list(zip(PLANES, src, back))[:3]:  # position, colour and SH: the source's bits
            assert a.tobytes() == b.tobytes(), name
        vals = np.frombuffer(data, np.uint8)[len(data) - 248 * n:].copy().view(np.float32).reshape(n, 62)
        _load(v, R.records(vals), ORA)
        _assert_same_planes(v, IMP, ORA, "round trip")
        # ... and the frames are the oracle's
        for a, b in zip(_frames(v, [IMP], poses=(5,)), _frames(v, [ORA], poses=(5,))):
            assert a[..., :3].max() > 0 and np.array_equal(a, b)


# ---- 7. beside frames in flight --------------------------------------------------------------------------------------------------------
def _lane_sequence(g, data, recs, import_at):
    """frames of model `src` on two lanes; with import_at, two frames are in flight (rendered, not downloaded) when the import is issued"""
    from wgpu_3dgs_viewer_app_amd import camera
    from wgpu_3dgs_viewer_app_amd.viewer import GaussianDisplayMode, GaussianShDegree

    frames, imported = [], None
    with MultiModelViewer() as v:
        v.set_render_options(frames_in_flight=2)
        _load(v, g, "src")
        for pose in range(1, 9):
            v.update_camera(camera.orbit_pose(pose), (model_ops.W, model_ops.H))
            v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
            v.render_frame(["src"])
            if pose in (4, 5):  # left in flight, one on each lane
                if pose == 5 and import_at:
                    assert v.import_ply(IMP, data, staging_bytes=1) == 2500
                continue
            frames.append(v.download_framebuffer())
        if not import_at:
            v.import_ply(IMP, data)
        imported = [a.tobytes() for a in _planes(v, IMP)]
        _load(v, recs, ORA)
        mine, oracle = _frames(v, [IMP]), _frames(v, [ORA])  # on the lanes too
    return frames, imported, mine, oracle


def test_import_beside_frames_in_flight(rows5000):
    vals, recs = rows5000
    g = common.small_scene(2500, 85)
    data = R.ply_bytes(R.canonical_layout(), vals[:2500])
    with_import, imported, mine, oracle = _lane_sequence(g, data, recs[:2500], True)
    without, idle, _, _ = _lane_sequence(g, data, recs[:2500], False)
    assert imported == idle
    assert len(with_import) == 6 and with_import[0][..., :3].max() > 0
    for k, (a, b) in enumerate(zip(with_import, without)):
        assert np.array_equal(a, b), k
    assert mine[0][..., :3].max() > 0
    for k, (a, b) in enumerate(zip(mine, oracle)):
        assert np.array_equal(a, b), k


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_nothing_behind(rows5000):
    vals, _ = rows5000
    n = 1500
    layout = R.canonical_layout()
    data = R.ply_bytes(layout, vals[:n])
    wide = layout + [("double", f"pad{k}") for k in range(97)] + [("int", "tail")]
    assert R.layout_header(wide)[0] == 1028
    ascii_file = R.ply_header_text(layout, 1, "ascii") + (" ".join(["0.5"] * 62) + "\n").encode()
    with MultiModelViewer() as v, MultiModelViewer() as other:
        assert v.import_ply("first", data) == n  # (the staging buffers exist from here on)
        held = viewer_mod.device_bytes()

        def refused(key, blob, status, word=None, **kw):
            st, count = _import_raw(v, key, blob, **kw)
            assert st == status, (key, st, v._L.gsx_last_error_string())
            if word:
                assert word in v._L.gsx_last_error_string(), v._L.gsx_last_error_string()
            if key != "first":
                assert model_ops.model_len(v, key)[0] == _lib.GSX_ERR_NOT_FOUND
            assert viewer_mod.device_bytes() == held, key

        refused("first", data, _lib.GSX_ERR_INVALID_ARG, b"exists")                         # a key that exists
        assert model_ops.model_len(v, "first") == (_lib.GSX_OK, n)
        refused("short", data[:-1], _lib.GSX_ERR_IO, b"truncated")                           # a file cut one byte short
        refused("ascii", ascii_file, _lib.GSX_ERR_UNSUPPORTED, b"gsx_ply_read_gaussians")
        refused("wide", R.ply_bytes(wide, vals[:4]), _lib.GSX_ERR_UNSUPPORTED, b"gsx_ply_read_gaussians")  # a stride of 1028
        refused("reserved", data, _lib.GSX_ERR_INVALID_ARG, b"reserved", reserved=1)
        refused("flags", data, _lib.GSX_ERR_INVALID_ARG, b"flag", flags=1)
        refused("magic", b"plx\n" + data[4:], _lib.GSX_ERR_PLY)                              # header errors: the reader's
        refused("lacks", R.ply_bytes([p for p in layout if p[1] != "opacity"], vals[:4]), _lib.GSX_ERR_PLY, b"opacity")
        # null arguments
        desc, count = _lib.ImportDesc(0, 0, 0), C.c_uint64()
        buf = np.frombuffer(data, np.uint8)
        L, args = v._L, (int(v.sh), int(v.cov3d))
        assert L.gsx_model_import_ply(v._h, None, buf.ctypes.data, buf.size, *args, C.byref(desc), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_import_ply(v._h, b"k", None, buf.size, *args, C.byref(desc), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_import_ply(v._h, b"k", buf.ctypes.data, buf.size, *args, None, C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_import_ply(v._h, b"k", buf.ctypes.data, buf.size, *args, C.byref(desc), None) == _lib.GSX_ERR_INVALID_ARG
        assert model_ops.model_len(v, "k")[0] == _lib.GSX_ERR_NOT_FOUND and viewer_mod.device_bytes() == held
        # a zero-vertex file: GSX_OK, count 0, no model
        st, zero = _import_raw(v, "empty", R.ply_bytes(layout, vals[:0]))
        assert (st, zero) == (_lib.GSX_OK, 0) and model_ops.model_len(v, "empty")[0] == _lib.GSX_ERR_NOT_FOUND and viewer_mod.device_bytes() == held
        assert v.import_ply("empty", R.ply_bytes(layout, vals[:0])) == 0 and "empty" not in v.models
        # a viewer with a communicator
        other.comm_init_group(CommGroup(1), 0)
        before = viewer_mod.device_bytes()
        with pytest.raises(GsxError) as e:
            other.import_ply("a", data)
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED and "communicator" in str(e.value)
        assert model_ops.model_len(other, "a")[0] == _lib.GSX_ERR_NOT_FOUND and viewer_mod.device_bytes() == before
        # the model that was there is what it was
        assert v.import_ply("second", data) == n
        _assert_same_planes(v, "first", "second", "after the errors")


def test_device_memory_returns_after_close(rows5000):
    vals, _ = rows5000
    start = viewer_mod.device_bytes()
    with MultiModelViewer() as v:
        v.import_ply(IMP, R.ply_bytes(R.canonical_layout(), vals), staging_bytes=1)
        created = viewer_mod.device_bytes()
        assert created - start >= 2 * 248 * 1024  # the two staging buffers are counted
        v.remove_model(IMP)
        assert viewer_mod.device_bytes() < created
    assert viewer_mod.device_bytes() == start
