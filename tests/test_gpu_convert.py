"""GPU: gsx_model_convert, gsx_model_set_pod_kind and gsx_model_pod_kind (spec/RENDER_SPEC.md §16; csrc/kernels_convert.hip,
csrc/gsx_api_convert.cpp).  The yardstick is the library's existing quantiser: a converted model must hold the bits that
gsx_model_upload_pod_device leaves in a fresh model of the destination kind for the planes gsx_model_download_pod returns of the
source's kept Gaussians (tests/convert_ref.py: upload_pod, pod); no arithmetic is restated.  Device bytes are read as the extract and
merge tests read them: the planes through the exact dequantisation of gsx_model_download_pod (equal only if the stored bits are), the
edit records through the edit buffer and its retained raw snapshot, the shade records through the later, speculated frames of a camera
path, which shade from them."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import convert_ref as R
from tests import extract_ref as X
from tests.model_ops import H, KIND_IDS, KINDS, W, frames as _frames, load as _load
from wgpu_3dgs_viewer_app_amd import _lib, query, scene
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as F
from wgpu_3dgs_viewer_app_amd.viewer import BufferHandle, CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
F32, N8H = (ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)
BIG = 263169  # the size tests/test_gpu_extract.py's edge test ends with: the scan of the partials takes more than one pass
PAIRS = [(s, d) for s in KINDS for d in KINDS]
PAIR_IDS = [f"{a}->{b}" for a in KIND_IDS for b in KIND_IDS]


def _id(kind):
    return f"{kind[0].name}-{kind[1].name}"


def _edits(v, key):
    return v.models[key].gaussian_buffers.gaussians_edit_buffer.download()


def _len_status(v, key):
    n = C.c_uint64()
    return v._L.gsx_model_len(v._h, key.encode(), C.byref(n))


def _edit_records(n, seed, hide=True):
    rng = np.random.default_rng(seed)
    e = query.default_edits(n)
    e["flag"][0::3] = int(F.ENABLED | F.HIDDEN) if hide else int(F.ENABLED | F.OVERRIDE_COLOR)
    e["flag"][1::3] = int(F.ENABLED)
    e["flag"][5::7] |= int(F.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    e["color"][:, 0] = rng.random(n).astype(np.float32)
    e["contrast"] = rng.random(n).astype(np.float32)
    return e


# ---- 1. every ordered pair of kinds, on stress values -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stress():
    """1025 Gaussians (two workgroups, the second with one Gaussian) whose SH and covariances hold tests/convert_ref.py's stress
    values, +-inf and, in the last Gaussian, NaN.  Never written to."""
    p = R.stress_pod(common.small_scene(1025, 61), 61)
    for a in p:
        a.setflags(write=False)
    return p


@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
def test_every_ordered_pair_holds_what_an_upload_stores(stress, src, dst):
    n = stress[0].shape[0]
    with MultiModelViewer(sh=src[0], cov3d=src[1]) as a, MultiModelViewer(sh=dst[0], cov3d=dst[1]) as b:
        R.upload_pod(a, "src", stress)  # (quantised into the source kind by the upload)
        assert a.models["src"].convert("c", *dst) == n
        assert R.pod_kind(a, "src") == src and R.pod_kind(a, "c") == dst and a.models["c"].pod_kind == dst
        held = R.pod(a, "src")  # zeros for the SH of an Sh None source
        R.upload_pod(b, "want", held)
        got = R.pod(a, "c")
        R.same_bytes(got, R.pod(b, "want"), f"{_id(src)} -> {_id(dst)}")
        # position and colour word: the stored bits
        assert got[0].tobytes() == stress[0].tobytes() and got[1].tobytes() == stress[1].tobytes()
        if dst[0] == ShKind.Remove or src[0] == ShKind.Remove:
            assert not got[2].view(np.uint32).any()
        elif src[0] == ShKind.Single and dst[0] == ShKind.Single:
            assert got[2].tobytes() == stress[2].tobytes()  # NaN payloads and -0.0 included
        if src[1] == Cov3dKind.Single and dst[1] == Cov3dKind.Single:
            assert got[3].tobytes() == stress[3].tobytes()
        # the same bits on every call
        assert a.models["src"].convert("again", *dst) == n
        R.same_bytes(R.pod(a, "again"), got, "second call")
        R.same_bytes(R.pod(a, "src"), held, "src is not written")


# ---- 2. frames: the shade records agree with the planes -----------------------------------------------------------------------------
@pytest.mark.parametrize("src", [F32, N8H], ids=_id)
@pytest.mark.parametrize("dst", KINDS, ids=KIND_IDS)
def test_frames_of_the_converted_model(src, dst):
    """A model's first frame shades from the SoA planes; the later frames of a camera path are speculated and shade from the shade
    records (16, 12 and 8 words a record: two staging passes of 8, one pass of 12, one pass of 8)."""
    n = 2500
    g = common.small_scene(n, 62)
    with MultiModelViewer(sh=src[0], cov3d=src[1]) as a, MultiModelViewer(sh=dst[0], cov3d=dst[1]) as b:
        _load(a, g)
        assert a.models["src"].convert("c", *dst) == n
        R.upload_pod(b, "want", R.pod(a, "src"))
        got, want = _frames(a, ["c"]), _frames(b, ["want"])
        assert want[0][..., :3].max() > 0 and not np.array_equal(want[0], want[2])
        for k, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), (k, float(np.abs(x - y).max()))


# ---- 3. the diagonal is extract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_the_same_kind_is_extract(sh, cov):
    n = 2500
    g = common.small_scene(n, 63)
    rng = np.random.default_rng(63)
    flt = X.MASKED | X.SKIP_HIDDEN | X.SELECTED
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        bufs = v.models["src"].gaussian_buffers
        bufs.mask_buffer.upload(X.words(rng.random(n) < 0.6, True))
        bufs.selection_buffer.upload(X.words(rng.random(n) < 0.7, True))
        bufs.gaussians_edit_buffer.upload(_edit_records(n, 63))
        count = v.models["src"].extract("x", flt)
        assert v.models["src"].convert("c", sh, cov, flt) == count and 0 < count < n
        assert R.pod_kind(v, "c") == (sh, cov)
        R.same_bytes(R.pod(v, "c"), R.pod(v, "x"))
        assert _edits(v, "c").tobytes() == _edits(v, "x").tobytes() and (_edits(v, "c")["flag"] != 0).any()
        assert BufferHandle(v, "c", "edits").download().tobytes() == BufferHandle(v, "x", "edits").download().tobytes()
        want = _frames(v, ["x"])
        assert want[0][..., :3].max() > 0
        for x, y in zip(_frames(v, ["c"]), want):
            assert np.array_equal(x, y)


# ---- 4. kept sets and joints ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One SH-0 scene; the sources are its prefixes.  Never written to."""
    g = scene.synthetic_gaussians(BIG, 91, 0)
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("n", [1, 31, 33, 1023, 1025, BIG])
@pytest.mark.parametrize("src,dst", [(F32, N8H), (N8H, F32)], ids=["f32->Norm8-Half", "Norm8-Half->f32"])
def test_kept_sets_and_joints(big, src, dst, n):
    rng = np.random.default_rng(n)
    keep = rng.random(n) < 0.6
    keep[0] = True
    kept = np.nonzero(keep)[0]
    with MultiModelViewer(sh=src[0], cov3d=src[1]) as a, MultiModelViewer(sh=dst[0], cov3d=dst[1]) as b:
        _load(a, big[:n])
        m = a.models["src"]
        m.gaussian_buffers.mask_buffer.upload(X.words(keep, True))  # garbage above n
        m.gaussian_buffers.selection_buffer.upload(X.words(~keep, True))
        m.gaussian_buffers.gaussians_edit_buffer.upload(_edit_records(n, n, hide=False))
        held, src_edits, src_raw = R.pod(a, "src"), _edits(a, "src"), BufferHandle(a, "src", "edits").download()

        def state():
            bufs = m.gaussian_buffers
            return [x.tobytes() for x in R.pod(a, "src")] + [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(),
                                                             bufs.gaussians_edit_buffer.download().tobytes()]

        before = state()
        small = n <= 1025
        if small:
            first = _frames(a, ["src"], poses=(5,), sh_deg=0)[0]

        def check(key, idx, want_edits, what):
            assert R.model_len(a, key) == idx.size and R.pod_kind(a, key) == dst
            R.upload_pod(b, "want_" + key, R.rows(held, idx))
            R.same_bytes(R.pod(a, key), R.pod(b, "want_" + key), what)
            assert _edits(a, key).tobytes() == want_edits.tobytes(), what
            bufs = a.models[key].gaussian_buffers
            assert np.all(bufs.mask_buffer.download() == 0xFFFFFFFF) and not bufs.selection_buffer.download().any()

        assert m.convert("c", *dst, X.MASKED) == kept.size
        check("c", kept, src_edits[kept], "masked")
        assert BufferHandle(a, "c", "edits").download().tobytes() == src_raw[kept].tobytes()
        rest = np.nonzero(~keep)[0]
        assert m.convert("ci", *dst, X.MASKED, invert=True) == rest.size
        if rest.size:
            check("ci", rest, src_edits[rest], "inverted")
        else:
            assert "ci" not in a.models and _len_status(a, "ci") == _lib.GSX_ERR_NOT_FOUND
        assert m.convert("cd", *dst, X.MASKED, drop_edits=True) == kept.size
        check("cd", kept, query.default_edits(kept.size), "edits dropped")
        # the selection is the mask's complement: nothing passes both
        assert m.convert("e", *dst, X.MASKED | X.SELECTED) == 0 and "e" not in a.models and _len_status(a, "e") == _lib.GSX_ERR_NOT_FOUND
        # src is not written, and draws what it drew
        assert state() == before
        if small:
            assert np.array_equal(_frames(a, ["src"], poses=(5,), sh_deg=0)[0], first)
            # the records of the kept set: c's frames are the frames of the yardstick with c's edits
            b.models["want_c"].gaussian_buffers.gaussians_edit_buffer.upload(src_edits[kept])
            for x, y in zip(_frames(a, ["c"], sh_deg=0), _frames(b, ["want_c"], sh_deg=0)):
                assert np.array_equal(x, y)


# ---- 5. round trips -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [(ShKind.Half, Cov3dKind.Half), N8H], ids=_id)
def test_round_trip_through_single_gives_the_stored_bits_back(stress, kind):
    """Half -> Single -> Half and Norm8 -> Single -> Norm8, SH and covariance: decoding is exact and encoding a decoded value gives its
    bits back (tests/test_convert_cpu.py checks q_snorm8(dq_snorm8(q)) == q over [-127, 127] in numpy; -128 is never stored)."""
    n = stress[0].shape[0]
    with MultiModelViewer(sh=kind[0], cov3d=kind[1]) as v:
        R.upload_pod(v, "src", stress)
        assert v.models["src"].convert("wide", *F32) == n and v.models["wide"].convert("back", *kind) == n
        held = R.pod(v, "src")
        R.same_bytes(R.pod(v, "wide"), held, "the wide model holds the decoded values")
        R.same_bytes(R.pod(v, "back"), held, "and they encode to the stored bits")
        if kind[0] == ShKind.Norm8:
            q = np.rint(held[2][:-1].astype(np.float64) * 127.0)  # (the last Gaussian holds NaN inputs: -127 after the clamp)
            assert q.min() == -127 and q.max() == 127 and np.abs(q / 127.0 - held[2][:-1]).max() <= 1e-7


# ---- 6. gsx_model_set_pod_kind --------------------------------------------------------------------------------------------------------
SET_CASES = [(F32, N8H), (F32, (ShKind.Remove, Cov3dKind.Half)), ((ShKind.Half, Cov3dKind.Half), F32)]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("src,dst", SET_CASES, ids=[f"{_id(s)}->{_id(d)}" for s, d in SET_CASES])
def test_set_pod_kind(src, dst, lanes):
    n = 2500
    g = common.small_scene(n, 66)
    rng = np.random.default_rng(66)
    tr = common.odd_transform()
    mask, sel, edits = X.words(rng.random(n) < 0.8, True), X.words(rng.random(n) < 0.4), _edit_records(n, 66)
    with MultiModelViewer(sh=src[0], cov3d=src[1]) as v:
        v.set_render_options(frames_in_flight=lanes)
        _load(v, g, "m")
        v.update_model_transform("m", tr.pos, tr.quat(), tr.scale)
        v.update_selection_highlight((1.0, 0.2, 0.1, 0.5))

        def dress(key):
            bufs = v.models[key].gaussian_buffers
            bufs.mask_buffer.upload(mask)
            bufs.selection_buffer.upload(sel)
            bufs.gaussians_edit_buffer.upload(edits)
            return bufs

        bufs = dress("m")
        warm = _frames(v, ["m"], poses=(1, 2, 3))  # speculation windows exist, and with lanes > 1 the lanes' shadow models
        assert warm[0][..., :3].max() > 0 and v.frame_stats("m")["speculated"]
        before = [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(), bufs.gaussians_edit_buffer.download().tobytes()]
        handles = [BufferHandle(v, "m", kind) for kind in ("mask", "selection", "edits")]
        snap = [h.download().tobytes() for h in handles]
        serial_len, first_planes = R.model_len(v, "m"), R.pod(v, "m")
        # the model convert makes, dressed alike (the edit records travel with convert; uploaded again they are the same bytes)
        assert v.models["m"].convert("ref", *dst) == n
        dress("ref")
        want_planes = R.pod(v, "ref")

        v.models["m"].set_pod_kind(*dst)
        assert v.models["m"].pod_kind == dst and R.pod_kind(v, "m") == dst and R.model_len(v, "m") == serial_len == n
        R.same_bytes(R.pod(v, "m"), want_planes)
        bufs = v.models["m"].gaussian_buffers
        assert [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(), bufs.gaussians_edit_buffer.download().tobytes()] == before
        assert [h.download().tobytes() for h in handles] == snap  # handles retained before the call keep their snapshots
        assert [BufferHandle(v, "m", kind).download().tobytes() for kind in ("mask", "selection", "edits")] == snap
        # the next frame is an unspeculated one, on every lane (its shadow model is new too); then the model speculates again
        got = []
        for k, pose in enumerate((5, 6, 7)):
            got += _frames(v, ["m"], poses=(pose,))
            assert bool(v.frame_stats("m")["speculated"]) == (k >= lanes), k
        want = _frames(v, ["ref"])
        assert want[0][..., :3].max() > 0
        for k, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), (k, float(np.abs(x - y).max()))
        # the same kind: nothing happens, the next frame is still a speculated one
        _frames(v, ["m"], poses=(6, 7))
        assert v.frame_stats("m")["speculated"]
        held = viewer_mod.device_bytes()
        v.models["m"].set_pod_kind(*dst)
        assert viewer_mod.device_bytes() == held
        again = _frames(v, ["m"], poses=(8,))[0]
        assert v.frame_stats("m")["speculated"]
        assert np.array_equal(again, _frames(v, ["ref"], poses=(8,))[0])
        # ... and back: the model is usable in its first kind again (Half -> Single -> Half: the stored bits return)
        v.models["m"].set_pod_kind(*src)
        assert R.pod_kind(v, "m") == src
        if src == (ShKind.Half, Cov3dKind.Half) and dst == F32:
            R.same_bytes(R.pod(v, "m"), first_planes)
        back = _frames(v, ["m"], poses=(1,))[0]
        assert not v.frame_stats("m")["speculated"]
        if src == (ShKind.Half, Cov3dKind.Half) and dst == F32:
            assert np.array_equal(back, warm[0])


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def _convert_raw(v, src, dst, flt=0, flags=0, sh=0, cov=0):
    desc, count = _lib.ConvertDesc(flt, flags, sh, cov), C.c_uint64(12345)
    _lib.check(v._L.gsx_model_convert(v._h, src.encode(), dst.encode(), C.byref(desc), C.byref(count)))
    return int(count.value)


def test_errors():
    """Every row of the error list but the allocation failure, which a test cannot ask of a shared device."""
    n = 700
    g = common.small_scene(n, 67)
    with MultiModelViewer() as v, MultiModelViewer(sh=ShKind.Norm8, cov3d=Cov3dKind.Half) as other:
        _load(v, g)
        assert v.models["src"].convert("exists", *N8H) == n  # (the first call allocates the viewer's extract workspace)
        reference = _frames(v, ["src"], poses=(9,))[0]
        held = viewer_mod.device_bytes()

        def unchanged():
            assert viewer_mod.device_bytes() == held
            assert _len_status(v, "new") == _lib.GSX_ERR_NOT_FOUND and R.model_len(v, "src") == n and R.model_len(v, "exists") == n
            assert R.pod_kind(v, "src") == F32 and R.pod_kind(v, "exists") == N8H

        cases = [("src", "new", 0, 0, 4, 0, _lib.GSX_ERR_INVALID_ARG),      # sh out of range
                 ("src", "new", 0, 0, 0, 2, _lib.GSX_ERR_INVALID_ARG),      # cov3d out of range
                 ("src", "new", 0, 0, 0xFFFFFFFF, 0, _lib.GSX_ERR_INVALID_ARG),
                 ("src", "new", 8, 0, 2, 1, _lib.GSX_ERR_INVALID_ARG),      # unknown filter bits
                 ("src", "new", 0, 4, 2, 1, _lib.GSX_ERR_INVALID_ARG),      # unknown flag bits
                 ("src", "exists", 0, 0, 2, 1, _lib.GSX_ERR_INVALID_ARG),   # dst exists
                 ("src", "src", 0, 0, 2, 1, _lib.GSX_ERR_INVALID_ARG),      # dst equals src
                 ("nope", "new", 0, 0, 2, 1, _lib.GSX_ERR_NOT_FOUND)]       # unknown src
        for src, dst, flt, flags, sh, cov, status in cases:
            with pytest.raises(GsxError) as e:
                _convert_raw(v, src, dst, flt, flags, sh, cov)
            assert e.value.status == status and "gsx_model_convert" in str(e.value), (src, dst, flt, flags, sh, cov)
            unchanged()
        L, desc, count = v._L, _lib.ConvertDesc(0, 0, 2, 1), C.c_uint64()
        assert L.gsx_model_convert(v._h, None, b"new", C.byref(desc), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_convert(v._h, b"src", None, C.byref(desc), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_convert(v._h, b"src", b"new", None, C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_convert(v._h, b"src", b"new", C.byref(desc), None) == _lib.GSX_ERR_INVALID_ARG
        unchanged()
        # gsx_model_set_pod_kind
        for key, sh, cov, status in (("src", 4, 0, _lib.GSX_ERR_INVALID_ARG), ("src", 0, 2, _lib.GSX_ERR_INVALID_ARG), ("src", -1, 0, _lib.GSX_ERR_INVALID_ARG),
                                     ("nope", 2, 1, _lib.GSX_ERR_NOT_FOUND)):
            assert L.gsx_model_set_pod_kind(v._h, key.encode(), sh, cov) == status, (key, sh, cov)
            assert b"gsx_model_set_pod_kind" in L.gsx_last_error_string()
            unchanged()
        assert L.gsx_model_set_pod_kind(v._h, None, 0, 0) == _lib.GSX_ERR_INVALID_ARG
        # gsx_model_pod_kind
        sh, cov = C.c_int32(), C.c_int32()
        assert L.gsx_model_pod_kind(v._h, b"nope", C.byref(sh), C.byref(cov)) == _lib.GSX_ERR_NOT_FOUND
        assert L.gsx_model_pod_kind(v._h, None, C.byref(sh), C.byref(cov)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_pod_kind(v._h, b"src", None, C.byref(cov)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_pod_kind(v._h, b"src", C.byref(sh), None) == _lib.GSX_ERR_INVALID_ARG
        unchanged()
        assert np.array_equal(_frames(v, ["src"], poses=(9,))[0], reference)  # the viewer still renders src
        held = viewer_mod.device_bytes()  # (the frame may have grown a buffer)
        # a sharded model
        v.shard_set_limits("src", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        held = viewer_mod.device_bytes()
        with pytest.raises(GsxError) as e:
            _convert_raw(v, "src", "new", sh=2, cov=1)
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED
        assert L.gsx_model_set_pod_kind(v._h, b"src", 2, 1) == _lib.GSX_ERR_UNSUPPORTED
        unchanged()
        # a viewer with a communicator
        _load(other, g[:50], "a")
        group = CommGroup(1)
        other.comm_init_group(group, 0)
        held_other = viewer_mod.device_bytes()
        with pytest.raises(GsxError) as e:
            other.models["a"].convert("new", *F32)
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED and "new" not in other.models
        with pytest.raises(GsxError) as e:
            other.models["a"].set_pod_kind(*F32)
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED and R.pod_kind(other, "a") == N8H
        assert viewer_mod.device_bytes() == held_other and _len_status(other, "new") == _lib.GSX_ERR_NOT_FOUND


# ---- 8. convert, then merge -----------------------------------------------------------------------------------------------------------
def test_convert_then_merge():
    na, nb = 900, 1300
    with MultiModelViewer() as v:
        _load(v, common.small_scene(na, 68), "a")
        R.create_model(v, "b", nb, *N8H)
        v.models["b"].gaussian_buffers.gaussians_buffer.update_range(0, common.small_scene(nb, 69))
        assert R.pod_kind(v, "a") == F32 and R.pod_kind(v, "b") == N8H
        with pytest.raises(GsxError) as e:
            v.merge("m", ["a", "b"])  # mixed kinds: refused, as before
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG and _len_status(v, "m") == _lib.GSX_ERR_NOT_FOUND
        assert v.models["b"].convert("b32", *F32) == nb
        assert v.merge("m", ["a", "b32"]) == (na + nb, [na, nb])
        assert R.pod_kind(v, "m") == F32
        pa, pb = R.pod(v, "a"), R.pod(v, "b")  # (b's decoded values are what b32 stores as float32)
        R.same_bytes(R.pod(v, "m"), [np.concatenate([x, y]) for x, y in zip(pa, pb)])
        # ... and the other way: a into b's kind
        assert v.models["a"].convert("a8", *N8H) == na
        assert v.merge("m8", ["a8", "b"]) == (na + nb, [na, nb]) and R.pod_kind(v, "m8") == N8H
        R.same_bytes(R.pod(v, "m8"), [np.concatenate([x, y]) for x, y in zip(R.pod(v, "a8"), pb)])
        assert _frames(v, ["m8"], poses=(5,))[0][..., :3].max() > 0
