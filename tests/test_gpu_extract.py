"""GPU: gsx_model_extract (spec/RENDER_SPEC.md §12; csrc/kernels_extract.hip) against numpy indexing of what was downloaded from the
source model before the call.  Equality is exact everywhere: the new model's planes, edit records and frames are compared bit for bit.
The kept set is restated in tests/extract_ref.py."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import extract_ref as X
from tests.model_ops import KINDS, frames as _frames, load as _load, model_len as _len, pod as _pod
from wgpu_3dgs_viewer_app_amd import _lib, query, scene
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as F
from wgpu_3dgs_viewer_app_amd.viewer import BufferHandle, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
SRC, DST = "src", "dst"
# word, wave and workgroup tails; one below, at and one above the Gaussians of a scatter workgroup; a few dozen workgroups; and one
# model just past what the scan's one workgroup takes in a pass (X.SCAN_PASS partials of X.GROUP Gaussians each)
EDGE_SIZES = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, X.GROUP - 1, X.GROUP, X.GROUP + 1, 70001, X.SCAN_PASS * X.GROUP + X.GROUP + 1]


@pytest.fixture(scope="module")
def big():
    """One SH-0 scene; the smaller models are its prefixes.  Never written to."""
    g = scene.synthetic_gaussians(EDGE_SIZES[-1], 91, 0)
    g.setflags(write=False)
    return g


def _same_rows(got, src, kept, what=""):
    """the four downloaded planes of dst are src's kept rows, bit for bit (bytes: a NaN equals itself)"""
    for name, a, b in zip(("pos", "color", "sh", "cov3d"), got, src):
        assert a.shape[0] == kept.size and a.tobytes() == np.ascontiguousarray(b[kept]).tobytes(), (what, name)


def _extract_raw(v, src, dst, flt=0, flags=0):
    desc, count = _lib.ExtractDesc(flt, flags), C.c_uint64(12345)
    _lib.check(v._L.gsx_model_extract(v._h, src.encode(), dst.encode(), C.byref(desc), C.byref(count)))
    return int(count.value)


def _mask_patterns(n):
    idx = np.arange(n)
    rng = np.random.default_rng(n)
    yield "all set", np.ones(n, bool), False
    yield "only bit 0", idx == 0, False
    yield "only bit n - 1", idx == n - 1, False
    yield "alternating", idx % 2 == 1, False
    yield "a clear word beside a set word", (idx // 32) % 2 == 1, False
    for p in (0.5, 0.01, 0.99):
        yield f"random p = {p}", rng.random(n) < p, False
    yield "garbage above n", rng.random(n) < 0.5, True


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_edges_of_the_compaction(big, n):
    g = big[:n]
    with MultiModelViewer(sh=ShKind.Remove) as v:
        _load(v, g)
        m = v.models[SRC]
        src = _pod(v, SRC)
        for name, keep, garbage in _mask_patterns(n):
            m.gaussian_buffers.mask_buffer.upload(X.words(keep, garbage))
            kept = X.kept(n, X.MASKED, 0, mask=keep)
            count = m.extract(DST, X.MASKED)
            assert count == kept.size, (name, count, kept.size)
            if count == 0:  # (p = 0.01 of a tiny model)
                assert _len(v, DST)[0] == _lib.GSX_ERR_NOT_FOUND and DST not in v.models
                continue
            assert _len(v, DST) == (_lib.GSX_OK, count)
            _same_rows(_pod(v, DST), src, kept, name)
            v.remove_model(DST)
        # an all-clear mask (garbage above n or not): nothing is kept, GSX_OK, and no model is created
        for garbage in (False, True):
            m.gaussian_buffers.mask_buffer.upload(X.words(np.zeros(n, bool), garbage))
            assert m.extract(DST, X.MASKED) == 0 and DST not in v.models
            assert _len(v, DST)[0] == _lib.GSX_ERR_NOT_FOUND


@pytest.mark.parametrize("sh,cov", KINDS, ids=[f"{sh.name}-{cov.name}" for sh, cov in KINDS])
def test_all_eight_pod_kinds(sh, cov):
    n = 600
    g = common.small_scene(n, 17)
    keep = np.random.default_rng(3).random(n) < 0.5
    kept = np.nonzero(keep)[0]
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        src = _pod(v, SRC)
        v.models[SRC].gaussian_buffers.mask_buffer.upload(X.words(keep))
        before = viewer_mod.device_bytes()
        assert v.models[SRC].extract(DST, X.MASKED) == kept.size
        extracted_bytes = viewer_mod.device_bytes() - before
        _same_rows(_pod(v, DST), src, kept, f"{sh.name}/{cov.name}")  # (the dequantised planes: equal only if the stored bits are)
        # dst has src's kinds: it holds what a new model of that many Gaussians and these kinds holds (the extract workspace is the
        # viewer's and was allocated by the call: ceil(n / 32) keep words and two words per workgroup, padded)
        before = viewer_mod.device_bytes()
        v.add_model("fresh", kept.size)
        assert 0 <= extracted_bytes - (viewer_mod.device_bytes() - before) <= 4096
        # a frame of dst renders: finite, not empty, and the same frames as a model uploaded from the kept host rows (this reads
        # the shade records too: the later frames of a camera path are speculated)
        v.models["fresh"].gaussian_buffers.gaussians_buffer.update_range(0, g[kept])
        got, want = _frames(v, [DST]), _frames(v, ["fresh"])
        assert np.isfinite(got[0]).all() and got[0][..., :3].max() > 0
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def _filter_model(v, n, seed=7):
    """a model with a mask, a selection and stored edits (some ENABLED + HIDDEN) and three non-finite positions; returns the host arrays"""
    g = common.small_scene(n, seed, 0)
    g["pos"][5, 0], g["pos"][n // 2, 1], g["pos"][n - 1, 2] = np.nan, np.inf, -np.inf
    rng = np.random.default_rng(seed)
    mask, sel = rng.random(n) < 0.6, rng.random(n) < 0.4
    mask[[5, n - 1]], sel[[5, n // 2]] = True, True
    edits = query.default_edits(n)
    edits["flag"][0::3] = int(F.ENABLED | F.HIDDEN)
    edits["flag"][1::3] = int(F.ENABLED)
    edits["flag"][5::7] |= int(F.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    edits["color"][:, 0] = rng.random(n).astype(np.float32)
    edits["contrast"] = rng.random(n).astype(np.float32)
    _load(v, g)
    bufs = v.models[SRC].gaussian_buffers
    bufs.mask_buffer.upload(X.words(mask, True))
    bufs.selection_buffer.upload(X.words(sel, True))
    bufs.gaussians_edit_buffer.upload(edits)
    return g, mask, sel, edits


def test_filters_and_flags():
    n = 4097
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, edits = _filter_model(v, n)
        m = v.models[SRC]
        src = _pod(v, SRC)
        stored = m.gaussian_buffers.gaussians_edit_buffer.download()["flag"]
        for flt in (X.MASKED, X.SKIP_HIDDEN, X.SELECTED, X.MASKED | X.SKIP_HIDDEN | X.SELECTED, 0):
            b = m.bounds(masked=bool(flt & X.MASKED), skip_hidden=bool(flt & X.SKIP_HIDDEN), selected=bool(flt & X.SELECTED))
            for invert in (False, True):
                kept = X.kept(n, flt, X.INVERT if invert else 0, mask, sel, stored)
                count = m.extract(DST, flt, invert=invert)
                assert count == kept.size, (flt, invert)
                if not invert:
                    assert count == b.count + b.n_nonfinite and count > 0, flt
                elif flt == 0:
                    assert count == 0 and DST not in v.models  # the complement of everything
                    continue
                else:
                    assert count == n - (b.count + b.n_nonfinite) and count > 0, flt
                _same_rows(_pod(v, DST), src, kept, (flt, invert))
                v.remove_model(DST)
        # SKIP_HIDDEN reads the stored flag, whatever gsx_model_show_unedited says
        v.show_unedited(SRC, True)
        assert m.extract(DST, X.SKIP_HIDDEN) == X.kept(n, X.SKIP_HIDDEN, 0, edit_flags=stored).size
        v.show_unedited(SRC, False)
    # absent planes: no mask = all, no edit records = none hidden, no selection = none (and all of them when inverted)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        _load(v, g)
        m = v.models[SRC]
        assert m.extract("a", X.MASKED | X.SKIP_HIDDEN) == n
        assert m.extract("b", X.SELECTED) == 0 and "b" not in v.models
        assert m.extract("c", X.SELECTED, invert=True) == n
        _same_rows(_pod(v, "c"), _pod(v, SRC), np.arange(n), "inverted empty selection")


def test_edits_mask_selection_and_transform_of_the_new_model():
    n = 1500
    tr = common.odd_transform()
    with MultiModelViewer() as v:
        g = common.small_scene(n, 23)
        keep = np.random.default_rng(4).random(n) < 0.45
        kept = np.nonzero(keep)[0]
        _load(v, g)
        m = v.models[SRC]
        v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)
        edits = query.default_edits(n)
        edits["flag"][0::3] = int(F.ENABLED | F.OVERRIDE_COLOR)
        edits["flag"][1::5] = int(F.ENABLED | F.HIDDEN)
        edits["color"][:, 1] = np.random.default_rng(5).random(n).astype(np.float32)
        edits["alpha"][0::3] = np.float32(0.5)
        m.gaussian_buffers.gaussians_edit_buffer.upload(edits)
        m.gaussian_buffers.mask_buffer.upload(X.words(keep))
        src_edits = m.gaussian_buffers.gaussians_edit_buffer.download()
        src_raw = BufferHandle(v, SRC, "edits").download()
        assert (src_edits["flag"] != 0).any() and (src_edits["flag"] == 0).any()
        # carried: the kept Gaussians' records; the never-edited ones read as the default pod
        assert m.extract("carried", X.MASKED) == kept.size
        got = v.models["carried"].gaussian_buffers.gaussians_edit_buffer.download()
        assert got.tobytes() == src_edits[kept].tobytes()
        assert BufferHandle(v, "carried", "edits").download().tobytes() == src_raw[kept].tobytes()
        never = src_edits["flag"][kept] == 0
        assert never.any() and got[never].tobytes() == query.default_edits(int(never.sum())).tobytes()
        # DROP_EDITS: every record is the default
        assert m.extract("dropped", X.MASKED, drop_edits=True) == kept.size
        assert v.models["dropped"].gaussian_buffers.gaussians_edit_buffer.download().tobytes() == query.default_edits(kept.size).tobytes()
        for key in ("carried", "dropped"):
            bufs = v.models[key].gaussian_buffers
            assert np.all(bufs.mask_buffer.download() == 0xFFFFFFFF) and not bufs.selection_buffer.download().any()
            assert np.all(BufferHandle(v, key, "mask").download() == 0xFFFFFFFF) and not BufferHandle(v, key, "selection").download().any()
        # the transform: dst draws where src draws (the hidden edits hide the same Gaussians in both)
        src_frames = _frames(v, [SRC])
        for a, b in zip(_frames(v, ["carried"]), src_frames):
            assert np.array_equal(a, b)
        # ... and without its edit records the hidden Gaussians show: another frame, under the same transform as a twin given it by hand
        _load(v, g[kept], "twin")
        v.update_model_transform("twin", tr.pos, tr.quat(), tr.scale)
        dropped = _frames(v, ["dropped"])
        assert not np.array_equal(dropped[0], src_frames[0])
        for a, b in zip(dropped, _frames(v, ["twin"])):
            assert np.array_equal(a, b)
    # a source without edit records gives a new model without edit records: it holds what a fresh model of n Gaussians holds
    with MultiModelViewer(sh=ShKind.Remove) as v:
        _load(v, g)
        m = v.models[SRC]
        assert m.extract("warm") == n  # (the viewer's extract workspace is allocated by the first call)
        v.remove_model("warm")

        def held_by(make):
            before = viewer_mod.device_bytes()
            make()
            return viewer_mod.device_bytes() - before

        without = held_by(lambda: m.extract(DST))
        assert without == held_by(lambda: v.add_model("fresh", n))
        assert v.models[DST].gaussian_buffers.gaussians_edit_buffer.download().tobytes() == query.default_edits(n).tobytes()
        m.gaussian_buffers.gaussians_edit_buffer.upload(query.default_edits(n))  # records, none of them enabled
        assert held_by(lambda: m.extract("with")) >= without + 32 * n  # two 16-byte planes a Gaussian
        assert held_by(lambda: m.extract("drop", drop_edits=True)) == without
        assert v.models["with"].gaussian_buffers.gaussians_edit_buffer.download().tobytes() == query.default_edits(n).tobytes()


@pytest.mark.parametrize("sh,cov", [(ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)], ids=["f32", "Norm8-Half"])
def test_the_frame_of_the_new_model_is_the_masked_frame(sh, cov):
    """Stable order: masked Gaussians are culled before the sort, the depth order is total with the index as tie-break, compaction
    is monotone in the index, and every frame is bit-identical to the single-pass frame: so dst alone draws what src draws under its mask."""
    n = 600
    g = common.small_scene(n, 29)
    tr = common.odd_transform()
    keep = np.random.default_rng(6).random(n) < 0.5
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)
        v.models[SRC].gaussian_buffers.mask_buffer.upload(X.words(keep))
        masked = _frames(v, [SRC])
        assert v.models[SRC].extract(DST, X.MASKED) == int(keep.sum())
        alone = _frames(v, [DST])
        assert masked[0][..., :3].max() > 0
        for k in (0, 2):  # the first frame and the third
            differing = np.argwhere(masked[k] != alone[k])
            assert differing.size == 0, (k, differing[:4])


def test_the_source_is_untouched():
    n = 3000
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            g, mask, sel, edits = _filter_model(vv, n)
        m = v.models[SRC]

        def state(vv):
            bufs = vv.models[SRC].gaussian_buffers
            return [a.tobytes() for a in _pod(vv, SRC)] + [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(),
                                                         bufs.gaussians_edit_buffer.download().tobytes(),
                                                         BufferHandle(vv, SRC, "mask").download().tobytes(),
                                                         BufferHandle(vv, SRC, "selection").download().tobytes()]

        before = state(v)
        first = _frames(v, [SRC], poses=(5,))[0]
        assert np.array_equal(first, _frames(twin, [SRC], poses=(5,))[0])
        for flt, invert, drop in ((0, False, False), (X.MASKED | X.SKIP_HIDDEN | X.SELECTED, False, False), (X.SELECTED, True, True)):
            assert m.extract(f"d{flt}{int(invert)}", flt, invert=invert, drop_edits=drop) > 0
        assert state(v) == before == state(twin)
        # src's next frames are the frames of the twin that was never extracted from
        for a, b in zip(_frames(v, [SRC], poses=(6, 7)), _frames(twin, [SRC], poses=(6, 7))):
            assert np.array_equal(a, b)


def _lane_sequence(g, sel, lanes):
    out = []
    with MultiModelViewer() as v:
        v.set_render_options(frames_in_flight=lanes)
        _load(v, g)
        v.models[SRC].gaussian_buffers.selection_buffer.upload(X.words(sel))
        for pose in (1, 2, 3, 4):
            out += _frames(v, [SRC], poses=(pose,))
        assert v.models[SRC].extract(DST, X.SELECTED) == int(sel.sum())  # behind the frames in flight on the lanes
        for pose in (5, 6, 7, 8):
            out += _frames(v, [SRC, DST], poses=(pose,))
    return out


def test_lanes():
    g = common.small_scene(2500, 37)
    sel = np.random.default_rng(8).random(2500) < 0.3
    two, one = _lane_sequence(g, sel, 2), _lane_sequence(g, sel, 1)
    assert len(two) == 8 and two[0][..., :3].max() > 0
    for k, (a, b) in enumerate(zip(two, one)):
        assert np.array_equal(a, b), k


def test_determinism_and_errors():
    n = 2 * X.GROUP + 77
    with MultiModelViewer() as v:
        g, mask, sel, edits = _filter_model(v, n)
        m = v.models[SRC]
        # two extractions under different keys are bit-identical
        flt = X.MASKED | X.SKIP_HIDDEN
        assert m.extract("one", flt) == m.extract("two", flt) > 0
        a, b = _pod(v, "one"), _pod(v, "two")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert (v.models["one"].gaussian_buffers.gaussians_edit_buffer.download().tobytes()
                == v.models["two"].gaussian_buffers.gaussians_edit_buffer.download().tobytes())
        frames_one = _frames(v, ["one"])
        for x, y in zip(frames_one, _frames(v, ["two"])):
            assert np.array_equal(x, y)
        reference = _frames(v, [SRC], poses=(9,))[0]
        cases = ((SRC, "one", 0, 0, _lib.GSX_ERR_INVALID_ARG),      # dst exists
                 (SRC, SRC, 0, 0, _lib.GSX_ERR_INVALID_ARG),        # dst equals src
                 ("nope", "new", 0, 0, _lib.GSX_ERR_NOT_FOUND),     # unknown src
                 (SRC, "new", 8, 0, _lib.GSX_ERR_INVALID_ARG),      # unknown filter bits
                 (SRC, "new", 0, 4, _lib.GSX_ERR_INVALID_ARG))      # unknown flag bits
        for src, dst, flt, flags, status in cases:
            with pytest.raises(GsxError) as e:
                _extract_raw(v, src, dst, flt, flags)
            assert e.value.status == status and "gsx_model_extract" in str(e.value)
            assert _len(v, "new")[0] == _lib.GSX_ERR_NOT_FOUND
            assert np.array_equal(_frames(v, [SRC], poses=(9,))[0], reference)  # the viewer still renders src
        # null arguments
        desc, count = _lib.ExtractDesc(0, 0), C.c_uint64()
        L = v._L
        assert L.gsx_model_extract(v._h, None, b"new", C.byref(desc), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_extract(v._h, SRC.encode(), None, C.byref(desc), C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_extract(v._h, SRC.encode(), b"new", None, C.byref(count)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_extract(v._h, SRC.encode(), b"new", C.byref(desc), None) == _lib.GSX_ERR_INVALID_ARG
        assert np.array_equal(_frames(v, [SRC], poses=(9,))[0], reference)
