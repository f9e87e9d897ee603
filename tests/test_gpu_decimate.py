"""GPU: gsx_model_decimate and gsx_model_decimate_edge (spec/RENDER_SPEC.md §22; csrc/kernels_decimate.hip) against
tests/decimate_driver.cpp, the float32 restatement that shares csrc/decimate_math.h with the kernels, bit for bit: the statistics, the
map, and the rows of dst.  Device bytes are read as tests/test_gpu_convert.py reads them: the resident planes through
gsx_model_download_pod (the exact dequantisation of the stored values: equal only if the stored bits are), compared with a model
uploaded from the driver's float32 rows (the upload quantises once, and writes planes and shade records from one value); the shade
records through the later, speculated frames of a camera path, which shade from them.  How far float32 lies from float64 is
tests/test_decimate_cpu.py's business."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import common
from tests import convert_ref as K
from tests import decimate_ref as D
from tests import extract_ref as X
from tests.model_ops import H, KIND_IDS, KINDS, W, frames as _frames, load as _load, model_len as _len
from wgpu_3dgs_viewer_app_amd import _lib, query
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as EF
from wgpu_3dgs_viewer_app_amd.viewer import BufferHandle, CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
F = np.float32
SRC, DST = "src", "dst"
LDS_BUCKET = int(re.search(r"kDecLdsBucket = (\d+)u", open(os.path.join(D.CSRC, "decimate_math.h")).read()).group(1))
TWO_KINDS = [(ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)]
TWO_IDS = ["f32", "Norm8-Half"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return D.build_driver(tmp_path_factory.mktemp("decimate"))


def _box(g):
    p = g["pos"]
    return p.min(axis=0), p.max(axis=0)


def _grouped(g, sizes, seed, lattice=16):
    """g with its first 1 + sum(sizes) positions rewritten: an anchor at the box's low corner, then groups of the given sizes, each
    inside its own cell of a lattice of `lattice` cells across the box (the cell edge is returned), at shuffled indices"""
    rng = np.random.default_rng(seed)
    lo, hi = _box(g)
    edge = F((hi - lo).max() / lattice)
    n = 1 + int(np.sum(sizes))
    g = g[:n].copy()
    cells = rng.permutation(lattice ** 3)[:len(sizes)]
    k = np.stack([cells % lattice, cells // lattice % lattice, cells // lattice ** 2], axis=1)
    k[:, 0] = np.maximum(k[:, 0], 1)  # (not the anchor's cell; two groups may then share a cell: the driver says what comes of it)
    pos = [lo.astype(np.float64)[None]]
    for c, size in zip(k, sizes):
        pos.append(lo + (c + 0.5 + rng.uniform(-0.3, 0.3, (size, 3))) * float(edge))
    pos = np.concatenate(pos).astype(F)
    g["pos"] = pos[rng.permutation(n)]  # (the anchor too lands at any index)
    return g, edge


def _check(v, driver, cell, flt=0, invert=False, kept=None, grid_bits=0, frames=True, key=DST):
    """decimate SRC into `key` and compare everything with the driver's answer for SRC's resident planes; returns (stats, driver's)"""
    src = K.pod(v, SRC)
    n = src[0].shape[0]
    kept = np.ones(n, bool) if kept is None else kept
    want = D.play(driver, src, kept, cell)
    got = v.models[SRC].decimate(key, cell, flt, invert, grid_bits, want_map=True)
    assert (got.count, got.n_nonfinite, got.cells, got.singletons, got.largest_cell) == (
        want["count"], want["n_nonfinite"], want["cells"], want["singletons"], want["largest_cell"]), (got, {k: want[k] for k in ("count", "cells")})
    assert np.array_equal(got.map, want["map"])
    if want["cells"] == 0:
        assert key not in v.models and _len(v, key)[0] == _lib.GSX_ERR_NOT_FOUND
        return got, want
    assert _len(v, key) == (_lib.GSX_OK, want["cells"])
    kind = K.pod_kind(v, SRC)
    assert K.pod_kind(v, key) == kind
    K.upload_pod(v, "want", want["planes"], kind)
    K.same_bytes(K.pod(v, key), K.pod(v, "want"), "dst against the driver's rows, uploaded")
    if frames:  # the speculated frames shade from the records: they agree with the planes word for word, as the upload's do
        a, b = _frames(v, [key]), _frames(v, ["want"])
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    v.remove_model("want")
    return got, want


# ---- 1. the smallest cases -----------------------------------------------------------------------------------------------------------
def test_one_gaussian_nothing_kept_and_a_nan(driver):
    g = common.small_scene(300, 71)
    with MultiModelViewer() as v:
        _load(v, g[:1])
        got, _ = _check(v, driver, 0.5)
        assert (got.count, got.cells, got.singletons, got.largest_cell) == (1, 1, 1, 1) and got.map[0] == 0
        K.same_bytes(K.pod(v, DST), K.pod(v, SRC))
    with MultiModelViewer() as v:
        bad = g.copy()
        bad["pos"][7, 1], bad["pos"][299, 0] = np.nan, np.inf
        _load(v, bad)
        # SELECTED of a model without a selection: nothing is kept, no model, GSX_OK
        got = v.models[SRC].decimate(DST, 0.5, X.SELECTED, want_map=True)
        assert (got.count, got.n_nonfinite, got.cells) == (0, 0, 0) and (got.map == D.NO_CELL).all() and DST not in v.models
        assert _len(v, DST)[0] == _lib.GSX_ERR_NOT_FOUND
        # the kept Gaussians with a non-finite coordinate are dropped and counted
        got, want = _check(v, driver, 0.5)
        assert got.n_nonfinite == 2 and got.count == 298 and got.map[7] == got.map[299] == D.NO_CELL and got.cells < 298


# ---- 2. every cell a singleton IS extract with DROP_EDITS ------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_singletons_are_extract(driver, sh, cov):
    n = 600
    g = common.small_scene(n, 72)
    keep = np.random.default_rng(72).random(n) < 0.7
    lo, hi = _box(g)
    cell = F((hi - lo).max() / 30000.0)  # (below extent / 32767 the clamp would join cells)
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        v.models[SRC].gaussian_buffers.mask_buffer.upload(X.words(keep, True))
        edits = query.default_edits(n)
        edits["flag"][0::3] = int(EF.ENABLED | EF.OVERRIDE_COLOR)
        v.models[SRC].gaussian_buffers.gaussians_edit_buffer.upload(edits)
        got, want = _check(v, driver, cell, X.MASKED, kept=keep, frames=False)
        assert got.cells == got.singletons == got.count == int(keep.sum()) and got.largest_cell == 1
        assert v.models[SRC].extract("ex", X.MASKED, drop_edits=True) == got.cells
        K.same_bytes(K.pod(v, DST), K.pod(v, "ex"))
        assert np.array_equal(got.map[keep], np.arange(got.cells))
        for a, b in zip(_frames(v, [DST]), _frames(v, ["ex"])):
            assert np.array_equal(a, b)


# ---- 3. the edges of the ordering and of the reduction ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", TWO_KINDS, ids=TWO_IDS)
def test_wave_edges_at_shuffled_indices(driver, sh, cov):
    sizes = [2, 63, 64, 65, 129, 1, 1, 3, 5, 17, 31, 33, 127, 128, 130]
    g, edge = _grouped(common.small_scene(1 + sum(sizes), 73), sizes, 73)
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        got, want = _check(v, driver, edge)
        assert set(sizes) <= set(want["members"].tolist())
        rep = np.array([np.nonzero(want["map"] == j)[0].min() for j in range(want["cells"])])
        assert np.array_equal(np.sort(rep), rep)  # ascending representative ...
        assert not np.array_equal(np.argsort(g["pos"][rep, 0], kind="stable"), np.arange(rep.size))  # ... which is not spatial order


@pytest.mark.parametrize("n,bits,lattice", [(6000, 1, 12), (40000, 8, 14), (5000, 8, 12)], ids=["global-2-buckets", "lds-256-buckets", "rank-256-buckets"])
def test_small_tables_many_cells_a_bucket(driver, n, bits, lattice):
    """a forced table of 2 or 256 buckets under a few thousand cells: every bucket holds many cells, and is ordered by the
    global-memory network (3000 records), in LDS (about 156) or by counting (about 20)"""
    g = common.small_scene(n, 74, 0)
    lo, hi = _box(g)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        _load(v, g)
        got, want = _check(v, driver, F((hi - lo).max() / lattice), grid_bits=bits, frames=False)
        assert got.grid_bits == bits and 500 < got.cells < n and got.largest_cell > 1
        assert (n >> bits > LDS_BUCKET) == (bits == 1)


@pytest.mark.parametrize("n", [LDS_BUCKET + 1, 2 * LDS_BUCKET + 3], ids=["lds+1", "2lds+3"])
def test_the_whole_model_in_one_cell(driver, n):
    g = common.small_scene(n, 75)
    lo, hi = _box(g)
    with MultiModelViewer() as v:
        _load(v, g)
        got, want = _check(v, driver, F((hi - lo).max() * 2))
        assert (got.cells, got.singletons, got.largest_cell, got.count) == (1, 0, n, n) and (got.map == 0).all()


def test_cells_beyond_the_clamp_are_joined(driver):
    n = 500
    g = common.small_scene(n, 76)
    lo, hi = _box(g)
    cell = F((hi - lo).max() / 200000.0)  # extent / edge far above 32767
    with MultiModelViewer() as v:
        _load(v, g)
        got, want = _check(v, driver, cell)
        u = (g["pos"] - lo) / cell
        assert (u.max(axis=0) > 3 * 32767).all() and got.cells < got.count and got.largest_cell > 1


# ---- 4. the filters ------------------------------------------------------------------------------------------------------------------
def test_every_filter(driver):
    n = 3000
    g = common.small_scene(n, 77)
    rng = np.random.default_rng(77)
    mask, sel = rng.random(n) < 0.6, rng.random(n) < 0.5
    edits = query.default_edits(n)
    edits["flag"][0::3] = int(EF.ENABLED | EF.HIDDEN)
    edits["flag"][1::3] = int(EF.ENABLED)
    edits["flag"][5::7] |= int(EF.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    lo, hi = _box(g)
    cell = F((hi - lo).max() / 10)
    with MultiModelViewer() as v:
        _load(v, g)
        bufs = v.models[SRC].gaussian_buffers
        bufs.mask_buffer.upload(X.words(mask, True))
        bufs.gaussians_edit_buffer.upload(edits)
        # SELECTED without a selection: none; inverted: all
        assert v.models[SRC].decimate_count(cell, X.SELECTED).count == 0
        assert v.models[SRC].decimate_count(cell, X.SELECTED, invert=True).count == n
        bufs.selection_buffer.upload(X.words(sel, True))
        for k, (flt, invert) in enumerate(((X.MASKED, False), (X.SELECTED, False), (X.SELECTED, True), (X.SKIP_HIDDEN, False),
                                           (X.MASKED | X.SKIP_HIDDEN | X.SELECTED, False), (X.MASKED | X.SKIP_HIDDEN | X.SELECTED, True))):
            kept = np.zeros(n, bool)
            kept[X.kept(n, flt, X.INVERT if invert else 0, mask, sel, edits["flag"])] = True
            got, want = _check(v, driver, cell, flt, invert, kept, frames=k == 4)
            assert got.count == int(kept.sum()) and 0 < got.cells < got.count
            # dst: no mask, no selection, no edits, src's transform
            d = v.models[DST].gaussian_buffers
            assert np.all(d.mask_buffer.download() == 0xFFFFFFFF) and not d.selection_buffer.download().any()
            assert d.gaussians_edit_buffer.download().tobytes() == query.default_edits(got.cells).tobytes()
            v.remove_model(DST)


# ---- 5. merged and one-member cells in every pod kind -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_mixed_cells_in_all_eight_pod_kinds(driver, sh, cov):
    n = 400
    g = common.small_scene(n, 78)
    lo, hi = _box(g)
    tr = common.odd_transform()
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)
        got, want = _check(v, driver, F((hi - lo).max() / 6), frames=False)
        assert 0 < got.singletons < got.cells < n and got.largest_cell > 2
        # dst has src's transform: under it dst draws what the driver's rows draw under it
        K.upload_pod(v, "want", want["planes"], (sh, cov))
        v.update_model_transform("want", tr.pos, tr.quat(), tr.scale)
        for a, b in zip(_frames(v, [DST]), _frames(v, ["want"])):
            assert np.array_equal(a, b)


def _stats(r):
    return (r.count, r.n_nonfinite, r.cells, r.singletons, r.largest_cell)


# ---- 6. the same bits, nothing of src written, count only ---------------------------------------------------------------------------------
def test_determinism_source_untouched_and_count_only(driver):
    n = 5000
    g = common.small_scene(n, 79)
    lo, hi = _box(g)
    cell = F((hi - lo).max() / 3)  # at most 27 cells for 3000 participants: cells of more members than a wave has lanes
    rng = np.random.default_rng(79)
    mask, sel = X.words(rng.random(n) < 0.8, True), X.words(rng.random(n) < 0.5, True)
    edits = query.default_edits(n)
    edits["flag"][0::4] = int(EF.ENABLED | EF.HIDDEN)
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _load(vv, g)
            bufs = vv.models[SRC].gaussian_buffers
            bufs.mask_buffer.upload(mask)
            bufs.selection_buffer.upload(sel)
            bufs.gaussians_edit_buffer.upload(edits)

        def state(vv):
            bufs = vv.models[SRC].gaussian_buffers
            return [a.tobytes() for a in K.pod(vv, SRC)] + [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(),
                                                          bufs.gaussians_edit_buffer.download().tobytes(), BufferHandle(vv, SRC, "edits").download().tobytes()]

        before = state(v)
        assert np.array_equal(_frames(v, [SRC], poses=(5,))[0], _frames(twin, [SRC], poses=(5,))[0])
        m = v.models[SRC]
        flt = X.MASKED | X.SKIP_HIDDEN
        one, two = m.decimate("one", cell, flt, want_map=True), m.decimate("two", cell, flt, grid_bits=9, want_map=True)
        assert one.cells == two.cells > 4 and one.largest_cell > 64 and np.array_equal(one.map, two.map)
        K.same_bytes(K.pod(v, "one"), K.pod(v, "two"))
        for a, b in zip(_frames(v, ["one"]), _frames(v, ["two"])):
            assert np.array_equal(a, b)
        # count only: the full call's statistics and map, and no model
        count = m.decimate_count(cell, flt, want_map=True)
        assert _stats(count) == _stats(one) and np.array_equal(count.map, one.map)
        assert sorted(v.models) == sorted([SRC, "one", "two"])
        # src as it was, byte for byte, and its next frames those of the twin that was never decimated
        assert state(v) == before == state(twin)
        for a, b in zip(_frames(v, [SRC], poses=(6, 7)), _frames(twin, [SRC], poses=(6, 7))):
            assert np.array_equal(a, b)


def test_dst_renders_on_lanes(driver):
    n = 2500
    g = common.small_scene(n, 80)
    lo, hi = _box(g)
    cell = F((hi - lo).max() / 8)
    out = []
    for lanes in (2, 1):
        with MultiModelViewer() as v:
            v.set_render_options(frames_in_flight=lanes)
            _load(v, g)
            seq = []
            for pose in (1, 2, 3):
                seq += _frames(v, [SRC], poses=(pose,))
            got, want = _check(v, driver, cell, frames=False)  # behind the frames in flight on the lanes
            K.upload_pod(v, "want", want["planes"], K.pod_kind(v, SRC))
            for pose in (4, 5, 6, 7):
                a, b = _frames(v, [DST], poses=(pose,))[0], _frames(v, ["want"], poses=(pose,))[0]
                assert np.array_equal(a, b), (lanes, pose)
                seq += [a] + _frames(v, [SRC, DST], poses=(pose,))
            out.append(seq)
    assert len(out[0]) == 11 and out[0][3][..., :3].max() > 0
    for k, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a, b), k


# ---- 7. the edge for a target count ---------------------------------------------------------------------------------------------------
def test_decimate_edge_is_the_drivers(driver):
    n = 4000
    g = common.small_scene(n, 81, 0)
    g["pos"][11, 2] = np.nan
    sel = np.random.default_rng(81).random(n) < 0.7
    with MultiModelViewer(sh=ShKind.Remove) as v:
        _load(v, g)
        v.models[SRC].gaussian_buffers.selection_buffer.upload(X.words(sel, True))
        src = K.pod(v, SRC)
        for target, flt, invert, kept in ((300, 0, False, np.ones(n, bool)), (1, 0, False, np.ones(n, bool)), (1500, X.SELECTED, False, sel),
                                          (50, X.SELECTED, True, ~sel)):
            cell, cells = v.models[SRC].decimate_edge(target, flt, invert)
            want_cell, want_cells = D.play_edge(driver, src, kept, target)
            assert (F(cell).tobytes(), cells) == (want_cell.tobytes(), want_cells), (target, cell, cells, want_cell, want_cells)
            assert 1 <= cells <= target and v.models[SRC].decimate_count(cell, flt, invert).cells == cells
        # nobody participates: edge 0, no cells
        v.models[SRC].gaussian_buffers.selection_buffer.upload(X.words(np.zeros(n, bool)))
        assert v.models[SRC].decimate_edge(10, X.SELECTED) == (0.0, 0)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_viewer_renders_on():
    n = 500
    g = common.small_scene(n, 82)
    with MultiModelViewer() as v, MultiModelViewer() as other:
        _load(v, g)
        _load(v, g[:10], "held")
        L = v._L
        reference = _frames(v, [SRC], poses=(9,))[0]
        stats, cell, cells = _lib.DecimateStats(), C.c_float(), C.c_uint64()

        def call(src=SRC, dst=b"new", desc=None, viewer=v, out=stats, **fields):
            d = _lib.DecimateDesc(0, 0, 0.5, 0)
            for k, val in fields.items():
                setattr(d, k, val)
            return L.gsx_model_decimate(viewer._h if viewer else None, src.encode() if src else None, dst, C.byref(d) if desc is None else desc, None,
                                        C.byref(out) if out is not None else None)

        bad = _lib.GSX_ERR_INVALID_ARG
        assert call(viewer=None) == bad and call(src=None) == bad and call(out=None) == bad
        assert L.gsx_model_decimate(v._h, SRC.encode(), b"new", None, None, C.byref(stats)) == bad  # a null desc
        assert call(filter=8) == bad and call(flags=2) == bad and call(flags=4) == bad and call(grid_bits=25) == bad
        for c in (0.0, -1.0, float("nan"), float("inf"), 1e-39):
            assert call(cell=c) == bad, c
        r = _lib.DecimateDesc(0, 0, 0.5, 0, (0, 1))
        assert call(desc=C.byref(r)) == bad
        r = _lib.DecimateDesc(0, 0, 0.5, 0, (1, 0))
        assert call(desc=C.byref(r)) == bad
        assert call(dst=b"held") == bad and call(dst=SRC.encode()) == bad
        assert b"gsx_model_decimate" in L.gsx_last_error_string()
        assert call(src="nope") == _lib.GSX_ERR_NOT_FOUND
        edge = lambda key, flt, flags, target: L.gsx_model_decimate_edge(v._h, key, flt, flags, target, C.byref(cell), C.byref(cells))  # noqa: E731
        assert edge(SRC.encode(), 0, 0, 0) == bad and edge(SRC.encode(), 8, 0, 5) == bad and edge(SRC.encode(), 0, 2, 5) == bad and edge(None, 0, 0, 5) == bad
        assert L.gsx_model_decimate_edge(v._h, SRC.encode(), 0, 0, 5, None, C.byref(cells)) == bad
        assert edge(b"nope", 0, 0, 5) == _lib.GSX_ERR_NOT_FOUND
        assert _len(v, "new")[0] == _lib.GSX_ERR_NOT_FOUND and sorted(v.models) == sorted([SRC, "held"])
        assert np.array_equal(_frames(v, [SRC], poses=(9,))[0], reference)  # the viewer still renders src
        assert call() == _lib.GSX_OK and stats.cells > 0 and _len(v, "new")[0] == _lib.GSX_OK  # (the arguments of `call` are good ones)
        # a sharded model
        v.shard_set_limits(SRC, np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        assert call(dst=b"new2") == _lib.GSX_ERR_UNSUPPORTED and edge(SRC.encode(), 0, 0, 5) == _lib.GSX_ERR_UNSUPPORTED
        # a viewer with a communicator
        _load(other, g[:50])
        group = CommGroup(1)
        other.comm_init_group(group, 0)
        with pytest.raises(GsxError) as e:
            other.models[SRC].decimate(DST, 0.5)
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED and DST not in other.models
        with pytest.raises(GsxError) as e:
            other.models[SRC].decimate_edge(5)
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED


# ---- 9. one visual sanity check (not a gate on arithmetic) ---------------------------------------------------------------------------------
def test_a_twice_stored_model_draws_as_its_single_copy():
    """Every Gaussian twice, at the same place, at half the opacity mass; decimated with a tiny cell the model draws what the single
    copy draws, within spec section 8's framebuffer tolerance (confirmed for this fixture on the CPU oracle by
    tests/test_decimate_cpu.py)."""
    single, twice, rows, cell = D.twice_stored()
    n = single[0].shape[0]
    with MultiModelViewer() as v:
        K.upload_pod(v, "single", single)
        K.upload_pod(v, SRC, twice)
        got = v.models[SRC].decimate(DST, cell)
        assert (got.count, got.cells, got.singletons, got.largest_cell) == (2 * n, n, 0, 2)
        doubled = _frames(v, [SRC])
        for k, (a, b) in enumerate(zip(_frames(v, [DST]), _frames(v, ["single"]))):
            assert b[..., :3].max() > 0
            assert float(np.abs(a - b).max()) <= 1e-3, (k, float(np.abs(a - b).max()))
        assert float(np.abs(doubled[0] - _frames(v, ["single"])[0]).max()) > 1e-3  # (two half-opaque copies do not draw as one: the merge matters)
