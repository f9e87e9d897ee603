"""GPU: gsx_model_neighbors and gsx_model_select_neighbors (spec/RENDER_SPEC.md §18; csrc/kernels_neighbors.hip).  Equality is exact
everywhere.  The yardsticks: gsx_model_download_pod for the stored positions, the float32 definition tests/neighbors_ref.py: brute on
them (tests/test_neighbors_cpu.py checks its lattice and coincident expectations and ties the cell function to
csrc/neighbors_math.h), tests/extract_ref.py for the filter, gsx_model_upload_selection for the frames.
Sizes: a workgroup of the passes in index order takes 1024 Gaussians in four rounds of 256, a wave 64 of them (two words of a bit
plane), a workgroup of the query 256 records: one Gaussian, two, a word and wave edge (63, 64, 65), a round edge (256, 257), a chunk
edge (1024, 1025), several chunks with a partial last one (5000).  No kernel caps its grid: every workgroup takes one chunk."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import extract_ref as X
from tests import neighbors_ref as N
from tests.model_ops import H, W, frames as _frames, load as _load, pod as _pod
from wgpu_3dgs_viewer_app_amd import _lib, query
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as EF
from wgpu_3dgs_viewer_app_amd.viewer import CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
SRC = "src"
F = np.float32
SIZES = [1, 2, 63, 64, 65, 256, 257, 1024, 1025, 5000]
HIGHLIGHT = (1.0, 0.0, 1.0, 0.3)


def _radius(pos, k=4):
    """a radius under which the median count is a few: the median distance to the k-th nearest other point, over a sample"""
    p = np.ascontiguousarray(pos, F)
    p = p[np.isfinite(p).all(axis=1)]
    if p.shape[0] <= k:
        return F(1.0)
    d2 = np.sort(N._d2(p[:: max(1, p.shape[0] // 256)], p), axis=1)[:, k]  # (column 0 is the point itself)
    return F(np.sqrt(np.median(d2.astype(np.float64))))


def _scene_model(v, g, key=SRC):
    _load(v, g, key)
    return v.models[key], _pod(v, key)[0]


def _check(got, pos, part, r, cap=N.MAX_COUNT, what="", want=None):
    want = N.brute(pos, part, r, cap) if want is None else want
    assert np.array_equal(got.counts, want), what
    assert np.array_equal(got.hist, N.hist(want, part, cap)), what
    assert got.count == int(part.sum()) == int(got.hist.sum()), what
    return want


def _filter_model(v, n, seed=7, key=SRC):
    """tests/test_gpu_property.py's recipe restated: a model with a mask, a selection (garbage in both tails) and stored edits (some
    ENABLED + HIDDEN), NaN and infinite positions (when it has room for them); returns the host arrays"""
    g = common.small_scene(n, seed, 0)
    if n >= 64:
        g["pos"][5, 0], g["pos"][n // 2, 0], g["pos"][n - 1, 0], g["pos"][7, 1] = np.nan, np.inf, -np.inf, np.nan
    rng = np.random.default_rng(seed)
    mask, sel = rng.random(n) < 0.6, rng.random(n) < 0.4
    mask[[0, n - 1]], sel[[0, n // 2]] = True, True
    edits = query.default_edits(n)
    edits["flag"][0::3] = int(EF.ENABLED | EF.HIDDEN)
    edits["flag"][1::3] = int(EF.ENABLED)
    edits["flag"][5::7] |= int(EF.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    _load(v, g, key)
    bufs = v.models[key].gaussian_buffers
    bufs.mask_buffer.upload(X.words(mask, True))
    bufs.selection_buffer.upload(X.words(sel, True))
    bufs.gaussians_edit_buffer.upload(edits)
    return g, mask, sel, bufs.gaussians_edit_buffer.download()["flag"]


def _passes(n, flt, mask=None, sel=None, flags=None):
    out = np.zeros(n, bool)
    out[X.kept(n, flt, 0, mask, sel, flags)] = True
    return out


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_counts_at_the_edges_of_the_passes(n):
    g = common.small_scene(n, 300 + n, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        r = _radius(pos)
        every = np.ones(n, bool)
        got = m.neighbors(r)
        want = _check(got, pos, every, r, what=n)
        assert (got.n_nonfinite, got.grid_bits) == (0, N.auto_bits(n))
        if n >= 256:
            assert 1 <= np.median(want) <= 16  # (the regime the radius is chosen for)
        # a cap below the largest count: saturated counts, the histogram's last bin holds the rest
        cap = max(1, int(want.max()) // 2)
        capped = m.neighbors(r, cap)
        _check(capped, pos, every, r, cap, (n, "capped"), want=np.minimum(want, cap).astype(np.uint32))
        assert capped.hist.size == cap + 1


# ---- 2. engineered sets -----------------------------------------------------------------------------------------------------------------
def _with_pos(pos):
    g = common.small_scene(pos.shape[0], 5, 0)
    g["pos"] = pos
    return g


def _points_model(v, pos, key=SRC):
    return _scene_model(v, _with_pos(pos), key)


def test_lattice_at_exactly_the_radius():
    lat = N.lattice()
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, lat)
        assert pos.tobytes() == lat.tobytes()
        every = np.ones(lat.shape[0], bool)
        got = m.neighbors(0.25)
        _check(got, pos, every, 0.25, what="lattice")
        k = np.rint(lat / F(0.25)).astype(int)
        assert np.array_equal(got.counts, 6 - (np.abs(k) == 4).sum(axis=1)) and (got.counts[(np.abs(k) < 4).all(axis=1)] == 6).all()
        below = m.neighbors(float(np.nextafter(F(0.25), F(0))))
        assert not below.counts.any() and below.hist[0] == lat.shape[0] == below.count
        for bits in (1, 3, 12):  # the six neighbours' cells meet in shared buckets
            assert np.array_equal(m.neighbors(0.25, grid_bits=bits).counts, got.counts), bits


@pytest.mark.parametrize("cap", [1, 7, 299, 4095])
def test_coincident_points(cap):
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, same)
        got = m.neighbors(0.5, cap)
        assert (got.counts == min(299, cap)).all()
        assert got.hist[min(299, cap)] == 300 == got.count and np.count_nonzero(got.hist) == 1 and got.hist.size == cap + 1
        _check(got, pos, np.ones(300, bool), 0.5, cap, cap)


def test_table_size_changes_nothing():
    g = common.small_scene(2000, 41, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        r = _radius(pos, 6)
        want = N.brute(pos, np.ones(2000, bool), r)
        for bits in (1, 2, 4, 10, 0):  # two buckets: every visited cell aliases with others
            got = m.neighbors(r, grid_bits=bits)
            _check(got, pos, np.ones(2000, bool), r, what=bits, want=want)
            assert got.grid_bits == (bits or N.auto_bits(2000))
        assert m.neighbors(r, grid_bits=24).counts.tobytes() == want.tobytes()


def test_far_huge_and_non_finite_positions():
    planted, r = N.special_scene(3000)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, planted)
        assert pos.tobytes() == planted.tobytes()  # NaN, inf and 3e38 are stored as they are
        part = N.participates(pos)
        got = m.neighbors(r)
        _check(got, pos, part, r, what="special")
        assert (got.n_nonfinite, got.count) == (3, 3000 - 3)
        assert got.counts[10] == got.counts[11] == 1          # the coincident pair at 1e6: each other's only neighbour
        assert not got.counts[12:20].any()                    # lone far points; NaN / inf: count 0
        assert (got.counts[20:31] >= 10).all()
        # the non-finite ones are nobody's neighbour: without them, the others' counts are the same
        _load(v, _with_pos(pos[part]), "finite")
        assert np.array_equal(v.models["finite"].neighbors(r).counts, got.counts[part])
        for bits in (1, 5):
            assert np.array_equal(m.neighbors(r, grid_bits=bits).counts, got.counts), bits


# ---- 3. filter --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1025, 2500])
def test_every_filter_combination(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 400 + n)
        _load(v, g, "bare")  # the same Gaussians without mask, selection and edit records
        pos = _pod(v)[0]
        r = _radius(pos, 8)
        finite = N.participates(pos)
        for key, planes in ((SRC, (mask, sel, flags)), ("bare", (None, None, None))):
            for flt in range(8):
                passes = _passes(n, flt, *planes)
                part = passes & finite
                got = v.models[key].neighbors(r, filter=flt)
                want = _check(got, pos, part, r, what=(key, flt))
                assert got.n_nonfinite == int((passes & ~finite).sum()), (key, flt)
                assert not got.counts[~part].any()
                # ... and they are nobody's neighbour: the counts are those of the participants alone
                assert np.array_equal(want[part], N.brute(pos[part], np.ones(int(part.sum()), bool), r)), (key, flt)
        assert v.models["bare"].neighbors(r, filter=X.SELECTED).count == 0  # SELECTED of a model without a selection: none


# ---- 4. select --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1025, 2500])
def test_select_against_the_restatement(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 500 + n)
        m = v.models[SRC]
        sb = m.gaussian_buffers.selection_buffer
        pos = _pod(v)[0]
        r = _radius(pos, 8)
        finite = N.participates(pos)
        for prior in ("random", None):
            for flt in (0, X.SELECTED, X.MASKED | X.SKIP_HIDDEN, 7):
                part = _passes(n, flt, mask, sel if prior else None, flags) & finite  # SELECTED reads the selection as it was
                full = N.brute(pos, part, r)
                for cap, lo, hi in ((N.MAX_COUNT, 2, 5), (3, 0, 2), (4, 4, 4)):
                    hit = N.hits(np.minimum(full, cap), part, lo, hi)
                    for op in (N.SET, N.ADD, N.REMOVE):
                        sb.upload(X.words(sel, True) if prior else None)  # (garbage in the tail bits of the prior selection)
                        old = sel if prior else np.zeros(n, bool)
                        want = hit if op == N.SET else (old | hit if op == N.ADD else old & ~hit)
                        nb = m.neighbors(r, cap, filter=flt)
                        got = m.select_neighbors(r, lo, hi, cap, op, flt)
                        assert got == (int(hit.sum()), int(want.sum())), (prior, op, flt, cap, got)
                        assert got[0] == int(nb.hist[lo:hi + 1].sum()), (prior, op, flt, cap)
                        assert np.array_equal(sb.download(), X.words(want)), (prior, op, flt, cap)  # tail bits zero
        # the out pointers are optional; a forced table gives the same selection
        desc = _lib.NeighborSelectDesc(0, 0, N.SET, 3, float(r), 0, 2, 1)
        assert v._L.gsx_model_select_neighbors(v._h, SRC.encode(), C.byref(desc), None, None) == _lib.GSX_OK
        assert np.array_equal(sb.download(), X.words(N.hits(N.brute(pos, finite, r, 3), finite, 0, 2)))


FINISH_N = 256 * 1024 + 1  # 257 workgroups' partials: the smallest n at which a lane of the one-workgroup finish takes a second one


def _finish_lattice():
    """FINISH_N points of the integer lattice, Gaussian i at (i mod 64, i / 64 mod 64, i / 4096): every nearest distance is 1"""
    i = np.arange(FINISH_N)
    return np.stack([i % 64, (i // 64) % 64, i // 4096], axis=1).astype(F)


def _selection_is(sb, on):
    return np.array_equal(sb.download(), X.words(np.full(FINISH_N, on, bool)))  # (all ones and a cleared tail, or all zeros)


def test_select_sums_more_partials_than_the_finish_has_lanes():
    n = FINISH_N
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, _ = _points_model(v, _finish_lattice())
        sb = m.gaussian_buffers.selection_buffer
        got = m.neighbors(0.25, 7)
        assert got.count == n and got.hist[0] == n and not got.hist[1:].any()
        assert m.select_neighbors(0.25, 0, 0, 7, N.SET) == (n, n) and _selection_is(sb, True)
        assert m.select_neighbors(0.25, 0, 0, 7, N.REMOVE) == (n, 0) and _selection_is(sb, False)
        assert m.select_neighbors(0.25, 1, 7, 7, N.SET) == (0, 0) and _selection_is(sb, False)


def test_floaters_recipe_then_extract_and_frames():
    n, k = 2500, 3
    g = common.small_scene(n, 37)
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _load(vv, g)
            vv.update_selection_edit_with_pod(query.GaussianEditPod(EF.ENABLED, alpha=0.6))
            vv.update_selection_highlight(HIGHLIGHT)
        m = v.models[SRC]
        pos = _pod(v)[0]
        r = _radius(pos, 4)
        plain = _frames(v, [SRC], poses=(4,))[0]
        assert np.array_equal(plain, _frames(twin, [SRC], poses=(4,))[0])
        counts = N.brute(pos, np.ones(n, bool), r)
        floaters = counts < k
        assert 0 < floaters.sum() < n
        # a model without a selection gets one
        assert m.select_neighbors(r, 0, k - 1) == (int(floaters.sum()), int(floaters.sum()))
        words = m.gaussian_buffers.selection_buffer.download()
        assert np.array_equal(words, X.words(floaters))
        # the frames with the highlight on: those of a twin whose selection was uploaded from the host with the same words
        twin.models[SRC].gaussian_buffers.selection_buffer.upload(words)
        got, want = _frames(v, [SRC], poses=(4, 5, 6, 7)), _frames(twin, [SRC], poses=(4, 5, 6, 7))
        assert not np.array_equal(got[0], plain)  # (the selection shows)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        # "delete the floaters": what is left is what the definition predicts
        assert m.extract("kept", X.SELECTED, invert=True) == n - int(floaters.sum())
        assert _pod(v, "kept")[0].tobytes() == pos[~floaters].tobytes()


def _lane_sequence(g, lanes, on_device, r):
    out = []
    with MultiModelViewer() as v:
        v.set_render_options(frames_in_flight=lanes)
        _load(v, g)
        v.update_selection_edit_with_pod(query.GaussianEditPod(EF.ENABLED, alpha=0.6))
        v.update_selection_highlight(HIGHLIGHT)
        m = v.models[SRC]
        for pose in (1, 2, 3, 4):
            out += _frames(v, [SRC], poses=(pose,))
        if on_device:
            m.select_neighbors(r, 0, 3)  # behind the frames in flight on the lanes
        else:
            m.gaussian_buffers.selection_buffer.upload(X.words(N.brute(_pod(v)[0], np.ones(g.shape[0], bool), r) <= 3))
        for pose in (5, 6, 7, 8):
            out += _frames(v, [SRC], poses=(pose,))
    return out


def test_lanes():
    g = common.small_scene(2500, 38)
    r = _radius(g["pos"], 4)
    two, one, host = _lane_sequence(g, 2, True, r), _lane_sequence(g, 1, True, r), _lane_sequence(g, 2, False, r)
    assert len(two) == 8 and two[0][..., :3].max() > 0
    for k, (a, b, c) in enumerate(zip(two, one, host)):
        assert np.array_equal(a, b) and np.array_equal(a, c), k


# ---- 5. independence ----------------------------------------------------------------------------------------------------------------------
def test_pod_kind_transform_and_repetition_change_nothing():
    n = 3000
    g = common.small_scene(n, 71)
    tr = common.odd_transform()
    results = []
    for sh, cov in ((ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)):
        with MultiModelViewer(sh=sh, cov3d=cov) as v:
            m, pos = _scene_model(v, g)
            r = _radius(pos, 5)
            a = m.neighbors(r)
            _check(a, pos, np.ones(n, bool), r, what=(sh, cov))
            b = m.neighbors(r)
            assert a.counts.tobytes() == b.counts.tobytes() and a.hist.tobytes() == b.hist.tobytes() and (a.count, a.n_nonfinite) == (b.count, b.n_nonfinite)
            v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)  # model space: the transform changes nothing
            c = m.neighbors(r)
            assert a.counts.tobytes() == c.counts.tobytes() and a.hist.tobytes() == c.hist.tobytes()
            first = m.select_neighbors(r, 0, 2)
            words = m.gaussian_buffers.selection_buffer.download()
            assert m.select_neighbors(r, 0, 2) == first and np.array_equal(m.gaussian_buffers.selection_buffer.download(), words)
            results.append((float(r), a.counts.tobytes()))
    assert results[0] == results[1]  # the position plane is float32 in every pod kind


# ---- 6. workspace, and what a count writes -------------------------------------------------------------------------------------------------
def test_workspace_and_the_model_is_not_written():
    n = 3000
    before = viewer_mod.device_bytes()
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _filter_model(vv, n, 51)
        m = v.models[SRC]

        def state(vv):
            bufs = vv.models[SRC].gaussian_buffers
            return [a.tobytes() for a in _pod(vv)] + [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(),
                                                      bufs.gaussians_edit_buffer.download().tobytes()]

        start = state(v)
        assert np.array_equal(_frames(v, [SRC], poses=(5,))[0], _frames(twin, [SRC], poses=(5,))[0])
        r = _radius(_pod(v)[0], 5)
        m.neighbors(r)  # (the first call sizes the shared workspace)
        held = viewer_mod.device_bytes()
        for flt in (0, 3, 7):
            m.neighbors(r, 16, filter=flt)
            m.neighbors(r * F(2), filter=flt)
        assert viewer_mod.device_bytes() == held
        assert state(v) == start == state(twin)
        for a, b in zip(_frames(v, [SRC], poses=(6, 7)), _frames(twin, [SRC], poses=(6, 7))):
            assert np.array_equal(a, b)
        held = viewer_mod.device_bytes()  # (the frames have sized their own buffers)
        m.select_neighbors(r, 0, 2, filter=3)
        m.neighbors(r)
        assert viewer_mod.device_bytes() == held  # (the model has a selection buffer already)
    assert viewer_mod.device_bytes() == before  # released with the viewer


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors():
    """every refusal of spec section 18 but GSX_ERR_OOM, which a test cannot provoke without exhausting the device"""
    n = 300
    with MultiModelViewer() as v, MultiModelViewer() as other:
        g, mask, sel, flags = _filter_model(v, n, 61)
        L, key = v._L, SRC.encode()
        sb = v.models[SRC].gaussian_buffers.selection_buffer
        sel_before = sb.download()
        counts, hist, stats = np.zeros(n, np.uint32), np.zeros(4096, np.uint64), _lib.NeighborStats()
        hit, selected = C.c_uint64(), C.c_uint64()
        INV, NF, UNS = _lib.GSX_ERR_INVALID_ARG, _lib.GSX_ERR_NOT_FOUND, _lib.GSX_ERR_UNSUPPORTED

        def neighbors(k=key, flt=0, flags_=0, radius=0.1, cap=16, bits=0, reserved=0, desc=True, st=stats, vv=v):
            d = _lib.NeighborDesc(flt, flags_, radius, cap, bits, reserved)
            return L.gsx_model_neighbors(vv._h if vv else None, k, C.byref(d) if desc else None, counts.ctypes.data, hist.ctypes.data,
                                         C.byref(st) if st is not None else None)

        def select(k=key, flt=0, flags_=0, op=0, cap=16, radius=0.1, lo=0, hi=3, bits=0, reserved=(0, 0), desc=True, vv=v):
            d = _lib.NeighborSelectDesc(flt, flags_, op, cap, radius, lo, hi, bits, (C.c_uint32 * 2)(*reserved))
            return L.gsx_model_select_neighbors(vv._h if vv else None, k, C.byref(d) if desc else None, C.byref(hit), C.byref(selected))

        bad_radii = (0.0, -1.0, float("nan"), float("inf"), 1e-23, 1.9e19)  # (1e-23: the square is 0; 1.9e19: the square is inf)
        cases = [
            (neighbors(vv=None), INV), (neighbors(k=None), INV), (neighbors(desc=False), INV), (neighbors(st=None), INV),
            (neighbors(flt=8), INV), (neighbors(flags_=1), INV), (neighbors(cap=0), INV), (neighbors(cap=4096), INV), (neighbors(bits=25), INV),
            (neighbors(reserved=1), INV), (neighbors(k=b"nope"), NF),
            (select(vv=None), INV), (select(k=None), INV), (select(desc=False), INV), (select(flt=8), INV), (select(flags_=1), INV),
            (select(op=3), INV), (select(cap=0), INV), (select(cap=4096), INV), (select(bits=25), INV), (select(lo=3, hi=2), INV),
            (select(cap=16, hi=17), INV), (select(reserved=(1, 0)), INV), (select(reserved=(0, 1)), INV), (select(k=b"nope"), NF),
        ] + [(neighbors(radius=r), INV) for r in bad_radii] + [(select(radius=r), INV) for r in bad_radii]
        for i, (got, want) in enumerate(cases):
            assert got == want, i
        assert b"gsx_model_select_neighbors" in L.gsx_last_error_string()
        assert np.array_equal(sb.download(), sel_before)  # a refused select leaves the selection
        # the ends of the legal ranges; the counts and the histogram are optional
        assert neighbors(cap=4095, bits=24, radius=4e-23) == _lib.GSX_OK and neighbors(cap=1, bits=1, radius=1.8e19) == _lib.GSX_OK
        d = _lib.NeighborDesc(0, 0, 0.1, 16, 0, 0)
        assert L.gsx_model_neighbors(v._h, key, C.byref(d), None, None, C.byref(stats)) == _lib.GSX_OK and stats.count == n - 4
        # an empty model, and no participants: GSX_OK with zeros; Set then clears the selection
        v.add_model("empty", 0)
        e = v.models["empty"]
        got = e.neighbors(0.1, 8)
        assert (got.counts.size, got.count, got.n_nonfinite) == (0, 0, 0) and not got.hist.any() and got.hist.size == 9
        assert e.select_neighbors(0.1, 0, 3) == (0, 0)
        _load(v, g, "bare")
        none = v.models["bare"].neighbors(0.1, 8, filter=X.SELECTED)
        assert (none.count, none.n_nonfinite) == (0, 0) and not none.counts.any() and not none.hist.any()
        assert v.models[SRC].select_neighbors(1e-6, 5, 8, 8) == (0, 0) and not sb.download().any()
        # a sharded model; a viewer with a communicator
        _frames(v, [SRC], poses=(5,))
        _load(v, g[:50], "b")
        v.shard_set_limits("b", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        _load(other, g[:50], "a")
        other.comm_init_group(CommGroup(1), 0)
        for model, word in ((v.models["b"], "shard"), (other.models["a"], "communicator")):
            for call in (lambda: model.neighbors(0.1), lambda: model.select_neighbors(0.1, 0, 3)):
                with pytest.raises(GsxError) as err:
                    call()
                assert err.value.status == UNS and word in str(err.value)
