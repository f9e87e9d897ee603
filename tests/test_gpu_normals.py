"""GPU: gsx_model_normals and gsx_model_select_normals (spec/RENDER_SPEC.md §26; csrc/kernels_normals.hip).  The neighbour lists,
the counts, the minimum, the maximum and every selection word are compared exactly; the lists' d2 with gsx_model_knn's rows bit for
bit; normals and variations with the host replay tests/normals_driver.cpp (csrc/normals_math.h compiled for the host) bit for bit, and
with the numpy definition tests/normals_ref.py (numpy.linalg.eigh) within the bounds tests/test_normals_cpu.py derives: the variation
within 1 float32 ulp of the reference's (plus the reference's own 2^-50 on the rows whose reference lies below 2^-26), every component
of a certain normal within 2^-23, the sign included wherever the reference decides it.  `mean` is a
sum of m <= 5000 values in [0, 1/3] in double divided by m: any order of the adds is within m * 2^-53 of the exact sum, relatively, so
two orders differ by at most 1.2e-12; the bound is §20's 2e-12.
Sizes: a workgroup of the passes in index order takes 1024 Gaussians in four rounds of 256, a wave 64 of them, a workgroup of the
query 256 entries; up to 1024 participants go straight to the exact fallback: 1, 3 (fewer than k + 1), 4 (k + 1 at k = 3), a wave
edge (63, 64, 65), a round edge (256, 257), the chunk and straight-to-fallback edge (1024, 1025), several chunks with a partial last
one (5000).  k: the template edges 4 | 5 and 8 | 9 and both ends 3 and 16."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import common
from tests import extract_ref as X
from tests import neighbors_ref as N
from tests import normals_ref as R
from tests.model_ops import H, W, frames as _frames, load as _load, pod as _pod
from tests.test_gpu_knn import _filter_model, _passes, _points_model, _scene_model
from tests.test_normals_cpu import CSRC, ROOT, check_fit, at_most_three_points, search
from wgpu_3dgs_viewer_app_amd import _lib
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.viewer import CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
SRC = "src"
F = np.float32
SIZES = [1, 3, 4, 63, 64, 65, 256, 257, 1024, 1025, 5000]
KS = [3, 4, 5, 8, 9, 16]
MEAN_RTOL = 2e-12


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("normals_gpu") / "normals_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "normals_driver.cpp"), "-o", exe])
    return exe


def _list_d2(pos, index):
    """the float32 d2 between every Gaussian and its listed neighbours, +inf where there is none"""
    none = index == R.NONE
    with np.errstate(over="ignore", invalid="ignore"):
        d = (pos[:, None, :] - pos[np.where(none, 0, index).astype(np.int64)]).astype(F)
        sq = (d * d).astype(F)
        d2 = ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)
    return np.where(none, R.INF, d2)


def _check_stats(got, part, nonfinite=0, what=""):
    want = R.stats(got.variation)
    assert (got.count, got.n_nonfinite, got.n_fitted) == (int(part.sum()), nonfinite, want["n_fitted"]), what
    assert got.variation_min.tobytes() == F(want["variation_min"]).tobytes() and got.variation_max.tobytes() == F(want["variation_max"]).tobytes(), what
    assert got.mean == pytest.approx(want["mean"], rel=MEAN_RTOL, abs=0), what


def _check(got, pos, part, k, full=None, nonfinite=0, what="", tiny_rows=None, **orient):
    """got: a ModelNormals with indices; full: normals_ref.lists with at least k columns (computed here without)"""
    index, d2 = R.lists(pos, part, k) if full is None else (full[0][:, :k], full[1][:, :k])
    # (a prefix of a longer list is the shorter list)
    assert np.array_equal(got.index, index), what
    want = R.fit(pos, index, d2, **orient)
    check_fit(got.normal, got.variation, want, what, tiny_rows)
    _check_stats(got, part, nonfinite, what)
    return want


def _same_words(a, b):
    return (a.normal.tobytes(), a.variation.tobytes(), None if a.index is None else a.index.tobytes(), a.count, a.n_nonfinite, a.n_fitted,
            a.variation_min.tobytes(), a.variation_max.tobytes(), a.mean) == \
        (b.normal.tobytes(), b.variation.tobytes(), None if b.index is None else b.index.tobytes(), b.count, b.n_nonfinite, b.n_fitted,
         b.variation_min.tobytes(), b.variation_max.tobytes(), b.mean)


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_lists_fits_and_statistics_at_the_edges_of_the_passes(driver, n):
    g = common.small_scene(n, 700 + n, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        every = np.ones(n, bool)
        full = R.lists(pos, every, 16)
        for k in KS:
            got = m.normals(k, indices=True)
            _check(got, pos, every, k, full, what=(n, k))
            assert _list_d2(pos, got.index).tobytes() == m.knn(k, rows=True).d2.tobytes()  # the lists' d2 are the nearest neighbours' rows
            assert got.grid_bits == N.auto_bits(n) and got.rounds + got.n_brute >= 1
            if n <= 1024:
                assert (got.rounds, got.n_brute) == (0, n)  # straight to the exact fallback
            else:
                assert got.rounds >= 1
            if n <= k:  # fewer than k others: nobody is fitted
                assert (got.index[:, n - 1:] == R.NONE).all() and np.isinf(got.variation).all() and not got.normal.any()
                assert (got.n_fitted, got.mean, got.variation_min, got.variation_max) == (0, 0, 0, 0)
            elif n > 4:
                assert got.n_fitted == n
            # the host replay of csrc/normals_math.h: the same bits (the definition loop of the driver only at the small sizes)
            replay = search(driver, pos, k, command="search" if n <= 1025 else "replay")
            assert np.array_equal(got.index, replay["index"]) and got.normal.tobytes() == replay["normal"].tobytes(), (n, k)
            assert got.variation.tobytes() == replay["variation"].tobytes(), (n, k)
            assert (got.n_fitted, got.variation_min, got.variation_max) == (replay["n_fitted"], replay["variation_min"], replay["variation_max"])
            assert got.mean == pytest.approx(replay["mean"], rel=MEAN_RTOL, abs=0)
            without = m.normals(k)  # the indices are optional, and nothing else depends on them
            assert without.index is None and without.normal.tobytes() == got.normal.tobytes() and without.variation.tobytes() == got.variation.tobytes()


@pytest.mark.parametrize("family", [f[0] for f in R.FAMILIES])
def test_the_three_families(driver, family):
    pos = dict(R.FAMILIES)[family](3000, 17)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, stored = _points_model(v, pos)
        assert stored.tobytes() == pos.tobytes()
        every = np.ones(3000, bool)
        full = R.lists(pos, every, 16)
        for k in (3, 8, 16):
            got = m.normals(k, indices=True)
            want = _check(got, pos, every, k, full, what=(family, k))
            assert (want["fitted"] & ((want["gap"] < R.CERTAIN) | ~want["signed"])).sum() <= 0.01 * 3000
            replay = search(driver, pos, k, command="replay")
            assert np.array_equal(got.index, replay["index"]) and got.normal.tobytes() == replay["normal"].tobytes()
            assert got.variation.tobytes() == replay["variation"].tobytes()


# ---- 2. the knobs change nothing ------------------------------------------------------------------------------------------------------
def test_the_knobs_change_nothing():
    n = 5000
    g = common.small_scene(n, 730, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        every = np.ones(n, bool)
        base = m.normals(9, indices=True)
        _check(base, pos, every, 9, what="default")
        assert base.rounds >= 1
        r = float(base.first_radius)
        sb = m.gaussian_buffers.selection_buffer
        m.select_normals(9, 0.0, 0.05)
        words = sb.download()
        paths = set()
        for what, kw in (("hint x 100", dict(radius_hint=r * 100)), ("hint / 100", dict(radius_hint=r / 100)), ("16 buckets", dict(grid_bits=4)),
                         ("2^20 buckets", dict(grid_bits=20)), ("one round", dict(max_rounds=1)),
                         ("all", dict(radius_hint=r / 100, grid_bits=4, max_rounds=1))):
            got = m.normals(9, indices=True, **kw)
            assert _same_words(got, base), what
            assert got.grid_bits == kw.get("grid_bits", N.auto_bits(n))
            paths.add((got.rounds, got.n_brute))
            sb.upload(None)
            assert m.select_normals(9, 0.0, 0.05, **kw)[:2] == (int(X.bits(words, n).sum()),) * 2 and np.array_equal(sb.download(), words), what
        assert len(paths) >= 3  # the paths differ; the words do not
        assert _same_words(m.normals(9, indices=True), base)  # nor does repetition


# ---- 3. engineered sets -----------------------------------------------------------------------------------------------------------------
def test_lattice_whose_kth_distance_ties_and_coincident_points(driver):
    lat = N.lattice(0.25, 11)  # 1331 points: past the straight-to-fallback edge, so the grid rounds answer
    same = np.tile(F([0.3, -1.7, 2.9]), (1300, 1))
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, lat)
        every = np.ones(lat.shape[0], bool)
        interior = (np.abs(np.rint(lat / F(0.25))) < 5).all(axis=1)
        for k in (5, 6, 7):  # six at exactly 0.25: at k = 5 the index decides who is left out
            got = m.normals(k, indices=True)
            index, d2 = R.lists(pos, every, k)
            assert np.array_equal(got.index, index) and got.n_fitted == lat.shape[0]
            for bits in (1, 3):
                assert _same_words(m.normals(k, indices=True, grid_bits=bits), got)
            if k == 6:  # isotropic: 1/3; the normals are not compared
                third = np.full(int(interior.sum()), 1.0 / 3.0, F)
                assert (np.abs(got.variation[interior].astype(np.float64) - third.astype(np.float64)) <= np.spacing(third)).all()
        for n, k in ((300, 16), (1300, 16), (1300, 5)):  # through the exact fallback, and through grid rounds that may not stop at k zeros
            m, pos = _points_model(v, same[:n], f"same{n}k{k}")
            got = m.normals(k, indices=True)
            want = np.tile(np.arange(k, dtype=np.uint32), (n, 1))
            want[:k] += np.triu(np.ones((k, k), np.uint32))  # (i's own index is skipped)
            assert np.array_equal(got.index, want)  # the k smallest indices, whoever was seen first
            assert (got.count, got.n_fitted, got.mean) == (n, 0, 0) and np.isinf(got.variation).all() and not got.normal.any()
            assert m.select_normals(k, 0.0, np.inf)[:2] == (0, 0)  # not fitted: never hit
        rng = np.random.default_rng(6)
        groups = np.concatenate([np.tile(rng.random((40, 1, 3)), (1, 3, 1)).reshape(-1, 3), np.tile(rng.random((4, 1, 3)), (1, 40, 1)).reshape(-1, 3),
                                 rng.random((1200, 3))]).astype(F)
        m, pos = _points_model(v, groups, "groups")
        got = m.normals(8, indices=True)
        _check(got, pos, np.ones(groups.shape[0], bool), 8, what="groups", tiny_rows=at_most_three_points(pos, got.index))
        assert np.isinf(got.variation[120:280]).all() and (got.index[120:280] != R.NONE).all()
        replay = search(driver, pos, 8)
        assert np.array_equal(got.index, replay["index"]) and got.normal.tobytes() == replay["normal"].tobytes()


def test_the_plane_and_the_sphere():
    rng = np.random.default_rng(8)
    plane = np.concatenate([rng.random((1300, 2)) * 4 - 2, np.zeros((1300, 1))], axis=1).astype(F)
    vec = rng.normal(size=(1500, 3))
    radial = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    centre, far = (1.0, -2.0, 0.5), (1000.0, 0.0, 0.0)
    sphere = (radial * 2.0 + centre).astype(F)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, _ = _points_model(v, plane, "plane")
        for k in (3, 8, 16):
            got = m.normals(k)
            assert got.n_fitted == 1300 and (got.normal == F([0, 0, 1])).all() and not got.variation.any()  # exactly
            assert (got.normal.view(np.uint32)[:, :2] == 0).all() and (got.variation_min, got.variation_max, got.mean) == (0, 0, 0)
        assert (m.normals(8, toward=(0.0, 0.0, -5.0)).normal == F([0, 0, -1])).all()
        assert (m.normals(8, toward=(0.5, 0.5, 0.0)).normal == F([0, 0, 1])).all()  # a dot product of exactly 0: the canonical rule
        m, pos = _points_model(v, sphere, "sphere")
        inward = m.normals(8, toward=centre, indices=True)
        _check(inward, pos, np.ones(1500, bool), 8, what="sphere", orient=R.ORIENT_TOWARD, toward=centre)
        assert ((inward.normal.astype(np.float64) * radial).sum(axis=1) < -0.9).all()
        outward = m.normals(8, toward=far)
        assert (((np.asarray(far) - pos.astype(np.float64)) * outward.normal).sum(axis=1) > 0).all()
        assert np.array_equal(np.abs(outward.normal), np.abs(inward.normal)) and outward.variation.tobytes() == inward.variation.tobytes()
        canonical = m.normals(8)
        assert not R.canonical_flip(canonical.normal).any() and np.array_equal(np.abs(canonical.normal), np.abs(inward.normal))
        # facing without ABS follows the sign rule: looking at the centre, the cosine with the radial direction of a pole is negative
        up = (0.0, 0.0, 1.0)
        hit, _, _ = m.select_normals(8, 0.9, 1.0, direction=up, toward=centre)
        words = m.gaussian_buffers.selection_buffer.download()
        assert np.array_equal(words, X.words(R.hit(inward.normal, inward.variation, R.SELECT_FACING, 0.9, 1.0, up))) and hit > 0
        assert (radial[X.bits(words, 1500), 2] < -0.8).all()  # the bottom cap


def test_far_huge_and_non_finite_positions(driver):
    planted, _ = N.special_scene(3000)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, planted)
        assert pos.tobytes() == planted.tobytes()  # NaN, inf and 3e38 are stored as they are
        part = N.participates(pos)
        got = m.normals(4, indices=True)
        _check(got, pos, part, 4, nonfinite=3, what="special")
        assert not np.isnan(got.normal).any() and not np.isnan(got.variation).any()
        assert (got.index[15] == R.NONE).all() and (got.index[16] == R.NONE).all()  # every difference overflows: d2 = +inf, no index
        assert (got.index[17:20] == R.NONE).all() and np.isinf(got.variation[14:20]).all() and not got.normal[14:20].any()
        assert np.isinf(got.variation[20:31]).all() and (got.index[20:31] != R.NONE).all()  # eleven coincident points: a list, no plane
        assert got.n_brute >= 3
        assert _list_d2(pos, got.index).tobytes() == m.knn(4, rows=True).d2.tobytes()
        replay = search(driver, pos, 4, command="replay")
        assert np.array_equal(got.index, replay["index"]) and got.normal.tobytes() == replay["normal"].tobytes()
        assert got.variation.tobytes() == replay["variation"].tobytes()
        for kw in (dict(grid_bits=1), dict(radius_hint=1e-3), dict(radius_hint=1.8e19), dict(max_rounds=1)):
            assert _same_words(m.normals(4, indices=True, **kw), got), kw


# ---- 4. filter --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2500])
def test_every_filter_combination(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 800 + n)
        _load(v, g, "bare")  # the same Gaussians without mask, selection and edit records
        pos = _pod(v)[0]
        finite = N.participates(pos)
        for key, planes in ((SRC, (mask, sel, flags)), ("bare", (None, None, None))):
            for flt in range(8):
                passes = _passes(n, flt, *planes)
                part = passes & finite
                got = v.models[key].normals(4, indices=True, filter=flt)
                _check(got, pos, part, 4, nonfinite=int((passes & ~finite).sum()), what=(key, flt))
                assert (got.index[~part] == R.NONE).all() and np.isinf(got.variation[~part]).all() and not got.normal[~part].any()
        none = v.models["bare"].normals(4, filter=X.SELECTED)  # SELECTED of a model without a selection: none
        assert (none.count, none.n_fitted, none.rounds, none.n_brute) == (0, 0, 0, 0) and np.isinf(none.variation).all()


# ---- 5. select --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1500])
def test_select_against_hits_from_the_returned_normals(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 900 + n)
        m = v.models[SRC]
        sb = m.gaussian_buffers.selection_buffer
        pos = _pod(v)[0]
        finite = N.participates(pos)
        d = (0.3, -1.0, 0.5)
        for prior in ("random", None):
            for flt in (0, X.SELECTED, X.MASKED | X.SKIP_HIDDEN, 7):
                sb.upload(X.words(sel, True) if prior else None)
                part = _passes(n, flt, mask, sel if prior else None, flags) & finite  # SELECTED reads the selection as it was
                for k, toward in ((5, None), (8, (0.0, 0.0, 10.0))):
                    sb.upload(X.words(sel, True) if prior else None)
                    got = m.normals(k, toward=toward, filter=flt)
                    assert got.count == int(part.sum())
                    fitted = np.isfinite(got.variation)
                    lo, hi = (np.quantile(got.variation[fitted], [0.25, 0.75]) if fitted.any() else (0.0, 1.0))
                    for mode, flags_, kw in ((R.SELECT_VARIATION, 0, dict(lo=float(F(lo)), hi=float(F(hi)))), (R.SELECT_VARIATION, 0, dict(lo=float(F(hi)), hi=np.inf)),
                                             (R.SELECT_FACING, 0, dict(lo=0.2, hi=1.0, direction=d)), (R.SELECT_FACING, R.ABS, dict(lo=0.0, hi=0.5, direction=d)),
                                             (R.SELECT_FACING, 0, dict(lo=-np.inf, hi=-0.5, direction=d))):
                        hit = R.hit(got.normal, got.variation, mode, kw["lo"], kw["hi"], kw.get("direction"), flags_)
                        for op in (N.SET, N.ADD, N.REMOVE):
                            sb.upload(X.words(sel, True) if prior else None)  # (garbage in the tail bits of the prior selection)
                            old = sel if prior else np.zeros(n, bool)
                            got_hit, got_selected, gs = m.select_normals(k, op=op, filter=flt, toward=toward, absolute=bool(flags_), **kw)
                            what = (prior, flt, k, mode, flags_, kw, op)
                            assert (gs.count, gs.n_fitted, gs.mean) == (got.count, got.n_fitted, got.mean), what
                            assert gs.variation_min.tobytes() == got.variation_min.tobytes() and gs.variation_max.tobytes() == got.variation_max.tobytes(), what
                            want = hit if op == N.SET else (old | hit if op == N.ADD else old & ~hit)
                            assert (got_hit, got_selected) == (int(hit.sum()), int(want.sum())), what
                            assert np.array_equal(sb.download(), X.words(want)), what  # tail bits zero
        # the out pointers are optional
        words = sb.download()
        desc = _lib.NormalsSelectDesc(0, 0, N.REMOVE, R.SELECT_VARIATION, 8, 0, 1e-4, 1, 1, 1.0, 2.0, 0)
        assert v._L.gsx_model_select_normals(v._h, SRC.encode(), C.byref(desc), None, None, None) == _lib.GSX_OK
        assert np.array_equal(sb.download(), words)  # (no variation is above 1/3: nothing was removed)


def test_select_the_floor_then_bounds_of_the_selection():
    rng = np.random.default_rng(21)
    floor = np.concatenate([rng.random((3000, 2)) * 10 - 5, rng.normal(0.0, 0.002, (3000, 1)) - 1.0], axis=1)  # y, x in the plane z = -1, jittered
    blob = rng.normal(0.0, 0.4, (1500, 3)) + [0.0, 0.0, 1.0]
    pos = np.concatenate([floor, blob]).astype(F)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, stored = _points_model(v, pos)
        hit, selected, st = m.select_normals(8, 0.95, 1.0, direction=(0.0, 0.0, 1.0), absolute=True)
        got = m.normals(8)
        want = R.hit(got.normal, got.variation, R.SELECT_FACING, 0.95, 1.0, (0.0, 0.0, 1.0), R.ABS)
        sel = X.bits(m.gaussian_buffers.selection_buffer.download(), pos.shape[0])
        assert np.array_equal(sel, want) and hit == selected == int(want.sum()) and st.n_fitted == pos.shape[0]
        assert sel[:3000].mean() > 0.9 and sel[3000:].mean() < 0.15  # the floor, and little of the blob
        box = m.bounds(selected=True, trim_permille=100)  # (a twentieth of an isotropic blob faces up too: trimmed away)
        assert box.count == hit
        assert -1.05 < box.trim_min[2] <= box.trim_max[2] < -0.95  # the trimmed box of the selection is the floor's slab
        assert box.trim_min[0] < -3.5 and box.trim_max[0] > 3.5 and box.trim_min[1] < -3.5 and box.trim_max[1] > 3.5


# ---- 6. independence ----------------------------------------------------------------------------------------------------------------------
def test_pod_kind_transform_and_repetition_change_nothing():
    n = 3000
    g = common.small_scene(n, 71)
    tr = common.odd_transform()
    results = []
    for sh, cov in ((ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)):
        with MultiModelViewer(sh=sh, cov3d=cov) as v:
            m, pos = _scene_model(v, g)
            a = m.normals(5, indices=True)
            _check(a, pos, np.ones(n, bool), 5, what=(sh, cov))
            assert _same_words(a, m.normals(5, indices=True))  # the same bits on every call, the double mean included
            v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)  # model space: the transform changes nothing
            assert _same_words(a, m.normals(5, indices=True))
            first = m.select_normals(5, 0.0, 0.02)
            words = m.gaussian_buffers.selection_buffer.download()
            again = m.select_normals(5, 0.0, 0.02)
            assert again[:2] == first[:2] and np.array_equal(m.gaussian_buffers.selection_buffer.download(), words)
            results.append((a.index.tobytes(), a.normal.tobytes(), a.variation.tobytes(), a.mean))
    assert results[0] == results[1]  # the position plane is float32 in every pod kind


# ---- 7. workspace, and what a call writes ----------------------------------------------------------------------------------------------
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
        m.normals(16, indices=True)  # (the first call sizes the shared workspace: the indices of the largest k)
        held = viewer_mod.device_bytes()
        for flt in (0, 3, 7):
            m.normals(3, filter=flt)
            m.normals(16, filter=flt, indices=True, radius_hint=1e-4, toward=(0.0, 1.0, 0.0))
        assert viewer_mod.device_bytes() == held
        assert state(v) == start == state(twin)
        for a, b in zip(_frames(v, [SRC], poses=(6, 7)), _frames(twin, [SRC], poses=(6, 7))):
            assert np.array_equal(a, b)  # the next frames are the twin's: the call wrote nothing a frame reads
        held = viewer_mod.device_bytes()  # (the frames have sized their own buffers)
        m.select_normals(8, 0.0, 0.1, filter=3)
        m.normals(3)
        assert viewer_mod.device_bytes() == held  # (the model has a selection buffer already)
    assert viewer_mod.device_bytes() == before  # released with the viewer


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors():
    """every refusal of spec section 26 but GSX_ERR_OOM, which a test cannot provoke without exhausting the device"""
    n = 300
    with MultiModelViewer() as v, MultiModelViewer() as other:
        g, mask, sel, flags = _filter_model(v, n, 61)
        L, key = v._L, SRC.encode()
        sb = v.models[SRC].gaussian_buffers.selection_buffer
        sel_before = sb.download()
        normal, variation, index, stats = np.zeros(n * 3, F), np.zeros(n, F), np.zeros(n * 16, np.uint32), _lib.NormalsStats()
        hit, selected = C.c_uint64(), C.c_uint64()
        INV, NF, UNS = _lib.GSX_ERR_INVALID_ARG, _lib.GSX_ERR_NOT_FOUND, _lib.GSX_ERR_UNSUPPORTED
        nan, inf = float("nan"), float("inf")
        vec = lambda t: (C.c_float * 3)(*t)  # noqa: E731

        def normals(k_=key, flt=0, flags_=0, k=8, orient=0, hint=0.0, bits=0, rounds=0, reserved=0, toward=(0, 0, 0), reserved2=0, desc=True, st=stats, vv=v):
            d = _lib.NormalsDesc(flt, flags_, k, orient, hint, bits, rounds, reserved, vec(toward), reserved2)
            return L.gsx_model_normals(vv._h if vv else None, k_, C.byref(d) if desc else None, normal.ctypes.data, variation.ctypes.data,
                                       index.ctypes.data, C.byref(st) if st is not None else None)

        def select(k_=key, flt=0, flags_=0, op=0, mode=0, k=8, orient=0, hint=0.0, bits=0, rounds=0, lo=0.0, hi=1.0, reserved=0, d=(0, 0, 1),
                   toward=(0, 0, 0), reserved2=(0, 0), desc=True, vv=v):
            sd = _lib.NormalsSelectDesc(flt, flags_, op, mode, k, orient, hint, bits, rounds, lo, hi, reserved, vec(d), vec(toward), (C.c_uint32 * 2)(*reserved2))
            return L.gsx_model_select_normals(vv._h if vv else None, k_, C.byref(sd) if desc else None, C.byref(hit), C.byref(selected), None)

        bad_hints = (-1.0, nan, inf, 1e-23, 1.9e19)  # (1e-23: the square is 0; 1.9e19: the square is inf)
        cases = [
            (normals(vv=None), INV), (normals(k_=None), INV), (normals(desc=False), INV), (normals(st=None), INV), (normals(flt=8), INV),
            (normals(flags_=1), INV), (normals(k=2), INV), (normals(k=0), INV), (normals(k=17), INV), (normals(orient=2), INV),
            (normals(orient=1, toward=(nan, 0, 0)), INV), (normals(orient=1, toward=(0, inf, 0)), INV), (normals(bits=25), INV),
            (normals(rounds=65), INV), (normals(reserved=1), INV), (normals(reserved2=1), INV), (normals(k_=b"nope"), NF),
            (select(vv=None), INV), (select(k_=None), INV), (select(desc=False), INV), (select(flt=8), INV), (select(flags_=2), INV),
            (select(op=3), INV), (select(mode=2), INV), (select(k=2), INV), (select(k=17), INV), (select(orient=2), INV),
            (select(orient=1, toward=(0, 0, nan)), INV), (select(bits=25), INV), (select(rounds=65), INV), (select(lo=2.0, hi=1.0), INV),
            (select(lo=nan), INV), (select(hi=nan), INV), (select(mode=1, d=(0, 0, 0)), INV), (select(mode=1, d=(nan, 0, 1)), INV),
            (select(mode=1, d=(inf, 0, 0)), INV), (select(reserved=1), INV), (select(reserved2=(0, 1)), INV), (select(k_=b"nope"), NF),
        ] + [(normals(hint=r), INV) for r in bad_hints] + [(select(hint=r), INV) for r in bad_hints]
        for i, (got, want) in enumerate(cases):
            assert got == want, i
        assert b"gsx_model_select_normals" in L.gsx_last_error_string()
        assert np.array_equal(sb.download(), sel_before)  # a refused select leaves the selection
        # the ends of the legal ranges; a toward or a dir that the mode does not read may be anything; every array is optional
        assert normals(k=16, bits=24, rounds=64, hint=4e-23) == _lib.GSX_OK and normals(k=3, bits=1, rounds=1, hint=1.8e19) == _lib.GSX_OK
        assert normals(orient=0, toward=(nan, nan, nan)) == _lib.GSX_OK and select(mode=0, d=(0, 0, 0)) == _lib.GSX_OK
        assert select(lo=-inf, hi=inf) == _lib.GSX_OK and hit.value == stats.n_fitted > 0
        assert select(mode=1, flags_=1, lo=0.0, hi=inf) == _lib.GSX_OK and hit.value == stats.n_fitted
        sb.upload(sel_before)
        d = _lib.NormalsDesc(0, 0, 3, 0, 0.0, 0, 0, 0)
        assert L.gsx_model_normals(v._h, key, C.byref(d), None, None, None, C.byref(stats)) == _lib.GSX_OK and stats.count == n - 4 and stats.n_nonfinite == 4
        # an empty model, and no participants: GSX_OK with zeros; Set then clears the selection
        v.add_model("empty", 0)
        e = v.models["empty"]
        got = e.normals(3, indices=True)
        assert (got.index.shape, got.normal.shape, got.variation.size, got.count, got.n_nonfinite, got.n_fitted, got.mean, got.rounds) == ((0, 3), (0, 3), 0, 0, 0, 0, 0, 0)
        assert e.select_normals(3, 0.0, 1.0)[:2] == (0, 0)
        _load(v, g, "bare")
        none = v.models["bare"].normals(3, filter=X.SELECTED, indices=True)
        assert (none.count, none.n_nonfinite, none.n_fitted) == (0, 0, 0) and (none.index == R.NONE).all() and np.isinf(none.variation).all()
        assert v.models[SRC].select_normals(3, 0.9, 1.0)[:2] == (0, 0) and not sb.download().any()  # (no variation is above 1/3)
        # a sharded model; a viewer with a communicator
        _frames(v, [SRC], poses=(5,))
        _load(v, g[:50], "b")
        v.shard_set_limits("b", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        _load(other, g[:50], "a")
        other.comm_init_group(CommGroup(1), 0)
        for model, word in ((v.models["b"], "shard"), (other.models["a"], "communicator")):
            for call in (lambda: model.normals(3), lambda: model.select_normals(3, 0.0, 0.1)):
                with pytest.raises(GsxError) as err:
                    call()
                assert err.value.status == UNS and word in str(err.value)
