"""GPU: gsx_model_knn and gsx_model_select_knn (spec/RENDER_SPEC.md §20; csrc/kernels_knn.hip).  Rows, scores, counts, minimum,
maximum and every selection word are compared bit for bit; `mean`, `std` and `threshold` within the bounds below.  The yardsticks:
gsx_model_download_pod for the stored positions, the float32 definition tests/knn_ref.py: brute on them (tests/test_knn_cpu.py checks
its engineered expectations and ties the rules to csrc/knn_math.h), tests/extract_ref.py for the filter, gsx_model_upload_selection
for the frames.
Sizes: a workgroup of the passes in index order takes 1024 Gaussians in four rounds of 256, a wave 64 of them, a workgroup of the
query 256 entries; up to 1024 participants go straight to the exact fallback: one Gaussian, two, a wave edge (63, 64, 65), a round
edge (256, 257), the chunk and straight-to-fallback edge (1024, 1025), several chunks with a partial last one (5000).  k: the
template edges 4 | 5 and 8 | 9, both ends 1 and 16, and the default 3.
The bounds.  mean is a sum of m <= 5000 non-negative doubles divided by m: any order of the adds is within m * 2^-53 < 6e-13 of the
exact sum, relatively, so two orders differ by at most 1.2e-12; the bound is 2e-12.  std's terms (s - mean)^2 carry the mean's error
amplified by mean / std, which is below 10 on every set here, and a second sum: 1e-10.  The threshold is float32: it may differ by one
unit in the last place where the double expression lies at a rounding boundary; a score is never compared with a threshold that
differs — the expected hit set is built from the returned threshold."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import extract_ref as X
from tests import knn_ref as K
from tests import neighbors_ref as N
from tests.model_ops import H, W, frames as _frames, load as _load, pod as _pod
from tests.test_gpu_neighbors import FINISH_N, _finish_lattice, _selection_is
from wgpu_3dgs_viewer_app_amd import _lib, query
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as EF
from wgpu_3dgs_viewer_app_amd.viewer import CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
SRC = "src"
F = np.float32
SIZES = [1, 2, 63, 64, 65, 256, 257, 1024, 1025, 5000]
KS = [1, 3, 4, 5, 8, 9, 16]
HIGHLIGHT = (1.0, 0.0, 1.0, 0.3)
MEAN_RTOL, STD_RTOL = 2e-12, 1e-10


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _with_pos(pos):
    g = common.small_scene(pos.shape[0], 5, 0)
    g["pos"] = pos
    return g


def _scene_model(v, g, key=SRC):
    _load(v, g, key)
    return v.models[key], _pod(v, key)[0]


def _points_model(v, pos, key=SRC):
    return _scene_model(v, _with_pos(np.ascontiguousarray(pos, F)), key)


def _check_stats(got, scores, part, nonfinite=0, what=""):
    want = K.stats(np.where(part, scores, K.INF))
    assert (got.count, got.n_nonfinite, got.n_scored) == (int(part.sum()), nonfinite, want["n_scored"]), what
    assert _same(got.score_min, want["score_min"]) and _same(got.score_max, want["score_max"]), what
    assert got.mean == pytest.approx(want["mean"], rel=MEAN_RTOL, abs=0) and got.std == pytest.approx(want["std"], rel=STD_RTOL, abs=0), what
    assert got.threshold == 0  # (only a select in mode OUTLIERS has one)
    return want


def _check(got, full, part, k, score, nonfinite=0, what=""):
    """got: a ModelKnn with rows; full: knn_ref.brute with at least k columns"""
    rows = full[:, :k]
    assert _same(got.d2, rows), what
    scores = K.score(rows, score)
    assert _same(got.score, scores), what
    return _check_stats(got, scores, part, nonfinite, what)


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_rows_scores_and_statistics_at_the_edges_of_the_passes(n):
    g = common.small_scene(n, 300 + n, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        every = np.ones(n, bool)
        full = K.brute(pos, every, 16)
        for k in (KS if n == 5000 else (1, 3, 16)):
            for score in (K.SCORE_KTH, K.SCORE_MEAN):
                got = m.knn(k, score, rows=True)
                st = _check(got, full, every, k, score, what=(n, k, score))
                assert got.grid_bits == N.auto_bits(n) and got.rounds + got.n_brute >= 1
                if n <= 1024:
                    assert (got.rounds, got.n_brute) == (0, n)  # straight to the exact fallback
                else:
                    assert got.rounds >= 1
                if n <= k:  # fewer than k others: every row holds a +inf
                    assert np.isinf(got.d2[:, n - 1:]).all() and np.isinf(got.score).all()
                    assert (st["n_scored"], got.mean, got.std, got.score_min, got.score_max) == (0, 0, 0, 0, 0)
            without = m.knn(k)  # the rows are optional, and the score does not depend on them
            assert without.d2 is None and _same(without.score, K.score(full[:, :k], K.SCORE_MEAN))


# ---- 2. the knobs change nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2500, 5000])
def test_the_knobs_change_nothing(n):
    g = common.small_scene(n, 330 + n, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        every = np.ones(n, bool)
        full = K.brute(pos, every, 9)
        d = np.sqrt(float(np.median(full[:, 0])))  # the median nearest distance
        base = m.knn(9, rows=True)
        _check(base, full, every, 9, K.SCORE_MEAN, what="default")
        assert base.rounds >= 1
        paths = set()
        for what, kw in (("tiny, one round", dict(radius_hint=d * 1e-6, max_rounds=1)), ("tiny", dict(radius_hint=d * 1e-6)),
                         ("tiny, two rounds", dict(radius_hint=d * 1e-6, max_rounds=2)), ("huge", dict(radius_hint=d * 1e6)),
                         ("chosen", dict(radius_hint=d * 2)), ("two buckets", dict(grid_bits=1)), ("eight", dict(grid_bits=3)),
                         ("4096", dict(grid_bits=12)), ("all", dict(radius_hint=d * 3, grid_bits=3, max_rounds=64))):
            got = m.knn(9, rows=True, **kw)
            assert got.d2.tobytes() == base.d2.tobytes() and got.score.tobytes() == base.score.tobytes(), what
            assert (got.count, got.n_scored, got.mean, got.std) == (base.count, base.n_scored, base.mean, base.std), what
            assert _same(got.score_min, base.score_min) and _same(got.score_max, base.score_max), what
            assert got.grid_bits == kw.get("grid_bits", 0) or got.grid_bits == N.auto_bits(n)
            paths.add((got.rounds, got.n_brute))
            if what == "tiny, one round":  # one round at the floor proves nobody: everything goes to the exact fallback
                assert (got.rounds, got.n_brute) == (1, got.count) and got.first_radius > F(kw["radius_hint"])
            if what == "tiny":
                assert got.rounds >= 2
            if what == "huge":
                assert (got.rounds, got.n_brute) == (1, 0) and got.first_radius == F(kw["radius_hint"])  # one cell, one round
        assert len(paths) >= 3


# ---- 3. engineered sets -----------------------------------------------------------------------------------------------------------------
def test_lattice_whose_kth_distance_ties():
    lat = N.lattice(0.25, 11)  # 1331 points: past the straight-to-fallback edge, so the grid rounds answer
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, lat)
        assert pos.tobytes() == lat.tobytes()
        every = np.ones(lat.shape[0], bool)
        full = K.brute(pos, every, 7)
        interior = (np.abs(np.rint(lat / F(0.25))) < 5).all(axis=1)
        for k in (6, 7):
            got = m.knn(k, K.SCORE_KTH, rows=True)
            _check(got, full, every, k, K.SCORE_KTH, what=k)
            assert (got.d2[interior, :6] == F(0.0625)).all()  # the six nearest at exactly 0.25
        assert (got.d2[interior, 6] == F(0.125)).all() and (got.score[interior] == np.sqrt(F(0.125))).all()  # the next at 0.25 sqrt 2
        for bits in (1, 3):
            assert m.knn(7, K.SCORE_KTH, grid_bits=bits, rows=True).d2.tobytes() == got.d2.tobytes()


def test_coincident_points():
    same = np.tile(F([0.3, -1.7, 2.9]), (1300, 1))
    with MultiModelViewer(sh=ShKind.Remove) as v:
        for n, k in ((300, 16), (1300, 5), (1300, 16)):  # through the exact fallback, and through a grid round that stops at k zeros
            m, pos = _points_model(v, same[:n], f"same{n}k{k}")
            got = m.knn(k, rows=True)
            assert not got.d2.any() and not got.score.any() and got.d2.shape == (n, k)
            assert (got.n_scored, got.mean, got.std, got.score_min, got.score_max) == (n, 0, 0, 0, 0)
        m, pos = _points_model(v, same[:10], "few")  # fewer than k others: nine zeros and seven +inf
        got = m.knn(16, rows=True)
        assert not got.d2[:, :9].any() and np.isinf(got.d2[:, 9:]).all() and np.isinf(got.score).all()
        assert (got.count, got.n_scored, got.n_brute, got.mean, got.std) == (10, 0, 10, 0, 0)
        assert m.knn(9, K.SCORE_KTH).n_scored == 10 and m.knn(10, K.SCORE_KTH).n_scored == 0


def test_two_scales_and_isolated_points():
    rng = np.random.default_rng(9)
    dense = rng.random((1500, 3)) * 0.01                    # spacing about 1e-3
    other = rng.random((1500, 3)) * 0.01 + [1.0, 0, 0]      # a second blob 1000 spacings away
    lone = rng.random((20, 3)) * 40.0 + 5.0                 # isolated points: their neighbours are far beyond the first radii
    pos = np.concatenate([dense, other, lone]).astype(F)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, stored = _points_model(v, pos)
        every = np.ones(pos.shape[0], bool)
        full = K.brute(stored, every, 8)
        got = m.knn(8, rows=True)
        _check(got, full, every, 8, K.SCORE_MEAN, what="two scales")
        assert got.rounds >= 2 or got.n_brute >= 20  # the later paths ran: a second grid, or the exact fallback
        # the isolated points are the statistical outliers
        hit, selected, st = m.select_knn(8, std_ratio=3.0)
        words = m.gaussian_buffers.selection_buffer.download()
        want = K.hit(got.score, every, K.SELECT_OUTLIERS, st=dict(n_scored=st.n_scored, mean=st.mean, std=st.std), std_ratio=3.0)
        assert np.array_equal(words, X.words(want)) and want[-20:].all() and hit == selected == int(want.sum()) < 100


def test_far_huge_and_non_finite_positions():
    planted, _ = N.special_scene(3000)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, planted)
        assert pos.tobytes() == planted.tobytes()  # NaN, inf and 3e38 are stored as they are
        part = N.participates(pos)
        full = K.brute(pos, part, 4)
        got = m.knn(4, rows=True)
        _check(got, full, part, 4, K.SCORE_MEAN, nonfinite=3, what="special")
        assert not np.isnan(got.d2).any() and not np.isnan(got.score).any()
        assert got.d2[10, 0] == 0 and got.d2[11, 0] == 0         # the coincident pair at 1e6
        assert np.isinf(got.d2[15]).all() and np.isinf(got.d2[16]).all()  # every difference overflows: +inf, and an infinite score
        assert np.isinf(got.d2[17:20]).all() and np.isinf(got.score[14:20]).all()  # NaN / inf positions do not participate
        assert got.n_brute >= 3 and got.n_scored == part.sum() - int(np.isinf(K.score(full, K.SCORE_MEAN)[part]).sum())
        assert not got.d2[20:31, :4].any()                       # eleven coincident points
        # the non-finite ones are nobody's neighbour: without them, the others' rows are the same
        _load(v, _with_pos(pos[part]), "finite")
        assert _same(v.models["finite"].knn(4, rows=True).d2, got.d2[part])
        for kw in (dict(grid_bits=1), dict(radius_hint=1e-3), dict(radius_hint=1.8e19), dict(max_rounds=1)):
            assert m.knn(4, rows=True, **kw).d2.tobytes() == got.d2.tobytes(), kw


# ---- 4. filter --------------------------------------------------------------------------------------------------------------------------
def _filter_model(v, n, seed=7, key=SRC):
    """tests/test_gpu_neighbors.py's recipe: a model with a mask, a selection (garbage in both tails) and stored edits (some ENABLED +
    HIDDEN), NaN and infinite positions; returns the host arrays"""
    g = common.small_scene(n, seed, 0)
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


@pytest.mark.parametrize("n", [65, 2500])
def test_every_filter_combination(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 400 + n)
        _load(v, g, "bare")  # the same Gaussians without mask, selection and edit records
        pos = _pod(v)[0]
        finite = N.participates(pos)
        for key, planes in ((SRC, (mask, sel, flags)), ("bare", (None, None, None))):
            for flt in range(8):
                passes = _passes(n, flt, *planes)
                part = passes & finite
                got = v.models[key].knn(3, rows=True, filter=flt)
                _check(got, K.brute(pos, part, 3), part, 3, K.SCORE_MEAN, nonfinite=int((passes & ~finite).sum()), what=(key, flt))
                assert np.isinf(got.d2[~part]).all() and np.isinf(got.score[~part]).all()
        none = v.models["bare"].knn(3, filter=X.SELECTED)  # SELECTED of a model without a selection: none
        assert (none.count, none.n_scored, none.rounds, none.n_brute) == (0, 0, 0, 0) and np.isinf(none.score).all()


# ---- 5. select --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1500])
def test_select_against_the_restatement(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 500 + n)
        m = v.models[SRC]
        sb = m.gaussian_buffers.selection_buffer
        pos = _pod(v)[0]
        finite = N.participates(pos)
        for prior in ("random", None):
            for flt in (0, X.SELECTED, X.MASKED | X.SKIP_HIDDEN, 7):
                part = _passes(n, flt, mask, sel if prior else None, flags) & finite  # SELECTED reads the selection as it was
                full = K.brute(pos, part, 5)
                for k, score in ((3, K.SCORE_MEAN), (5, K.SCORE_KTH)):
                    scores = np.where(part, K.score(full[:, :k], score), K.INF)
                    st = K.stats(scores)
                    lo, hi = (np.quantile(scores[np.isfinite(scores)], [0.25, 0.75]) if st["n_scored"] else (0.0, 1.0))
                    for mode, kw in ((K.SELECT_RANGE, dict(lo=float(F(lo)), hi=float(F(hi)))), (K.SELECT_RANGE, dict(lo=float(F(hi)), hi=np.inf)),
                                     (K.SELECT_OUTLIERS, dict(std_ratio=1.0)), (K.SELECT_OUTLIERS, dict(std_ratio=-0.5))):
                        for op in (N.SET, N.ADD, N.REMOVE):
                            sb.upload(X.words(sel, True) if prior else None)  # (garbage in the tail bits of the prior selection)
                            old = sel if prior else np.zeros(n, bool)
                            got_hit, got_selected, gs = m.select_knn(k, score, op=op, filter=flt, **kw)
                            what = (prior, flt, k, mode, kw, op)
                            assert (gs.count, gs.n_scored) == (int(part.sum()), st["n_scored"]), what
                            assert gs.mean == pytest.approx(st["mean"], rel=MEAN_RTOL, abs=0) and gs.std == pytest.approx(st["std"], rel=STD_RTOL, abs=0), what
                            if mode == K.SELECT_OUTLIERS:
                                t = K.threshold(st["mean"], st["std"], kw["std_ratio"])
                                assert abs(int(_bits(gs.threshold)) - int(_bits(t))) <= 1, what
                                hit = part & (scores > gs.threshold) if st["n_scored"] else np.zeros(n, bool)
                            else:
                                assert gs.threshold == 0
                                hit = K.hit(scores, part, mode, **kw)
                            want = hit if op == N.SET else (old | hit if op == N.ADD else old & ~hit)
                            assert (got_hit, got_selected) == (int(hit.sum()), int(want.sum())), what
                            assert np.array_equal(sb.download(), X.words(want)), what  # tail bits zero
        # hi = +inf also takes the Gaussians with fewer than k others; the out pointers are optional; the knobs change no word
        assert m.select_knn(16, lo=0.0, hi=np.inf)[0] == int(finite.sum())
        words = sb.download()
        desc = _lib.KnnSelectDesc(0, 0, N.SET, K.SELECT_RANGE, 16, K.SCORE_MEAN, 1e-4, 1, 1, 0.0, np.inf, 0.0)
        assert v._L.gsx_model_select_knn(v._h, SRC.encode(), C.byref(desc), None, None, None) == _lib.GSX_OK
        assert np.array_equal(sb.download(), words)


def test_select_sums_more_partials_than_the_finish_has_lanes():
    n = FINISH_N
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, _ = _points_model(v, _finish_lattice())
        got = m.knn(1, K.SCORE_KTH)
        # (sums of ones are exact in double: the mean is exactly 1, the deviation exactly 0)
        assert (got.n_scored, got.score_min, got.score_max, got.mean, got.std) == (n, 1.0, 1.0, 1.0, 0.0)
        assert m.select_knn(1, K.SCORE_KTH, lo=1.0, hi=1.0, op=N.SET)[:2] == (n, n) and _selection_is(m.gaussian_buffers.selection_buffer, True)


def test_outlier_removal_then_extract_and_frames():
    n = 2500
    g = common.small_scene(n, 37)
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _load(vv, g)
            vv.update_selection_edit_with_pod(query.GaussianEditPod(EF.ENABLED, alpha=0.6))
            vv.update_selection_highlight(HIGHLIGHT)
        m = v.models[SRC]
        pos = _pod(v)[0]
        plain = _frames(v, [SRC], poses=(4,))[0]
        assert np.array_equal(plain, _frames(twin, [SRC], poses=(4,))[0])
        scores = K.score(K.brute(pos, np.ones(n, bool), 3), K.SCORE_MEAN)
        # a model without a selection gets one
        hit, selected, st = m.select_knn(3, std_ratio=1.5)
        floaters = scores > st.threshold
        assert 0 < floaters.sum() < n // 4 and hit == selected == int(floaters.sum())
        assert abs(int(_bits(st.threshold)) - int(_bits(K.threshold(*[K.stats(scores)[w] for w in ("mean", "std")], 1.5)))) <= 1
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
        # stats.mean of the k-th distance is a radius for the neighbour counts and the clusters
        r = m.knn(4, K.SCORE_KTH).mean
        assert 1 <= np.median(m.neighbors(r).counts) <= 16 and m.clusters(r).n_clusters >= 1


def _lane_sequence(g, lanes, on_device, hi):
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
            m.select_knn(3, lo=0.0, hi=float(hi))  # behind the frames in flight on the lanes
        else:
            scores = K.score(K.brute(_pod(v)[0], np.ones(g.shape[0], bool), 3), K.SCORE_MEAN)
            m.gaussian_buffers.selection_buffer.upload(X.words(scores <= hi))
        for pose in (5, 6, 7, 8):
            out += _frames(v, [SRC], poses=(pose,))
    return out


def test_lanes():
    g = common.small_scene(2500, 38)
    scores = K.score(K.brute(g["pos"], np.ones(2500, bool), 3), K.SCORE_MEAN)
    hi = F(np.median(scores))
    two, one, host = _lane_sequence(g, 2, True, hi), _lane_sequence(g, 1, True, hi), _lane_sequence(g, 2, False, hi)
    assert len(two) == 8 and two[0][..., :3].max() > 0
    for k, (a, b, c) in enumerate(zip(two, one, host)):
        assert np.array_equal(a, b) and np.array_equal(a, c), k


# ---- 6. independence ----------------------------------------------------------------------------------------------------------------------
def test_pod_kind_transform_and_repetition_change_nothing():
    n = 3000
    g = common.small_scene(n, 71)
    tr = common.odd_transform()
    results = []
    for sh, cov in ((ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)):
        with MultiModelViewer(sh=sh, cov3d=cov) as v:
            m, pos = _scene_model(v, g)
            a = m.knn(5, rows=True)
            _check(a, K.brute(pos, np.ones(n, bool), 5), np.ones(n, bool), 5, K.SCORE_MEAN, what=(sh, cov))
            b = m.knn(5, rows=True)
            same = lambda p, q: (p.d2.tobytes(), p.score.tobytes(), p.count, p.n_scored, p.mean, p.std, float(p.score_min), float(p.score_max)) == \
                (q.d2.tobytes(), q.score.tobytes(), q.count, q.n_scored, q.mean, q.std, float(q.score_min), float(q.score_max))  # noqa: E731
            assert same(a, b)  # the same bits on every call, the double statistics included
            v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)  # model space: the transform changes nothing
            assert same(a, m.knn(5, rows=True))
            first = m.select_knn(5, std_ratio=1.0)
            words = m.gaussian_buffers.selection_buffer.download()
            again = m.select_knn(5, std_ratio=1.0)
            assert again[:2] == first[:2] and _same(again[2].threshold, first[2].threshold) and np.array_equal(m.gaussian_buffers.selection_buffer.download(), words)
            results.append((a.d2.tobytes(), a.mean, a.std))
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
        m.knn(16, rows=True)  # (the first call sizes the shared workspace: the rows of the largest k)
        held = viewer_mod.device_bytes()
        for flt in (0, 3, 7):
            m.knn(3, filter=flt)
            m.knn(16, K.SCORE_KTH, filter=flt, rows=True, radius_hint=1e-4)
        assert viewer_mod.device_bytes() == held
        assert state(v) == start == state(twin)
        for a, b in zip(_frames(v, [SRC], poses=(6, 7)), _frames(twin, [SRC], poses=(6, 7))):
            assert np.array_equal(a, b)
        held = viewer_mod.device_bytes()  # (the frames have sized their own buffers)
        m.select_knn(3, std_ratio=2.0, filter=3)
        m.knn(3)
        assert viewer_mod.device_bytes() == held  # (the model has a selection buffer already)
    assert viewer_mod.device_bytes() == before  # released with the viewer


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors():
    """every refusal of spec section 20 but GSX_ERR_OOM, which a test cannot provoke without exhausting the device"""
    n = 300
    with MultiModelViewer() as v, MultiModelViewer() as other:
        g, mask, sel, flags = _filter_model(v, n, 61)
        L, key = v._L, SRC.encode()
        sb = v.models[SRC].gaussian_buffers.selection_buffer
        sel_before = sb.download()
        rows, score, stats = np.zeros(n * 16, F), np.zeros(n, F), _lib.KnnStats()
        hit, selected = C.c_uint64(), C.c_uint64()
        INV, NF, UNS = _lib.GSX_ERR_INVALID_ARG, _lib.GSX_ERR_NOT_FOUND, _lib.GSX_ERR_UNSUPPORTED
        nan, inf = float("nan"), float("inf")

        def knn(k_=key, flt=0, flags_=0, k=3, sc=1, hint=0.0, bits=0, rounds=0, reserved=0, desc=True, st=stats, vv=v):
            d = _lib.KnnDesc(flt, flags_, k, sc, hint, bits, rounds, reserved)
            return L.gsx_model_knn(vv._h if vv else None, k_, C.byref(d) if desc else None, rows.ctypes.data, score.ctypes.data,
                                   C.byref(st) if st is not None else None)

        def select(k_=key, flt=0, flags_=0, op=0, mode=0, k=3, sc=1, hint=0.0, bits=0, rounds=0, lo=0.0, hi=1.0, ratio=0.0, desc=True, vv=v):
            d = _lib.KnnSelectDesc(flt, flags_, op, mode, k, sc, hint, bits, rounds, lo, hi, ratio)
            return L.gsx_model_select_knn(vv._h if vv else None, k_, C.byref(d) if desc else None, C.byref(hit), C.byref(selected), None)

        bad_hints = (-1.0, nan, inf, 1e-23, 1.9e19)  # (1e-23: the square is 0; 1.9e19: the square is inf)
        cases = [
            (knn(vv=None), INV), (knn(k_=None), INV), (knn(desc=False), INV), (knn(st=None), INV), (knn(flt=8), INV), (knn(flags_=1), INV),
            (knn(k=0), INV), (knn(k=17), INV), (knn(sc=2), INV), (knn(bits=25), INV), (knn(rounds=65), INV), (knn(reserved=1), INV),
            (knn(k_=b"nope"), NF),
            (select(vv=None), INV), (select(k_=None), INV), (select(desc=False), INV), (select(flt=8), INV), (select(flags_=1), INV),
            (select(op=3), INV), (select(mode=2), INV), (select(k=0), INV), (select(k=17), INV), (select(sc=2), INV), (select(bits=25), INV),
            (select(rounds=65), INV), (select(lo=2.0, hi=1.0), INV), (select(lo=nan), INV), (select(hi=nan), INV), (select(ratio=1.0), INV),
            (select(mode=1, lo=0.0, hi=0.0, ratio=nan), INV), (select(mode=1, lo=0.0, hi=0.0, ratio=inf), INV),
            (select(mode=1, lo=0.0, hi=1.0, ratio=1.0), INV), (select(k_=b"nope"), NF),
        ] + [(knn(hint=r), INV) for r in bad_hints] + [(select(hint=r), INV) for r in bad_hints]
        for i, (got, want) in enumerate(cases):
            assert got == want, i
        assert b"gsx_model_select_knn" in L.gsx_last_error_string()
        assert np.array_equal(sb.download(), sel_before)  # a refused select leaves the selection
        # the ends of the legal ranges; the rows and the scores are optional
        assert knn(k=16, bits=24, rounds=64, hint=4e-23) == _lib.GSX_OK and knn(k=1, sc=0, bits=1, rounds=1, hint=1.8e19) == _lib.GSX_OK
        assert select(lo=-inf, hi=inf) == _lib.GSX_OK and hit.value == n - 4
        assert select(mode=1, lo=0.0, hi=0.0, ratio=-3.0) == _lib.GSX_OK
        sb.upload(sel_before)
        d = _lib.KnnDesc(0, 0, 3, 1, 0.0, 0, 0, 0)
        assert L.gsx_model_knn(v._h, key, C.byref(d), None, None, C.byref(stats)) == _lib.GSX_OK and stats.count == n - 4 and stats.n_nonfinite == 4
        # an empty model, and no participants: GSX_OK with zeros; Set then clears the selection
        v.add_model("empty", 0)
        e = v.models["empty"]
        got = e.knn(3, rows=True)
        assert (got.d2.shape, got.score.size, got.count, got.n_nonfinite, got.n_scored, got.mean, got.std, got.rounds) == ((0, 3), 0, 0, 0, 0, 0, 0, 0)
        assert e.select_knn(3, std_ratio=1.0)[:2] == (0, 0)
        _load(v, g, "bare")
        none = v.models["bare"].knn(3, filter=X.SELECTED, rows=True)
        assert (none.count, none.n_nonfinite, none.n_scored) == (0, 0, 0) and np.isinf(none.d2).all() and np.isinf(none.score).all()
        assert v.models[SRC].select_knn(3, lo=1e9, hi=1e10)[:2] == (0, 0) and not sb.download().any()
        # a sharded model; a viewer with a communicator
        _frames(v, [SRC], poses=(5,))
        _load(v, g[:50], "b")
        v.shard_set_limits("b", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        _load(other, g[:50], "a")
        other.comm_init_group(CommGroup(1), 0)
        for model, word in ((v.models["b"], "shard"), (other.models["a"], "communicator")):
            for call in (lambda: model.knn(3), lambda: model.select_knn(3, std_ratio=1.0)):
                with pytest.raises(GsxError) as err:
                    call()
                assert err.value.status == UNS and word in str(err.value)
