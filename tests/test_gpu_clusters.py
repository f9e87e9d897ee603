"""GPU: gsx_model_clusters and gsx_model_select_clusters (spec/RENDER_SPEC.md §19; csrc/kernels_clusters.hip).  Equality is exact
everywhere.  The yardsticks: gsx_model_download_pod for the stored positions, tests/clusters_ref.py on them (the float32 pairs of the
definition, a sequential union-find; tests/test_clusters_cpu.py proves its expectations on the engineered sets and ties
csrc/clusters_math.h to it), tests/extract_ref.py for the filter, gsx_model_upload_selection for the frames.
Sizes: a workgroup of the passes in index order takes 1024 Gaussians in four rounds of 256 (the label, the stats, the select) or 256
(init, hook), a wave 64 of them (two words of a bit plane): one Gaussian, two, a word and wave edge (63, 64, 65), a round edge (256, 257),
a chunk edge (1024, 1025), several chunks with a partial last one (5000).  No kernel caps its grid."""
import ctypes as C

import numpy as np
import pytest

from tests import clusters_ref as K
from tests import common
from tests import extract_ref as X
from tests import neighbors_ref as N
from tests.model_ops import H, W, frames as _frames, load as _load, pod as _pod
from tests.test_gpu_neighbors import FINISH_N, _filter_model, _finish_lattice, _passes, _points_model, _radius, _scene_model, _selection_is
from wgpu_3dgs_viewer_app_amd import _lib, camera, query
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as EF
from wgpu_3dgs_viewer_app_amd.viewer import (CommGroup, Cov3dKind, GaussianDisplayMode, GaussianShDegree, GsxError, MultiModelViewer,
                                             ShKind)

pytestmark = pytest.mark.gpu
SRC = "src"
F = np.float32
SIZES = [1, 2, 63, 64, 65, 256, 257, 1024, 1025, 5000]
HIGHLIGHT = (1.0, 0.0, 1.0, 0.3)
RADIUS_K = 3  # the k of _radius: on small_scene it leaves one large cluster, dozens of small ones and dozens of singletons at every size
MODES = ((K.BY_SIZE, 1, 1), (K.BY_SIZE, 2, 40), (K.LARGEST, 0, 0), (K.SEEDED, 0, 0))
OPS = (K.SET, K.ADD, K.REMOVE)


def _check(got, want: K.Clusters, what=""):
    assert np.array_equal(got.labels, want.labels), what
    assert np.array_equal(got.sizes, want.sizes), what
    assert (got.count, got.n_clusters, got.largest_size, got.largest_label) == (want.count, want.n_clusters, want.largest_size, want.largest_label), what


def _same(a, b):
    return (a.labels.tobytes(), a.sizes.tobytes(), a.count, a.n_nonfinite, a.n_clusters, a.largest_size, a.largest_label) == \
           (b.labels.tobytes(), b.sizes.tobytes(), b.count, b.n_nonfinite, b.n_clusters, b.largest_size, b.largest_label)


def _bits(words, n):
    return ((words[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_clusters_at_the_edges_of_the_passes(n):
    g = common.small_scene(n, 700 + n, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        r = _radius(pos, RADIUS_K)
        want = K.clusters(pos, np.ones(n, bool), r)
        if n >= 256:  # (from the restatement, not the device) the input has every kind of cluster
            roots = want.sizes[want.labels == np.arange(n)]
            assert (roots >= 2).sum() >= 2 and (roots == 1).sum() >= 1, n
        got = m.clusters(r)
        _check(got, want, n)
        assert (got.n_nonfinite, got.grid_bits) == (0, N.auto_bits(n))


# ---- 2. engineered sets -----------------------------------------------------------------------------------------------------------------
def test_chain_at_exactly_the_radius():
    pos, k = K.chain()
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, stored = _points_model(v, pos)
        assert stored.tobytes() == pos.tobytes()
        one = m.clusters(0.5)  # d2 == r2 exactly between consecutive points
        assert (one.n_clusters, one.largest_size, one.largest_label, one.count) == (1, 4096, 0, 4096)
        assert not one.labels.any() and (one.sizes == 4096).all()
        apart = m.clusters(float(np.nextafter(F(0.5), F(0))))
        assert apart.n_clusters == 4096 and np.array_equal(apart.labels, np.arange(4096)) and (apart.sizes == 1).all()
        assert (apart.largest_size, apart.largest_label) == (1, 0)
        pos2, k2 = K.chain(split=True)
        m2, _ = _points_model(v, pos2, "split")
        two = m2.clusters(0.5)
        low, high = np.nonzero(k2 < 2048)[0], np.nonzero(k2 >= 2048)[0]
        assert two.n_clusters == 2 and (two.sizes == 2048).all() and (two.largest_size, two.largest_label) == (2048, 0)
        assert (two.labels[low] == low.min()).all() and (two.labels[high] == high.min()).all()


def test_chain_past_the_cell_clamp():
    """70 000 points half a unit apart: the last 2 400 lie in the clamped cell 32767 of x.  One cluster (analytic: no brute force)"""
    pos, _ = K.chain(70000, 12)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, stored = _points_model(v, pos)
        assert stored.tobytes() == pos.tobytes()
        got = m.clusters(0.5)
        assert (got.count, got.n_clusters, got.largest_size, got.largest_label) == (70000, 1, 70000, 0)
        assert not got.labels.any() and (got.sizes == 70000).all()
        assert m.select_clusters(0.5, K.LARGEST) == (70000, 70000)


def test_lattice_at_exactly_the_radius():
    lat = N.lattice()
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, lat)
        assert pos.tobytes() == lat.tobytes()
        for bits in (0, 1, 3, 12):  # the six neighbours' cells meet in shared buckets
            got = m.clusters(0.25, grid_bits=bits)
            assert (got.n_clusters, got.largest_size, got.largest_label) == (1, 729, 0) and not got.labels.any(), bits
        below = m.clusters(float(np.nextafter(F(0.25), F(0))))
        assert below.n_clusters == 729 == below.count and np.array_equal(below.labels, np.arange(729)) and (below.sizes == 1).all()


def test_coincident_points():
    same = np.tile(F([0.3, -1.7, 2.9]), (300, 1))
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, same)
        got = m.clusters(0.5)
        assert (got.count, got.n_clusters, got.largest_size, got.largest_label) == (300, 1, 300, 0)
        assert not got.labels.any() and (got.sizes == 300).all()
        _check(got, K.clusters(pos, np.ones(300, bool), 0.5))


def test_far_huge_and_non_finite_positions():
    planted, r = N.special_scene(3000)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _points_model(v, planted)
        assert pos.tobytes() == planted.tobytes()  # NaN, inf and 3e38 are stored as they are
        part = N.participates(pos)
        got = m.clusters(r)
        _check(got, K.clusters(pos, part, r), "special")
        assert (got.n_nonfinite, got.count) == (3, 3000 - 3)
        assert got.labels[10] == got.labels[11] == 10 and got.sizes[10] == got.sizes[11] == 2  # the coincident pair at 1e6
        assert np.array_equal(got.labels[12:17], np.arange(12, 17)) and (got.sizes[12:17] == 1).all()
        assert (got.labels[17:20] == K.NONE).all() and not got.sizes[17:20].any()
        for bits in (1, 5):
            assert _same(m.clusters(r, grid_bits=bits), got), bits


def test_a_bridge_and_a_tie_for_the_largest():
    """the filter decides connectivity, not only membership: without the point between them the two blobs are two clusters, of one
    size — the largest is then the one with the smaller label"""
    pos, at = K.bridge()
    every = np.ones(55, bool)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, stored = _points_model(v, pos)
        assert stored.tobytes() == pos.tobytes()
        sb = m.gaussian_buffers.selection_buffer
        m.gaussian_buffers.mask_buffer.upload(X.words(np.arange(55) != at, True))
        joined = m.clusters(0.25)
        _check(joined, K.clusters(pos, every, 0.25))
        assert (joined.n_clusters, joined.largest_size) == (1, 55)
        want = K.clusters(pos, np.arange(55) != at, 0.25)
        split = m.clusters(0.25, filter=X.MASKED)
        _check(split, want)
        assert (split.n_clusters, split.largest_size, split.count) == (2, 27, 54) and split.labels[at] == K.NONE
        assert split.largest_label == split.labels[split.labels != K.NONE].min()
        assert m.select_clusters(0.25, K.LARGEST, filter=X.MASKED) == (27, 27)
        assert np.array_equal(sb.download(), X.words(want.labels == want.largest_label))
        # a seed on the bridge itself does not pass the filter: no seed
        sb.upload(X.words(np.arange(55) == at))
        assert m.select_clusters(0.25, K.SEEDED, filter=X.MASKED) == (0, 0)
        sb.upload(X.words(np.arange(55) == at))
        assert m.select_clusters(0.25, K.SEEDED) == (55, 55)


def test_table_size_changes_nothing():
    g = common.small_scene(2000, 41, 0)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, pos = _scene_model(v, g)
        r = _radius(pos, RADIUS_K)
        want = K.clusters(pos, np.ones(2000, bool), r)
        auto = m.clusters(r)
        _check(auto, want)
        for bits in (1, 8, 24):  # two buckets: every visited cell aliases with others
            got = m.clusters(r, grid_bits=bits)
            assert _same(got, auto) and got.grid_bits == bits, bits
        assert auto.grid_bits == N.auto_bits(2000)


# ---- 3. filter --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1025, 2500])
def test_every_filter_combination(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 400 + n)
        _load(v, g, "bare")  # the same Gaussians without mask, selection and edit records
        pos = _pod(v)[0]
        r = _radius(pos, RADIUS_K)
        finite = N.participates(pos)
        for key, planes in ((SRC, (mask, sel, flags)), ("bare", (None, None, None))):
            for flt in range(8):
                passes = _passes(n, flt, *planes)
                part = passes & finite
                got = v.models[key].clusters(r, filter=flt)
                _check(got, K.clusters(pos, part, r), (key, flt))
                assert got.n_nonfinite == int((passes & ~finite).sum()), (key, flt)
        none = v.models["bare"].clusters(r, filter=X.SELECTED)  # SELECTED of a model without a selection: none
        assert (none.count, none.n_clusters, none.largest_size, none.largest_label) == (0, 0, 0, K.NONE)
        assert (none.labels == K.NONE).all() and not none.sizes.any()


# ---- 4. select --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1025, 2500])
def test_select_against_the_restatement(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 500 + n)
        m = v.models[SRC]
        sb = m.gaussian_buffers.selection_buffer
        pos = _pod(v)[0]
        r = _radius(pos, RADIUS_K)
        finite = N.participates(pos)
        for prior in ("random", None):
            old = sel if prior else np.zeros(n, bool)
            for flt in (0, X.SELECTED, X.MASKED | X.SKIP_HIDDEN, 7):
                part = _passes(n, flt, mask, sel if prior else None, flags) & finite  # SELECTED reads the selection as it was
                want = K.clusters(pos, part, r)
                sb.upload(X.words(sel, True) if prior else None)
                stats = m.clusters(r, filter=flt)
                _check(stats, want, (prior, flt))
                for mode, lo, hi in MODES:
                    hit = K.hits(want, mode, lo, hi, seeds=sel if prior else None)  # (seeds that fail the filter are in `sel`)
                    # the identity with gsx_model_clusters' own answer
                    if mode == K.BY_SIZE:
                        roots = stats.labels == np.arange(n)
                        implied = int(stats.sizes[roots & (stats.sizes >= lo) & (stats.sizes <= hi)].sum())
                    elif mode == K.LARGEST:
                        implied = stats.largest_size
                    else:
                        implied = int(hit.sum())
                    for op in OPS:
                        sb.upload(X.words(sel, True) if prior else None)  # (garbage in the tail bits of the prior selection)
                        now = K.apply_op(old, hit, op)
                        got = m.select_clusters(r, mode, lo, hi, op, flt)
                        assert got == (int(hit.sum()), int(now.sum())) and got[0] == implied, (prior, flt, mode, op, got)
                        assert np.array_equal(sb.download(), X.words(now)), (prior, flt, mode, op)  # tail bits zero
                if prior is None:
                    assert not K.hits(want, K.SEEDED).any()  # a model without a selection has no seeds
        # the out pointers are optional; a forced table gives the same selection
        desc = _lib.ClusterSelectDesc(0, 0, K.SET, K.BY_SIZE, float(r), 1, 2, 1)
        assert v._L.gsx_model_select_clusters(v._h, SRC.encode(), C.byref(desc), None, None) == _lib.GSX_OK
        assert np.array_equal(sb.download(), X.words(K.hits(K.clusters(pos, finite, r), K.BY_SIZE, 1, 2)))


def test_select_sums_more_partials_than_the_finish_has_lanes():
    n = FINISH_N
    with MultiModelViewer(sh=ShKind.Remove) as v:
        m, _ = _points_model(v, _finish_lattice())
        got = m.clusters(0.25)
        assert (got.count, got.n_clusters, got.largest_size) == (n, n, 1)
        assert m.select_clusters(0.25, K.BY_SIZE, 1, 1, K.SET) == (n, n) and _selection_is(m.gaussian_buffers.selection_buffer, True)


def test_keep_the_largest_recipe_then_extract_and_frames():
    n = 2500
    g = common.small_scene(n, 37)
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _load(vv, g)
        m = v.models[SRC]
        pos = _pod(v)[0]
        r = _radius(pos, RADIUS_K)
        want = K.clusters(pos, np.ones(n, bool), r)
        keep = K.hits(want, K.LARGEST)
        assert 1 < keep.sum() == want.largest_size < n
        assert m.select_clusters(r, K.LARGEST) == (int(keep.sum()), int(keep.sum()))  # a model without a selection gets one
        assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), X.words(keep))
        twin.models[SRC].gaussian_buffers.selection_buffer.upload(X.words(keep))
        assert m.extract("kept", X.SELECTED) == int(keep.sum()) == twin.models[SRC].extract("kept", X.SELECTED)
        assert _pod(v, "kept")[0].tobytes() == pos[keep].tobytes()
        for a, b in zip(_frames(v, ["kept"], poses=(4, 5, 6, 7)), _frames(twin, ["kept"], poses=(4, 5, 6, 7))):
            assert a[..., :3].max() > 0 and np.array_equal(a, b)
        # debris: every cluster below 5
        small = K.hits(want, K.BY_SIZE, 1, 4)
        assert m.select_clusters(r, K.BY_SIZE, 1, 4) == (int(small.sum()), int(small.sum())) and 0 < small.sum() < n
        assert m.extract("clean", X.SELECTED, invert=True) == n - int(small.sum())
        assert _pod(v, "clean")[0].tobytes() == pos[~small].tobytes()


def test_select_linked_recipe_brush_then_seeded_add():
    n = 2500
    g = common.small_scene(n, 39)
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _load(vv, g)
            vv.update_selection_edit_with_pod(query.GaussianEditPod(EF.ENABLED, alpha=0.6))
            vv.update_selection_highlight(HIGHLIGHT)
        m = v.models[SRC]
        sb = m.gaussian_buffers.selection_buffer
        pos = _pod(v)[0]
        r = _radius(pos, RADIUS_K)
        plain = _frames(v, [SRC], poses=(4,))[0]
        # the brush: a short stroke in the middle of the frame, as the app makes it
        v.update_camera(camera.orbit_pose(4), (W, H))
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
        v.update_query(query.QueryPod.brush((W / 2 - 6.0, H / 2), (W / 2 + 6.0, H / 2), 5.0, query.QuerySelectionOp.Set))
        v.preprocessor.preprocess(SRC)
        v.radix_sorter.sort(SRC)
        v.renderer.render([SRC])
        v.postprocessor.postprocess(SRC)
        v.poll()
        v.update_query(query.QueryPod.none())
        seeds = _bits(sb.download(), n)
        want = K.clusters(pos, np.ones(n, bool), r)
        linked = K.hits(want, K.SEEDED, seeds=seeds)
        assert 0 < seeds.sum() < linked.sum() < n  # the brush took something, the clusters add to it
        assert m.select_clusters(r, K.SEEDED, op=K.ADD) == (int(linked.sum()), int(linked.sum()))
        assert np.array_equal(sb.download(), X.words(linked))
        twin.models[SRC].gaussian_buffers.selection_buffer.upload(X.words(linked))
        got, expect = _frames(v, [SRC], poses=(4, 5, 6, 7)), _frames(twin, [SRC], poses=(4, 5, 6, 7))
        assert not np.array_equal(got[0], plain)  # (the selection shows)
        for a, b in zip(got, expect):
            assert np.array_equal(a, b)


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
            m.select_clusters(r, K.LARGEST)  # behind the frames in flight on the lanes
        else:
            c = K.clusters(_pod(v)[0], np.ones(g.shape[0], bool), r)
            m.gaussian_buffers.selection_buffer.upload(X.words(K.hits(c, K.LARGEST)))
        for pose in (5, 6, 7, 8):
            out += _frames(v, [SRC], poses=(pose,))
    return out


def test_lanes():
    g = common.small_scene(2500, 38)
    r = _radius(g["pos"], RADIUS_K)
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
            r = _radius(pos, RADIUS_K)
            a = m.clusters(r)
            _check(a, K.clusters(pos, np.ones(n, bool), r), (sh, cov))
            for _ in range(20):  # the order of the atomics differs from run to run; no bit does
                assert _same(m.clusters(r), a)
            v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)  # model space: the transform changes nothing
            assert _same(m.clusters(r), a)
            first = m.select_clusters(r, K.BY_SIZE, 1, 3)
            words = m.gaussian_buffers.selection_buffer.download()
            assert m.select_clusters(r, K.BY_SIZE, 1, 3) == first and np.array_equal(m.gaussian_buffers.selection_buffer.download(), words)
            results.append((float(r), a.labels.tobytes(), a.sizes.tobytes()))
    assert results[0] == results[1]  # the position plane is float32 in every pod kind


# ---- 6. workspace, and what a labelling writes ------------------------------------------------------------------------------------------
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
        r = _radius(_pod(v)[0], RADIUS_K)
        first = m.clusters(r)  # (the first call sizes the shared workspace)
        held = viewer_mod.device_bytes()
        for flt in (0, 3, 7):
            m.clusters(r, filter=flt)
            m.clusters(r * F(2), filter=flt)
        m.neighbors(r)  # the other model operations fit into the same workspace, and leave the clusters' answer as it was
        m.histogram(0, 16, -1.0, 1.0)
        assert _same(m.clusters(r), first)
        assert viewer_mod.device_bytes() == held
        assert state(v) == start == state(twin)
        for a, b in zip(_frames(v, [SRC], poses=(6, 7)), _frames(twin, [SRC], poses=(6, 7))):
            assert np.array_equal(a, b)
        held = viewer_mod.device_bytes()  # (the frames have sized their own buffers)
        m.select_clusters(r, K.SEEDED, filter=3)
        m.clusters(r)
        assert viewer_mod.device_bytes() == held  # (the model has a selection buffer already)
    assert viewer_mod.device_bytes() == before  # released with the viewer


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors():
    """every refusal of spec section 19 but GSX_ERR_OOM, which a test cannot provoke without exhausting the device"""
    n = 300
    with MultiModelViewer() as v, MultiModelViewer() as other:
        g, mask, sel, flags = _filter_model(v, n, 61)
        L, key = v._L, SRC.encode()
        sb = v.models[SRC].gaussian_buffers.selection_buffer
        sel_before = sb.download()
        labels, sizes, stats = np.zeros(n, np.uint32), np.zeros(n, np.uint32), _lib.ClusterStats()
        hit, selected = C.c_uint64(), C.c_uint64()
        INV, NF, UNS = _lib.GSX_ERR_INVALID_ARG, _lib.GSX_ERR_NOT_FOUND, _lib.GSX_ERR_UNSUPPORTED

        def clusters(k=key, flt=0, flags_=0, radius=0.1, bits=0, reserved=(0, 0), desc=True, st=stats, vv=v):
            d = _lib.ClusterDesc(flt, flags_, radius, bits, (C.c_uint32 * 2)(*reserved))
            return L.gsx_model_clusters(vv._h if vv else None, k, C.byref(d) if desc else None, labels.ctypes.data, sizes.ctypes.data,
                                        C.byref(st) if st is not None else None)

        def select(k=key, flt=0, flags_=0, op=0, mode=K.BY_SIZE, radius=0.1, lo=1, hi=3, bits=0, reserved=(0, 0), desc=True, vv=v):
            d = _lib.ClusterSelectDesc(flt, flags_, op, mode, radius, lo, hi, bits, (C.c_uint32 * 2)(*reserved))
            return L.gsx_model_select_clusters(vv._h if vv else None, k, C.byref(d) if desc else None, C.byref(hit), C.byref(selected))

        bad_radii = (0.0, -1.0, float("nan"), float("inf"), 1e-23, 1.9e19)  # (1e-23: the square is 0; 1.9e19: the square is inf)
        cases = [
            (clusters(vv=None), INV), (clusters(k=None), INV), (clusters(desc=False), INV), (clusters(st=None), INV),
            (clusters(flt=8), INV), (clusters(flags_=1), INV), (clusters(bits=25), INV), (clusters(reserved=(1, 0)), INV),
            (clusters(reserved=(0, 1)), INV), (clusters(k=b"nope"), NF),
            (select(vv=None), INV), (select(k=None), INV), (select(desc=False), INV), (select(flt=8), INV), (select(flags_=1), INV),
            (select(op=3), INV), (select(mode=3), INV), (select(bits=25), INV), (select(lo=0, hi=3), INV), (select(lo=3, hi=2), INV),
            (select(mode=K.LARGEST, lo=1, hi=3), INV), (select(mode=K.LARGEST, lo=0, hi=1), INV), (select(mode=K.SEEDED, lo=1, hi=0), INV),
            (select(reserved=(1, 0)), INV), (select(reserved=(0, 1)), INV), (select(k=b"nope"), NF),
        ] + [(clusters(radius=r), INV) for r in bad_radii] + [(select(radius=r), INV) for r in bad_radii]
        for i, (got, want) in enumerate(cases):
            assert got == want, i
        assert b"gsx_model_select_clusters" in L.gsx_last_error_string()
        assert np.array_equal(sb.download(), sel_before)  # a refused select leaves the selection
        # the ends of the legal ranges; the labels and the sizes are optional
        assert clusters(bits=24, radius=4e-23) == _lib.GSX_OK and clusters(bits=1, radius=1.8e19) == _lib.GSX_OK
        assert select(mode=K.LARGEST, lo=0, hi=0, flt=X.SELECTED) == select(mode=K.SEEDED, lo=0, hi=0, op=K.ADD) == _lib.GSX_OK
        assert select(lo=1, hi=0xFFFFFFFF, op=K.ADD) == _lib.GSX_OK
        sb.upload(sel_before)
        d = _lib.ClusterDesc(0, 0, 0.1, 0)
        assert L.gsx_model_clusters(v._h, key, C.byref(d), None, None, C.byref(stats)) == _lib.GSX_OK and stats.count == n - 4
        assert np.array_equal(sb.download(), sel_before)
        # an empty model, and no participants: GSX_OK with zeros; Set then clears the selection
        v.add_model("empty", 0)
        e = v.models["empty"]
        got = e.clusters(0.1)
        assert (got.labels.size, got.count, got.n_nonfinite, got.n_clusters, got.largest_size, got.largest_label) == (0, 0, 0, 0, 0, K.NONE)
        assert e.select_clusters(0.1, K.LARGEST) == (0, 0) and e.select_clusters(0.1, K.BY_SIZE, 1, 3) == (0, 0)
        _load(v, g, "bare")
        none = v.models["bare"].clusters(0.1, filter=X.SELECTED)
        assert (none.count, none.n_nonfinite, none.n_clusters, none.largest_label) == (0, 0, 0, K.NONE) and (none.labels == K.NONE).all()
        assert v.models["bare"].select_clusters(0.1, K.LARGEST, filter=X.SELECTED) == (0, 0)
        assert v.models[SRC].select_clusters(1e-6, K.BY_SIZE, 5, 8) == (0, 0) and not sb.download().any()
        # a sharded model; a viewer with a communicator
        _frames(v, [SRC], poses=(5,))
        _load(v, g[:50], "b")
        v.shard_set_limits("b", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        _load(other, g[:50], "a")
        other.comm_init_group(CommGroup(1), 0)
        for model, word in ((v.models["b"], "shard"), (other.models["a"], "communicator")):
            for call in (lambda: model.clusters(0.1), lambda: model.select_clusters(0.1, K.LARGEST)):
                with pytest.raises(GsxError) as err:
                    call()
                assert err.value.status == UNS and word in str(err.value)
