"""CPU: tests/model_shadow.py, the host shadow and schedule of tests/test_gpu_model_fuzz.py, without a GPU: the schedule is the same on
every run and covers every op kind (condition (a) of the fuzz), the shadow carries keys, kinds, mask, selection and edits through
extract, merge and convert as tests/extract_ref.py's kept set says, `verify` finds a wrong row, and the select parameters the default
seeds draw give hit sets that are neither empty nor full under the restatements alone (condition (b)), on the scenes the GPU test uses.
A decimate follows the kept set, orders its cells by representative and takes its merged rows from tests/decimate_driver.cpp (a host
program built once per module); select_nearest writes the source and reads both selections as they were; and the default seeds meet
the fuzz's conditions (e), (f) and (h) on decimate, the nearest calls across two models and the align step, and (i) to (m) on the
visibility and depth map calls, which depend on what is resident when a call comes and not on what the planes hold."""
import functools

import numpy as np
import pytest

from tests import decimate_ref as D
from tests import extract_ref as X
from tests import model_shadow as S
from tests import nearest_ref as R
from tests import property_ref as P
from tests import transform_ref as T

F = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/decimate_driver.cpp, a stand-alone host program: the merged rows of a decimate, on the host as on the device"""
    return D.build_driver(tmp_path_factory.mktemp("decimate"))


@functools.lru_cache(maxsize=None)
def _host_run(seed, driver, again=0):
    """a seed's whole schedule applied to the shadow alone"""
    s = S.Session(seed, driver)
    s.load_start()
    for kind in S.plan(seed):
        s.apply({"kind": "cam_step"} if kind == "cam_step" else s.draw(kind))
    return s


def test_the_schedule_covers_every_op_kind_and_is_the_same_on_every_run():
    assert len(set(S.OP_KINDS)) == len(S.OP_KINDS) and set(S.MODEL_CHANGING) | set(S.SELECTS) | set(S.READ_ONLY) <= set(S.OP_KINDS)
    assert "decimate" in S.MODEL_CHANGING and "select_nearest" in S.SELECTS and {"decimate_edge", "nearest", "align_step"} <= set(S.READ_ONLY)
    assert set(S.NEAREST_FAMILY) <= set(S.SPATIAL) <= set(S.OP_KINDS) and {v.split(":")[0] for v in S.SELECT_VARIANTS} == set(S.SELECTS)
    # the visibility and depth map calls: "visibility" is the camera op that hides models, the calls go by other names
    assert set(S.VIEW_CALLS) == {"vis_view", "depth_map"} <= set(S.READ_ONLY) and "select_visibility" in S.SELECTS and "visibility" in S.CAMERA
    assert set(S.DEVICE_ONLY_VARIANTS) == {"select_visibility:" + m for m in S.VIS_MEASURES} <= set(S.SELECT_VARIANTS)
    for seed in S.DEFAULT_SEEDS:
        p = S.plan(seed)
        assert p == S.plan(seed)
        assert set(p) == set(S.OP_KINDS), (seed, set(S.OP_KINDS) - set(p))
        assert 0.45 <= p.count("cam_step") / len(p) <= 0.7, (seed, p.count("cam_step"), len(p))
        # a run of camera steps follows every op that changes a model
        for i, k in enumerate(p):
            if k in S.MODEL_CHANGING:
                assert p[i + 1:i + 1 + S.POST_OP_RUN] == ["cam_step"] * S.POST_OP_RUN, (seed, i, k)
    assert S.plan(1) != S.plan(2)
    starts = [S.START_KINDS[s % len(S.START_KINDS)] for s in S.DEFAULT_SEEDS]
    assert S.SINGLE in starts and S.NORM8_HALF in starts and set(starts) == set(S.KINDS)
    lanes = {S.Session(s).lanes for s in S.DEFAULT_SEEDS}
    assert lanes == {1, 2, 3}


@pytest.mark.parametrize("seed", [5, 7])
def test_the_drawn_parameters_are_the_same_on_every_run(seed, driver):
    a, b = _host_run(seed, driver), _host_run(seed, driver, 1)
    assert a is not b and a.log == b.log and len(a.log) == len(S.OP_KINDS) - 1 + S.EXTRA_OPS
    assert sorted(a.shadow.models) == sorted(b.shadow.models)
    for k, m in a.shadow.models.items():
        assert all(p.tobytes() == q.tobytes() for p, q in zip(m.planes, b.shadow.models[k].planes))  # (a decimate's merged rows too)
    kinds = [op["kind"] for op in a.log]
    assert {"decimate", "decimate_edge", "nearest", "select_nearest", "align_step", "vis_view", "depth_map", "select_visibility"} <= set(kinds)
    assert a.cases == b.cases and a.decimates == b.decimates and len(a.decimates) == kinds.count("decimate")
    assert (a.vis_views, a.vis_selects, a.vis_refusals, a.depth_maps) == (b.vis_views, b.vis_selects, b.vis_refusals, b.depth_maps)
    assert (len(a.vis_views), len(a.vis_selects), len(a.depth_maps)) == tuple(kinds.count(k) for k in ("vis_view", "select_visibility", "depth_map"))


def test_the_default_seeds_meet_the_conditions_on_decimate_nearest_and_align(driver):
    """(e), (f) and (h) of tests/test_gpu_model_fuzz.py, which draws the same parameters: stated once, in model_shadow.unmet.  (g) is
    the device's to count; that the draws ask for frames in flight is checked here."""
    runs = [_host_run(seed, driver) for seed in S.DEFAULT_SEEDS]
    unmet = S.unmet(set().union(*(s.cases for s in runs)), [d for s in runs for d in s.decimates])
    assert not unmet, unmet
    assert S.unmet(set(S.NEAREST_CASES), [d for s in runs for d in s.decimates]) == ["(h) no align draw that is not degenerate with a reference rotation above 1 degree"]
    assert len(S.unmet(set(), [dict(filtered=False, kind_differs=False, count=300, cells=300, singletons=300, largest_cell=1)])) == 9
    for kind in ("decimate", "select_nearest"):
        assert any(op["kind"] == kind and op["inflight"] >= 2 for s in runs if s.lanes > 1 for op in s.log), kind
    pairs = [(op["key"], op["dst"]) for s in runs for op in s.log if op["kind"] == "select_nearest"]
    assert any(a == b for a, b in pairs) and any(a != b for a, b in pairs)  # the source as its own target, and another model


def _vis_records(runs):
    return dict(views=[r for s in runs for r in s.vis_views], selects=[r for s in runs for r in s.vis_selects],
                refusals=[r for s in runs for r in s.vis_refusals], depth_maps=[r for s in runs for r in s.depth_maps])


def test_the_default_seeds_meet_the_conditions_on_visibility_and_the_depth_map(driver):
    """(i) to (m) of tests/test_gpu_model_fuzz.py, stated once in model_shadow.unmet_views.  They depend on the draws alone: on which
    planes are RESIDENT when a call comes (the shadow follows the library's drops), not on what the planes hold."""
    runs = [_host_run(seed, driver) for seed in S.DEFAULT_SEEDS]
    vis = _vis_records(runs)
    assert not S.unmet_views(**vis), S.unmet_views(**vis)
    assert not S.unmet(set().union(*(s.cases for s in runs)), [d for s in runs for d in s.decimates], vis)
    # nothing at all meets nothing: three of (i), two of (j), three and the three thresholds and three of (k), four of (l), three of (m)
    assert len(S.unmet_views([], [], [], [])) == 21
    # a refused call meets none of the conditions on the calls that ran
    refused = dict(vis, views=[dict(r, refused=True) for r in vis["views"]], depth_maps=[dict(r, refused=True) for r in vis["depth_maps"]])
    assert len(S.unmet_views(**refused)) == 3 + 9 + 2 + 2  # (all of (i) and (k), "run twice" of (l) and (m) for the two)
    # every refused view and depth map found planes, or a map of its viewport, resident: the refusal has something to leave as it was.
    # Some were there from an earlier op of the seed, the others from the unrefused call the session put in front (`primed`)
    for recs in (vis["views"], vis["depth_maps"]):
        assert all(r["resident"] for r in recs if r["refused"]) and any(r["primed"] for r in recs) and not any(r["primed"] and not r["refused"] for r in recs)
    assert any(r["refused"] and not r["primed"] for r in vis["views"])
    # a refusal without anything resident does not meet (l)
    bare = dict(vis, views=[dict(r, resident=False) for r in vis["views"]], depth_maps=[dict(r, resident=False) for r in vis["depth_maps"]])
    assert len(S.unmet_views(**bare)) == 2
    # each of the three calls that drop a model's planes did so somewhere, and a select by them was refused at once; two do not meet (j)
    assert set(vis["refusals"]) == set(S.DROPPERS) and len(S.unmet_views(**dict(vis, refusals=list(S.DROPPERS[:2])))) == 1
    # some depth map ran without the ndc plane
    assert any(not op["ndc"] for s in runs for op, r in zip([o for o in s.log if o["kind"] == "depth_map"], s.depth_maps) if not r["refused"])
    # every measure of a select_visibility is drawn on resident planes somewhere (the hit sets are the device's to show: condition (b))
    ran = {op["measure"] for s in runs for op, r in zip([o for o in s.log if o["kind"] == "select_visibility"], s.vis_selects) if not r["refused"]}
    assert ran == {0, 1, 2}


def test_every_select_variant_is_non_trivial_somewhere_in_the_default_seeds(driver):
    """The three select_visibility variants are the device's to show (tests/test_gpu_model_fuzz.py asserts them with the others): the
    host run holds no planes to select by, and says so here instead of dropping them silently."""
    seen, sizes = set(), []
    for seed in S.DEFAULT_SEEDS:
        s = _host_run(seed, driver)
        seen |= s.nontrivial
        assert 1 <= len(s.shadow.models) <= S.MAX_MODELS
        sizes += [m.n for m in s.shadow.models.values()]
        assert all(s.ran.get(k) for k in S.OP_KINDS if k != "cam_step"), seed
    assert seen == set(S.SELECT_VARIANTS) - set(S.DEVICE_ONLY_VARIANTS), (set(S.SELECT_VARIANTS) - seen, seen & set(S.DEVICE_ONLY_VARIANTS))
    assert S.MIN_N <= min(sizes) and max(sizes) <= S.MAX_N


# ---- the shadow's bookkeeping on hand-built cases -------------------------------------------------------------------------------------
def _planes(n, base):
    pos = (np.arange(3 * n, dtype=F).reshape(n, 3) + F(base)) / F(8)
    return [pos, np.arange(n, dtype=np.uint32) + np.uint32(base), np.full((n, 45), base, F), np.full((n, 6), base + 1, F)]


def _dressed(sh, key, n, base, kind=S.SINGLE, mt=(S.ZERO3, S.IDENT, S.ONE3)):
    m = sh.add(key, kind, _planes(n, base), mt)
    i = np.arange(n)
    m.mask, m.sel = i % 3 != 0, i % 2 == 0
    e = S.default_edits(n)
    e["flag"][i % 5 == 0] = 3      # enabled and hidden
    e["flag"][i % 5 == 1] = 1      # enabled
    e["flag"][i % 5 == 2] = 2      # hidden without enabled: hides nothing, and reads back as the default
    e["alpha"] = F(0.5)
    m.edits = S.normalise_edits(e)
    return m


def test_edit_records_are_kept_as_the_library_keeps_them():
    m = _dressed(S.Shadow(), "a", 40, 0)
    i = np.arange(40)
    assert (m.edits["flag"][i % 5 == 2] == 0).all() and (m.edits["alpha"][i % 5 >= 2] == 1).all() and (m.edits["alpha"][i % 5 < 2] == F(0.5)).all()
    assert np.array_equal(X.hidden(m.edits["flag"]), i % 5 == 0)


@pytest.mark.parametrize("flt", S.FILTERS)
@pytest.mark.parametrize("invert", [False, True])
def test_extract_and_convert_follow_the_kept_set(flt, invert):
    n = 70
    sh = S.Shadow()
    mt = (F([1, 2, 3]), F([0, 0, 1, 0]), F([1, 2, 1]))
    m = _dressed(sh, "a", n, 100, mt=mt)
    want = X.kept(n, flt, X.INVERT if invert else 0, m.mask, m.sel, m.edits["flag"])
    count, exact = sh.extract("a", "b", flt, invert)
    assert count == want.size
    if count == 0:
        assert "b" not in sh.models and exact is None
        return
    d = sh.models["b"]
    assert d.kind == m.kind and d.mask is None and d.sel is None and not d.unedited and all(np.array_equal(x, y) for x, y in zip(d.mt, mt))
    assert all(np.array_equal(a, b[want]) for a, b in zip(d.planes, m.planes)) and all(e.all() for e in exact)
    assert d.edits.tobytes() == m.edits[want].tobytes()
    # a conversion: the same rows, the new kind, covariance and SH left to the device; drop_edits
    count, exact = sh.extract("a", "c", flt, invert, drop_edits=True, kind=S.NORM8_HALF)
    c = sh.models["c"]
    assert count == want.size and c.kind == S.NORM8_HALF and c.edits is None
    assert exact[0].all() and exact[1].all() and not exact[2].any() and not exact[3].any()
    assert np.array_equal(c.pos, m.pos[want]) and np.array_equal(c.color, m.color[want])
    assert sh.models["a"] is m and m.n == n  # the source is not written


def _backwards(m):
    """the model's positions in reverse: along the diagonal the cell key then FALLS with the index, so that the ascending order of the
    cells' representatives is the descending order of their keys"""
    m.planes[0] = np.ascontiguousarray(m.planes[0][::-1])
    return m


@pytest.mark.parametrize("flt", S.FILTERS)
@pytest.mark.parametrize("invert", [False, True])
def test_decimate_follows_the_kept_set_and_orders_by_representative(flt, invert, driver):
    """_planes puts Gaussian i at 3 i / 8 on every axis (here: 3 (n - 1 - i) / 8): under a cell edge of 2 the cell of a participant
    is floor(3 (i_last - i) / 16), i_last the participant at the grid's origin: five or six neighbours a cell, fewer where the filter
    leaves gaps"""
    n = 70
    sh = S.Shadow()
    mt = (F([1, 2, 3]), F([0, 0, 1, 0]), F([1, 2, 1]))
    m = _backwards(_dressed(sh, "a", n, 100, mt=mt))
    before = [p.copy() for p in m.planes]
    want = X.kept(n, flt, X.INVERT if invert else 0, m.mask, m.sel, m.edits["flag"])
    stats, dmap, exact = sh.decimate("a", "b", 2.0, flt, invert, driver)
    if want.size == 0:
        assert stats == (0, 0, 0, 0, 0) and (dmap == D.NO_CELL).all() and "b" not in sh.models and exact is None
        return
    key = 3 * (want.max() - want) // 16
    rank = np.unique(-key, return_inverse=True)[1].reshape(-1)  # the cells in the order their first member comes
    members = np.bincount(rank)
    assert stats == (want.size, 0, members.size, int((members == 1).sum()), int(members.max()))
    assert np.array_equal(dmap[want], rank) and (np.delete(dmap, want) == D.NO_CELL).all()  # non-participants go nowhere
    rep = want[np.unique(rank, return_index=True)[1]]
    assert np.array_equal(np.sort(rep), rep) and (members > 1).any()
    d = sh.models["b"]
    assert d.n == members.size and d.kind == m.kind and d.mask is None and d.sel is None and d.edits is None and not d.unedited
    assert all(np.array_equal(x, y) for x, y in zip(d.mt, mt))
    single = members == 1
    for k in range(4):  # a one-member cell is its member's row; Single + Single: the driver's merged rows are known too
        assert np.array_equal(d.planes[k][single], m.planes[k][rep[single]]) and exact[k].all()
    for j in np.nonzero(~single)[0]:  # a merged Gaussian lies among its cell's members, and is not its representative
        p = m.pos[want[rank == j]]
        assert (p.min(axis=0) <= d.pos[j]).all() and (d.pos[j] <= p.max(axis=0)).all() and not np.array_equal(d.pos[j], m.pos[rep[j]])
    assert all(np.array_equal(a, b) for a, b in zip(m.planes, before)) and sh.models["a"] is m  # the source is not written
    # without the driver the merged rows are nobody's to say; in a compressed kind the device quantises them: pos and colour are known
    _, _, loose = sh.decimate("a", "c", 2.0, flt, invert)
    assert all(np.array_equal(e, single) for e in loose)
    m.kind = S.NORM8_HALF
    _, _, half = sh.decimate("a", "e", 2.0, flt, invert, driver)
    assert half[0].all() and half[1].all() and np.array_equal(half[2], single) and np.array_equal(half[3], single) and sh.models["e"].kind == S.NORM8_HALF


@pytest.mark.parametrize("flt", [0, X.MASKED | X.SKIP_HIDDEN, X.SELECTED])
def test_a_decimate_of_singletons_is_an_extract_that_drops_the_edits(flt, driver):
    sh = S.Shadow()
    m = _backwards(_dressed(sh, "a", 70, 100))
    stats, dmap, exact = sh.decimate("a", "b", 0.125, flt, False, driver)  # the Gaussians are 3 / 8 apart
    count, _ = sh.extract("a", "x", flt, False, drop_edits=True)
    assert stats == (count, 0, count, count, 1) and np.array_equal(dmap[m.kept(flt)], np.arange(count)) and all(e.all() for e in exact)
    b, x = sh.models["b"], sh.models["x"]
    assert all(p.tobytes() == q.tobytes() for p, q in zip(b.planes, x.planes)) and b.edits is None and x.edits is None
    assert b.kind == x.kind and all(np.array_equal(p, q) for p, q in zip(b.mt, x.mt))


def _nearest_by_hand(q, t, t_part):
    """index of the nearest participating target, float64 (the cases below have no ties and no rounding to speak of)"""
    d = ((q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    d[:, ~t_part] = np.inf
    return d.argmin(axis=1), np.sqrt(d.min(axis=1))


def _applied(op, old, hit):
    return hit if op == P.SET else (old | hit if op == P.ADD else old & ~hit)


def test_select_nearest_range_and_transfer_apply_every_op_to_the_source():
    sh = S.Shadow()
    a, b = _dressed(sh, "a", 60, 0), _dressed(sh, "b", 40, 4)  # b's Gaussian j lies 4 / 8 up the diagonal from a's Gaussian j
    prior, b_sel = a.sel.copy(), b.sel.copy()
    for fs, fd in ((0, 0), (X.SELECTED, X.MASKED), (X.MASKED | X.SKIP_HIDDEN, X.SELECTED)):
        q_part, t_part = a.passes(fs), b.passes(fd)
        index, d = _nearest_by_hand(a.pos, b.pos, t_part)
        lo, hi = np.quantile(d[q_part], [0.2, 0.7])
        for transfer, hit in ((False, q_part & (d >= F(lo)) & (d <= F(hi))), (True, q_part & b_sel[index])):
            assert 0 < hit.sum() and (hit.sum() < q_part.sum() or (transfer and fd & X.SELECTED)), (fs, fd, transfer)  # (only selected targets: all hit)
            for op in (P.SET, P.ADD, P.REMOVE):
                a.sel = prior.copy()
                want = _applied(op, prior, hit)
                got = sh.select_nearest("a", "b", transfer, 0.0 if transfer else float(F(lo)), 0.0 if transfer else float(F(hi)), op, fs, fd)
                assert got == (int(hit.sum()), int(want.sum())) and np.array_equal(a.sel, want), (fs, fd, transfer, op)
                assert np.array_equal(b.sel, b_sel)  # the target's selection is read, never written
    # a max_distance: what lies beyond finds nothing, and a transfer does not hit it
    index, d = _nearest_by_hand(a.pos, b.pos, np.ones(40, bool))
    reach = 0.25  # (the neighbours up the diagonal are sqrt(3) / 8 away; the first Gaussian of `a` and those past `b`'s end are further)
    a.sel = None
    hit = (d <= reach) & b_sel[index]
    assert sh.select_nearest("a", "b", True, max_distance=reach) == (int(hit.sum()), int(hit.sum())) and 0 < hit.sum() < b_sel[index].sum()
    # a target model without a selection: no hits, and Set then clears the source's selection
    a.sel, b.sel = prior.copy(), None
    assert sh.select_nearest("a", "b", True, op=P.ADD) == (0, int(prior.sum())) and np.array_equal(a.sel, prior)
    assert sh.select_nearest("a", "b", True, op=P.SET) == (0, 0) and not a.sel.any() and b.sel is None


def test_select_nearest_on_one_model_reads_the_selection_as_it_was():
    """src == dst under a matrix that carries every Gaussian onto the next one up the diagonal, or the one before: Gaussian i finds
    i + 1 or i - 1, so a transfer shifts the selection by one, down or up, which shows at once whether bits written by the call were
    read back, in whichever order of the indices it writes"""
    n = 60
    sh = S.Shadow()
    m = _dressed(sh, "a", n, 0)
    m.sel = np.arange(n) % 5 < 2
    prior = m.sel.copy()
    up, down = (np.concatenate([np.eye(3), np.full((3, 1), step / 8)], axis=1).astype(F) for step in (3, -3))
    for xform, found in ((up, np.minimum(np.arange(n) + 1, n - 1)), (down, np.maximum(np.arange(n) - 1, 0))):
        assert np.array_equal(sh.nearest("a", "a", xform=xform)["index"], found)
        for fs in (0, X.SELECTED):
            hit = prior[found] & (prior if fs else True)
            for op in (P.SET, P.ADD, P.REMOVE):
                m.sel = prior.copy()
                want = _applied(op, prior, hit)
                assert sh.select_nearest("a", "a", True, op=op, src_filter=fs, xform=xform) == (int(hit.sum()), int(want.sum())), (fs, op)
                assert np.array_equal(m.sel, want) and (op == P.ADD or not np.array_equal(want, prior))
    # RANGE with the SELECTED filter on both sides: the participants and the targets are the selection as it was
    m.sel = prior.copy()
    index, d = _nearest_by_hand(R.map_points(up, m.pos), m.pos, prior)
    hit = prior & (d <= 0.25)
    assert 0 < hit.sum() < prior.sum()
    assert sh.select_nearest("a", "a", False, 0.0, 0.25, P.SET, X.SELECTED, X.SELECTED, up) == (int(hit.sum()), int(hit.sum())) and np.array_equal(m.sel, hit)


def test_merge_orders_the_sources_and_bakes_positions():
    sh = S.Shadow()
    a = _dressed(sh, "a", 33, 0)
    mt = (F([0.5, 0, -1]), F([0, 0, 1, 1]), F([1, -2, 1]))
    b = sh.add("b", S.SINGLE, _planes(50, 1000), mt)  # no mask, selection or edits
    b.sel = np.arange(50) < 20
    flt = X.MASKED | X.SKIP_HIDDEN
    ka, kb = a.kept(flt), b.kept(flt)
    assert kb.size == 50 and np.array_equal(ka, X.kept(33, flt, 0, a.mask, a.sel, a.edits["flag"]))
    total, counts, exact = sh.merge("ab", ["a", "b", "a"], flt)
    d = sh.models["ab"]
    assert (total, counts) == (2 * ka.size + 50, [ka.size, 50, ka.size]) and d.n == total and d.kind == S.SINGLE
    assert S.M.is_identity(*d.mt) and d.mask is None and d.sel is None
    o = ka.size
    for k in range(4):  # the identity source twice, its stored rows; in between the baked one: positions and colour words known
        assert np.array_equal(d.planes[k][:o], a.planes[k][ka]) and np.array_equal(d.planes[k][o + 50:], a.planes[k][ka])
        assert exact[k][:o].all() and exact[k][o + 50:].all() and exact[k][o:o + 50].all() == (k < 2)
    assert d.pos[o:o + 50].tobytes() == T.position(b.pos, *mt).tobytes() and np.array_equal(d.color[o:o + 50], b.color)
    assert d.edits[:o].tobytes() == a.edits[ka].tobytes() and d.edits[o:o + 50].tobytes() == S.default_edits(50).tobytes()
    # SELECTED: a source without a selection gives nothing; nothing at all creates no model; drop_edits
    b.sel = None
    assert sh.merge("none", ["b"], X.SELECTED) == (0, [0], None) and "none" not in sh.models
    total, counts, _ = sh.merge("sel", ["b", "a"], X.SELECTED, drop_edits=True)
    assert counts == [0, int(a.sel.sum())] and sh.models["sel"].edits is None
    with pytest.raises(AssertionError):
        sh.add("x", S.NORM8_HALF, _planes(4, 0))
        sh.merge("bad", ["a", "x"])


def test_apply_transform_touches_the_kept_rows_only():
    sh = S.Shadow()
    m = _dressed(sh, "a", 45, 7)
    before = [p.copy() for p in m.planes]
    kept = m.kept(X.SELECTED)
    t, q, s = F([0.25, 0, -1]), F([0, 1, 0, 1]), F([1, 1, -1.5])
    pivot = F([1, 2, 3])
    for (tt, qq, ss), loose in (((t, S.IDENT, S.ONE3), ()), ((S.ZERO3, S.IDENT, s), (3,)), ((t, q, s), (2, 3))):
        start = m.pos.copy()
        count, exact = sh.apply_transform("a", tt, qq, ss, pivot, X.SELECTED)
        assert count == kept.size and m.pos[kept].tobytes() == T.position(start[kept], tt, qq, ss, pivot).tobytes()
        rest = np.setdiff1d(np.arange(45), kept)
        assert np.array_equal(m.pos[rest], before[0][rest])
        for k in range(4):
            assert exact[k][rest].all() and exact[k][kept].all() == (k not in loose), (k, loose)
    count, exact = sh.apply_transform("a", S.ZERO3, F([0, 0, 0, -1]), S.ONE3, pivot)  # the identity writes nothing
    assert count == 45 and all(e.all() for e in exact)
    assert all(np.array_equal(a, b) for a, b in zip(m.planes[1:], before[1:]))


def test_visibility_planes_are_dropped_exactly_where_the_library_drops_them():
    """Model::vis in the shadow: residency alone (no device to adopt planes from)"""
    s = S.Session(1)
    sh = s.shadow
    m = _dressed(sh, "a", 45, 7)
    _dressed(sh, "b", 30, 9)
    t = F([0.25, 0, -1])

    def view(key="a", accumulate=False):
        return s._view(key, s.view.pose, accumulate, None)

    assert m.vis is None and view() == (1, False) and m.vis["views"] == 1 and m.vis_lost is None
    s.view.pose += 1
    assert view(accumulate=True) == (2, True) and view(accumulate=True) == (3, True) and view() == (1, False)
    # kept: mask, selection, edit, show-unedited, model transform, camera; the identity transform and an empty kept set
    for op in (dict(kind="mask_eval", key="a", expr="0"), dict(kind="sel_upload", key="a", rseed=3, density=0.5), dict(kind="edits_upload", key="a", rseed=4),
               dict(kind="unedited", key="a", on=True), dict(kind="model_transform", key="a", mt=(t, S.IDENT, S.ONE3)), dict(kind="cam_jump", pose=7),
               dict(kind="viewport", size=(83, 51)), dict(kind="visibility", hidden=["a"])):
        s.apply(op)
    assert m.vis is not None and m.vis["survived"] == {"mask", "sel", "edit"}
    sh.apply_transform("a", S.ZERO3, S.IDENT, S.ONE3)
    m.sel = np.zeros(m.n, bool)
    sh.apply_transform("a", t, S.IDENT, S.ONE3, flt=X.SELECTED)
    assert m.vis is not None and m.vis_lost is None
    # dropped: a transform that moves something, a pod kind change; a new model starts without
    sh.apply_transform("a", t, S.IDENT, S.ONE3)
    assert m.vis is None and m.vis_lost == "apply_transform"
    view()
    assert m.vis_lost is None and m.vis["survived"] == set()
    sh.set_pod_kind("a", S.NORM8_HALF)
    assert m.vis is None and m.vis_lost == "set_pod_kind"
    sh.set_pod_kind("a", S.SINGLE)
    assert m.vis_lost == "set_pod_kind"  # (nothing was resident: nothing was dropped)
    view()
    view("b")
    sh.extract("a", "c")
    sh.merge("d", ["a", "b"])
    assert sh.models["c"].vis is None and sh.models["d"].vis is None and m.vis is not None and sh.models["b"].vis is not None
    # the views of the two models are their own
    assert sh.models["b"].vis["views"] == 1 and sh.models["b"].vis["at"] == m.vis["at"]


def test_verify_finds_a_wrong_row_where_the_shadow_knows_it(driver):
    sh = S.Shadow()
    # after a decimate the merged rows are the driver's: the shadow claims to know them where the kind stores float32
    src = _backwards(_dressed(sh, "src", 70, 100))
    stats, dmap, exact = sh.decimate("src", "dec", 1.0, X.MASKED, False, driver)
    d = sh.models["dec"]
    merged = np.nonzero(np.bincount(dmap[dmap != D.NO_CELL]) > 1)[0]
    assert 0 < merged.size == stats[2] - stats[3] < d.n and src.n == 70
    sh.verify("dec", [p.copy() for p in d.planes], exact)
    for plane in range(4):
        wrong = [p.copy() for p in d.planes]
        row = wrong[plane].reshape(d.n, -1).view(np.uint32)
        row[merged[-1], 0] ^= 1  # one unit in the last place of a merged row, or one colour level
        with pytest.raises(AssertionError):
            sh.verify("dec", wrong, exact)
    sh.remove("dec")
    sh.remove("src")
    m = sh.add("a", S.SINGLE, _planes(20, 3))
    good = [p.copy() for p in m.planes]
    sh.verify("a", good, S._all(20))
    bad = [p.copy() for p in good]
    bad[3][7, 2] = np.nextafter(bad[3][7, 2], F(np.inf))
    with pytest.raises(AssertionError):
        sh.verify("a", bad, S._all(20))
    loose = S._all(20)
    loose[3][7] = False
    sh.verify("a", bad, loose)  # that row is the device's to say
    with pytest.raises(AssertionError):
        sh.verify("a", [p[:19] for p in good], S._all(20))  # the count
    swapped = [p.copy() for p in good]
    swapped[0][[2, 3]] = swapped[0][[3, 2]]
    with pytest.raises(AssertionError):
        sh.verify("a", swapped, S._all(20))  # the order
    sh.adopt("a", bad)
    sh.verify("a", bad, S._all(20))
