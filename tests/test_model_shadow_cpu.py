"""CPU: tests/model_shadow.py, the host shadow and schedule of tests/test_gpu_model_fuzz.py, without a GPU: the schedule is the same on
every run and covers every op kind (condition (a) of the fuzz), the shadow carries keys, kinds, mask, selection and edits through
extract, merge and convert as tests/extract_ref.py's kept set says, `verify` finds a wrong row, and the select parameters the default
seeds draw give hit sets that are neither empty nor full under the restatements alone (condition (b)), on the scenes the GPU test uses."""
import functools

import numpy as np
import pytest

from tests import extract_ref as X
from tests import model_shadow as S
from tests import transform_ref as T

F = np.float32


@functools.lru_cache(maxsize=None)
def _host_run(seed, again=0):
    """a seed's whole schedule applied to the shadow alone"""
    s = S.Session(seed)
    s.load_start()
    for kind in S.plan(seed):
        s.apply({"kind": "cam_step"} if kind == "cam_step" else s.draw(kind))
    return s


def test_the_schedule_covers_every_op_kind_and_is_the_same_on_every_run():
    assert len(set(S.OP_KINDS)) == len(S.OP_KINDS) and set(S.MODEL_CHANGING) | set(S.SELECTS) | set(S.READ_ONLY) <= set(S.OP_KINDS)
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
def test_the_drawn_parameters_are_the_same_on_every_run(seed):
    a, b = _host_run(seed), _host_run(seed, 1)
    assert a is not b and a.log == b.log and len(a.log) == len(S.OP_KINDS) - 1 + S.EXTRA_OPS
    assert sorted(a.shadow.models) == sorted(b.shadow.models)
    for k, m in a.shadow.models.items():
        assert m.planes[0].tobytes() == b.shadow.models[k].planes[0].tobytes()


def test_every_select_variant_is_non_trivial_somewhere_in_the_default_seeds():
    seen, sizes = set(), []
    for seed in S.DEFAULT_SEEDS:
        s = _host_run(seed)
        seen |= s.nontrivial
        assert 1 <= len(s.shadow.models) <= S.MAX_MODELS
        sizes += [m.n for m in s.shadow.models.values()]
        assert all(s.ran.get(k) for k in S.OP_KINDS if k != "cam_step"), seed
    assert seen == set(S.SELECT_VARIANTS), set(S.SELECT_VARIANTS) - seen
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


def test_verify_finds_a_wrong_row_where_the_shadow_knows_it():
    sh = S.Shadow()
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
