"""GPU: gsx_model_property_values, gsx_model_histogram and gsx_model_select_range (spec/RENDER_SPEC.md §17;
csrc/kernels_property.hip).  Equality is exact everywhere.  The yardsticks: gsx_model_download_pod for the stored positions and colour
words, the float32 restatement tests/property_ref.py for the HSV, the bins, the hit set and the op (tests/test_property_cpu.py ties
it to csrc/property_math.h, the header the kernels include), gsx_model_export for the scales, gsx_model_merge for world positions,
tests/extract_ref.py for the filter, gsx_model_upload_selection for the frames.
Sizes: a workgroup takes chunks of 1024 Gaussians in four rounds of 256, a wave 64 of them (two selection words): one Gaussian; a
word and wave edge (63, 64, 65); a round edge (256, 257); a chunk edge (1024, 1025); several chunks with a partial last one (5000);
and one model past 2048 chunks, where a workgroup takes more than one chunk (1024 chunks in the histogram)."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import extract_ref as X
from tests import property_ref as P
from tests.model_ops import H, KIND_IDS, KINDS, W, frames as _frames, load as _load, model_len as _len, pod as _pod
from wgpu_3dgs_viewer_app_amd import _lib, query
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as EF
from wgpu_3dgs_viewer_app_amd.viewer import CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
SRC = "src"
F = np.float32
SIZES = [1, 63, 64, 65, 256, 257, 1024, 1025, 5000]
PC_PROPS = list(range(10))
HIGHLIGHT = (1.0, 0.0, 1.0, 0.3)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b, what=""):
    assert np.asarray(a).shape == np.asarray(b).shape and _bits(a).tobytes() == _bits(b).tobytes(), what


def _filter_model(v, n, seed=7, key=SRC):
    """a model with a mask, a selection (garbage in both tails) and stored edits (some ENABLED + HIDDEN), NaN and infinite
    positions (when it has room for them); returns the host arrays"""
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


def _check_hist(h, want, what):
    assert np.array_equal(h.bins, want["bins"]), what
    assert (h.count, h.below, h.above, h.n_nonfinite) == (want["count"], want["below"], want["above"], want["n_nonfinite"]), what
    for name in ("lo", "hi", "min", "max"):
        assert _bits(getattr(h, name))[()] == _bits(want[name])[()], (what, name, getattr(h, name), want[name])
    assert int(h.bins.sum()) == h.count - h.below - h.above, what


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_values_of_all_eight_pod_kinds(sh, cov):
    n = 1500
    g = common.small_scene(n, 67)
    g["scale"][0:100] = g["scale"][0:100, :1]        # spheres
    g["scale"][100:200, 2] = 0                        # one zero scale
    g["scale"][200:300] = 0                           # an all-zero covariance
    g["scale"][300:308] = F([300.0, 2.0, 0.5])        # 300^2 overflows a Half covariance: no solve, the diagonal's roots
    g["rot"][300:308] = F([0, 0, 0, 1])
    g["pos"][310] = [np.nan, np.inf, -0.0]            # carried as bits
    g["color"][311:315] = [[0, 0, 0, 0], [255, 255, 255, 255], [128, 128, 128, 7], [255, 0, 255, 1]]
    tr = common.odd_transform()
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g)
        m = v.models[SRC]
        pos, color, _, cov3d = _pod(v)
        vals = [m.property_values(p) for p in range(P.COUNT)]
        for k in range(3):  # the stored position bits
            _same(vals[k], pos[:, k], f"pos {k}")
        for k in range(4):  # the bytes of the stored colour word / 255
            _same(vals[P.RED + k], ((color >> np.uint32(8 * k)) & np.uint32(255)).astype(F) / F(255), f"colour byte {k}")
        for p in (P.HUE, P.SATURATION, P.VALUE):  # em_rgb_to_hsv on the same colour words (divisions only: no libm call differs)
            _same(vals[p], P.values_pc(p, pos, color), f"hsv {p}")
        out = m.export().gaussians  # the scales gsx_model_export writes for the same Gaussians
        for k in range(3):
            _same(vals[P.SCALE_MAX + k], out["scale"][:, k], f"scale {k}")
        assert (vals[P.SCALE_MIN][200:300] == 0).all() and (vals[P.SCALE_MAX][200:300] == 0).all()
        if cov == Cov3dKind.Half:
            assert np.isinf(cov3d[300:308, 0]).all() and np.isinf(vals[P.SCALE_MAX][300:308]).all()
            assert np.array_equal(vals[P.SCALE_MID][300:308], np.full(8, 2, F)) and np.array_equal(vals[P.SCALE_MIN][300:308], np.full(8, 0.5, F))
        # an identity transform: WORLD gives the stored bits (inf and NaN rows too)
        for k in range(3):
            _same(m.property_values(k, world=True), pos[:, k], f"identity world {k}")
        # a TRS: the positions gsx_model_merge bakes
        v.update_model_transform(SRC, tr.pos, tr.quat(), tr.scale)
        assert v.merge("baked", [SRC])[0] == n
        baked = _pod(v, "baked")[0]
        for k in range(3):
            got = m.property_values(k, world=True)
            _same(got, baked[:, k], f"world {k}")
            _same(m.property_values(k), pos[:, k], f"model space under a transform {k}")
        assert not np.array_equal(baked[:300], pos[:300])
        # the same bytes on every call
        _same(m.property_values(P.SCALE_MID), vals[P.SCALE_MID])
        _same(m.property_values(P.HUE), vals[P.HUE])


@pytest.mark.parametrize("n", SIZES)
def test_values_at_the_edges_of_the_frame(n):
    g = common.small_scene(n, 40 + n)
    with MultiModelViewer(sh=ShKind.Remove, cov3d=Cov3dKind.Half) as v:
        _load(v, g)
        m = v.models[SRC]
        pos, color, _, _ = _pod(v)
        out = m.export().gaussians
        for p in PC_PROPS:
            _same(m.property_values(p), P.values_pc(p, pos, color), (n, p))
        for k in range(3):
            _same(m.property_values(P.SCALE_MAX + k), out["scale"][:, k], (n, k))


# ---- 2. histogram ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_histogram_against_the_restatement(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 100 + n)
        _load(v, g, "bare")  # the same Gaussians without mask, selection and edit records
        for key, planes in ((SRC, (mask, sel, flags)), ("bare", (None, None, None))):
            m = v.models[key]
            for prop, lo, hi in ((P.POS_X, -0.75, 1.5), (P.OPACITY, 0.0, 1.0), (P.SCALE_MAX, 0.01, 0.2)):
                values = m.property_values(prop)
                for flt in range(8):
                    passes = _passes(n, flt, *planes)
                    for bins in P.BIN_COUNTS:
                        _check_hist(m.histogram(prop, bins, lo, hi, filter=flt), P.histogram(values, passes, bins, lo, hi), (key, prop, flt, bins, "explicit"))
                        _check_hist(m.histogram(prop, bins, filter=flt), P.histogram(values, passes, bins), (key, prop, flt, bins, "auto"))
        if n >= 64:
            h = v.models[SRC].histogram(P.POS_X, 16)
            assert h.n_nonfinite == 3 and h.count == n - 3 and np.isfinite([h.lo, h.hi, h.min, h.max]).all()  # (NaN, inf, -inf in x)
        # SELECTED of a model without a selection: none; zeros, the explicit range echoed
        h = v.models["bare"].histogram(P.POS_X, 4, -1.0, 1.0, filter=X.SELECTED)
        assert (h.count, h.below, h.above, h.n_nonfinite, h.lo, h.hi, h.min, h.max) == (0, 0, 0, 0, -1.0, 1.0, 0.0, 0.0) and not h.bins.any()
        h = v.models["bare"].histogram(P.POS_X, 4, filter=X.SELECTED)
        assert (h.count, h.lo, h.hi, h.min, h.max) == (0, 0.0, 0.0, 0.0, 0.0) and not h.bins.any()


@pytest.mark.parametrize("bins", P.BIN_COUNTS)
def test_histogram_of_planted_values(bins):
    """positions planted on every bin edge and one ulp either side of it; all values equal; a range of a few ulps; NaN and inf"""
    lo, hi = F(-2.0), F(6.0)
    r = P.Range(lo, hi, bins)
    edges = r.edge(np.arange(bins + 1))
    planted = np.concatenate([edges, [P.next_up(e, 1) for e in edges], [P.next_up(e, -1) for e in edges],
                              [np.nan, np.inf, -np.inf, -0.0, 0.0, 7.0, -3.0]]).astype(F)
    n = planted.size + 100
    g = common.small_scene(n, 3, 0)
    g["pos"][: planted.size, 0] = planted
    g["pos"][:, 1] = F(2.5)                                              # all values equal
    g["pos"][:, 2] = [P.next_up(F(1.0), k % 4) for k in range(n)]        # a range of three ulps
    with MultiModelViewer(sh=ShKind.Remove) as v:
        _load(v, g)
        m = v.models[SRC]
        every = np.ones(n, bool)
        x = m.property_values(P.POS_X)
        _same(x[: planted.size], planted)
        h = m.histogram(P.POS_X, bins, lo, hi)
        _check_hist(h, P.histogram(x, every, bins, lo, hi), "edges")
        assert h.n_nonfinite == 3 and h.below >= 2 and h.above >= 2
        _check_hist(m.histogram(P.POS_X, bins), P.histogram(x, every, bins), "edges, auto")
        y = m.histogram(P.POS_Y, bins)  # lo == hi: not live, everything in bin 0
        assert (y.count, y.below, y.above, int(y.bins[0]), y.lo, y.hi, y.min, y.max) == (n, 0, 0, n, 2.5, 2.5, 2.5, 2.5)
        _check_hist(y, P.histogram(m.property_values(P.POS_Y), every, bins), "equal")
        z = m.property_values(P.POS_Z)
        _check_hist(m.histogram(P.POS_Z, bins), P.histogram(z, every, bins), "few ulps, auto")
        _check_hist(m.histogram(P.POS_Z, bins, 1.0, float(P.next_up(F(1.0), 2))), P.histogram(z, every, bins, 1.0, P.next_up(F(1.0), 2)), "few ulps")
        _check_hist(m.histogram(P.POS_X, bins, 0.0, 1e-42), P.histogram(x, every, bins, 0.0, 1e-42), "a width that underflows")


# ---- 3. select ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_select_against_the_restatement(n):
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 200 + n)
        m = v.models[SRC]
        sb = m.gaussian_buffers.selection_buffer
        values = {p: m.property_values(p) for p in (P.POS_X, P.OPACITY, P.SCALE_MIN)}
        ranges = {P.POS_X: (-0.5, 0.75), P.OPACITY: (0.25, 1.0), P.SCALE_MIN: (0.0, 0.05)}
        for prior in ("random", None):
            for op in (P.SET, P.ADD, P.REMOVE):
                for flt in (0, X.SELECTED, X.MASKED | X.SKIP_HIDDEN, 7):
                    for prop, (lo, hi) in ranges.items():
                        sb.upload(X.words(sel, True) if prior else None)  # (garbage in the tail bits of the prior selection)
                        old = sel if prior else np.zeros(n, bool)
                        hit = P.hits(values[prop], _passes(n, flt, mask, sel if prior else None, flags), lo, hi)
                        want = P.apply_op(op, old, hit)
                        got = m.select_range(prop, lo, hi, op, flt)
                        assert got == (int(hit.sum()), int(want.sum())), (prior, op, flt, prop, got)
                        assert np.array_equal(sb.download(), P.words(want)), (prior, op, flt, prop)  # tail bits zero
        # SELECTED with Set narrows the selection
        sb.upload(X.words(sel))
        hit, selected = m.select_range(P.OPACITY, 0.5, 1.0, P.SET, X.SELECTED)
        narrowed = sel & (values[P.OPACITY] >= F(0.5))
        assert hit == selected == int(narrowed.sum()) and np.array_equal(sb.download(), P.words(narrowed))
        # the out pointers are optional
        desc = _lib.SelectDesc(P.OPACITY, 0, 0, P.SET, 0.0, 1.0, 0, 0, 0, 0)
        assert v._L.gsx_model_select_range(v._h, SRC.encode(), C.byref(desc), None, None) == _lib.GSX_OK
        assert np.array_equal(sb.download(), P.words(np.ones(n, bool)))


def test_select_by_bin_matches_the_histogram():
    n, bins = 5000, 16
    with MultiModelViewer(sh=ShKind.Remove) as v:
        g, mask, sel, flags = _filter_model(v, n, 31)
        m = v.models[SRC]
        sb = m.gaussian_buffers.selection_buffer
        for prop, flt in ((P.POS_X, 0), (P.OPACITY, X.MASKED | X.SKIP_HIDDEN), (P.SCALE_MAX, X.MASKED)):
            h = m.histogram(prop, bins, filter=flt)
            values = m.property_values(prop)
            union = np.zeros(n, bool)
            for b in range(bins):
                hit, selected = m.select_range(prop, h.lo, h.hi, P.SET, flt, bins=bins, bin_lo=b, bin_hi=b)
                assert hit == selected == int(h.bins[b]), (prop, b)
                one = P.unwords(sb.download(), n)
                assert not (union & one).any()
                union |= one
            in_range = P.hits(values, _passes(n, flt, mask, None, flags), h.lo, h.hi)
            assert np.array_equal(union, in_range) and int(union.sum()) == h.count  # auto range: nothing below or above
            hit, _ = m.select_range(prop, h.lo, h.hi, P.SET, flt, bins=bins, bin_lo=3, bin_hi=9)
            assert hit == int(h.bins[3:10].sum())


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------
def test_select_then_extract_and_frames():
    n = 2500
    g = common.small_scene(n, 37)
    x = 0.35
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _load(vv, g)
            vv.update_selection_edit_with_pod(query.GaussianEditPod(EF.ENABLED, alpha=0.6))
            vv.update_selection_highlight(HIGHLIGHT)
        m = v.models[SRC]
        plain = _frames(v, [SRC], poses=(4,))[0]
        assert np.array_equal(plain, _frames(twin, [SRC], poses=(4,))[0])
        opacity = m.property_values(P.OPACITY)
        low = opacity <= F(x)
        assert m.select_range(P.OPACITY, 0.0, x) == (int(low.sum()), int(low.sum())) and 0 < low.sum() < n
        words = m.gaussian_buffers.selection_buffer.download()
        assert np.array_equal(words, P.words(low))
        # the frames with the highlight on: those of a twin whose selection was uploaded from the host with the same words
        twin.models[SRC].gaussian_buffers.selection_buffer.upload(words)
        got, want = _frames(v, [SRC], poses=(4, 5, 6, 7)), _frames(twin, [SRC], poses=(4, 5, 6, 7))
        assert not np.array_equal(got[0], plain)  # (the selection shows)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        # "delete the near-transparent splats": what is left is what numpy predicts
        assert m.extract("kept", X.SELECTED, invert=True) == n - int(low.sum())
        _same(v.models["kept"].property_values(P.OPACITY), opacity[~low])


def _lane_sequence(g, lanes, on_device):
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
            m.select_range(P.HUE, 0.0, 0.5)  # behind the frames in flight on the lanes
        else:
            hue = P.values_pc(P.HUE, *_pod(v)[:2])
            m.gaussian_buffers.selection_buffer.upload(P.words(hue <= F(0.5)))
        for pose in (5, 6, 7, 8):
            out += _frames(v, [SRC], poses=(pose,))
    return out


def test_lanes():
    g = common.small_scene(2500, 38)
    two, one, host = _lane_sequence(g, 2, True), _lane_sequence(g, 1, True), _lane_sequence(g, 2, False)
    assert len(two) == 8 and two[0][..., :3].max() > 0
    for k, (a, b, c) in enumerate(zip(two, one, host)):
        assert np.array_equal(a, b) and np.array_equal(a, c), k


# ---- 5. the read-only calls -------------------------------------------------------------------------------------------------------------
def test_values_and_histogram_write_nothing():
    n = 3000
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _filter_model(vv, n, 51)
        m = v.models[SRC]

        def state(vv):
            bufs = vv.models[SRC].gaussian_buffers
            return [a.tobytes() for a in _pod(vv)] + [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(),
                                                      bufs.gaussians_edit_buffer.download().tobytes()]

        before = state(v)
        assert np.array_equal(_frames(v, [SRC], poses=(5,))[0], _frames(twin, [SRC], poses=(5,))[0])
        m.property_values(P.SCALE_MAX)  # (the first calls size the shared workspace)
        m.histogram(P.POS_X, 4096)
        held = viewer_mod.device_bytes()
        for prop in (P.POS_Y, P.HUE, P.SCALE_MIN):
            m.property_values(prop, world=prop < 3)
            m.histogram(prop, 255, filter=7)
            m.histogram(prop, 4096, 0.0, 1.0)
        assert viewer_mod.device_bytes() == held
        assert state(v) == before == state(twin)
        for a, b in zip(_frames(v, [SRC], poses=(6, 7)), _frames(twin, [SRC], poses=(6, 7))):
            assert np.array_equal(a, b)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors():
    n = 300
    with MultiModelViewer() as v, MultiModelViewer() as other:
        g, mask, sel, flags = _filter_model(v, n, 61)
        L, key = v._L, SRC.encode()
        sb = v.models[SRC].gaussian_buffers.selection_buffer
        sel_before = sb.download()
        out, bins, hist = np.zeros(n, F), (C.c_uint64 * 4096)(), _lib.Histogram()
        hit, selected = C.c_uint64(), C.c_uint64()
        INV, NF, UNS = _lib.GSX_ERR_INVALID_ARG, _lib.GSX_ERR_NOT_FOUND, _lib.GSX_ERR_UNSUPPORTED

        def values(k=key, prop=0, flags_=0, o=out.ctypes.data, count=n, vv=v):
            return L.gsx_model_property_values(vv._h if vv else None, k, prop, flags_, o, count)

        def histogram(k=key, prop=0, flags_=0, flt=0, nb=4, lo=0.0, hi=1.0, desc=True, b=bins, h=hist, vv=v):
            d = _lib.HistogramDesc(prop, flags_, flt, nb, lo, hi)
            return L.gsx_model_histogram(vv._h if vv else None, k, C.byref(d) if desc else None, b, C.byref(h) if h is not None else None)

        def select(k=key, prop=0, flags_=0, flt=0, op=0, lo=0.0, hi=1.0, nb=0, b0=0, b1=0, reserved=0, desc=True, vv=v):
            d = _lib.SelectDesc(prop, flags_, flt, op, lo, hi, nb, b0, b1, reserved)
            return L.gsx_model_select_range(vv._h if vv else None, k, C.byref(d) if desc else None, C.byref(hit), C.byref(selected))

        cases = [
            (values(vv=None), INV), (values(k=None), INV), (values(o=None), INV), (values(prop=13), INV), (values(flags_=2), INV),
            (values(flags_=4), INV), (values(prop=P.RED, flags_=1), INV), (values(prop=P.SCALE_MAX, flags_=1), INV), (values(count=n - 1), INV),
            (values(k=b"nope"), NF),
            (histogram(vv=None), INV), (histogram(k=None), INV), (histogram(desc=False), INV), (histogram(b=None), INV), (histogram(h=None), INV),
            (histogram(prop=13), INV), (histogram(flags_=2), INV), (histogram(flags_=8), INV), (histogram(prop=P.HUE, flags_=1), INV),
            (histogram(flt=8), INV), (histogram(nb=0), INV), (histogram(nb=4097), INV), (histogram(lo=1.0, hi=0.0), INV),
            (histogram(lo=float("nan")), INV), (histogram(hi=float("inf")), INV), (histogram(k=b"nope"), NF),
            (select(vv=None), INV), (select(k=None), INV), (select(desc=False), INV), (select(prop=13), INV), (select(flags_=2), INV),
            (select(flags_=4), INV),  # AUTO_RANGE is not legal here
            (select(prop=P.OPACITY, flags_=1), INV), (select(flt=8), INV), (select(op=3), INV), (select(reserved=1), INV),
            (select(nb=4097), INV), (select(nb=16, b0=5, b1=4), INV), (select(nb=16, b0=0, b1=16), INV), (select(lo=1.0, hi=0.0), INV),
            (select(lo=float("-inf")), INV), (select(hi=float("nan")), INV), (select(k=b"nope"), NF),
        ]
        for i, (got, want) in enumerate(cases):
            assert got == want, i
        assert b"gsx_model_select_range" in L.gsx_last_error_string()
        assert np.array_equal(sb.download(), sel_before)  # a refused select leaves the selection
        # a non-finite range is fine with AUTO_RANGE (lo / hi are ignored)
        assert histogram(prop=P.OPACITY, flags_=4, lo=float("nan"), hi=float("nan")) == _lib.GSX_OK and hist.count == n
        # an empty model: GSX_OK with zeros
        v.add_model("empty", 0)
        e = v.models["empty"]
        assert e.property_values(P.POS_X).size == 0
        h = e.histogram(P.POS_X, 8)
        assert (h.count, h.n_nonfinite, h.lo, h.hi) == (0, 0, 0.0, 0.0) and not h.bins.any()
        assert e.select_range(P.POS_X, 0.0, 1.0) == (0, 0)
        # a sharded model; a viewer with a communicator
        _frames(v, [SRC], poses=(5,))
        _load(v, g[:50], "b")
        v.shard_set_limits("b", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        _load(other, g[:50], "a")
        other.comm_init_group(CommGroup(1), 0)
        for model, word in ((v.models["b"], "shard"), (other.models["a"], "communicator")):
            for call in (lambda: model.property_values(P.POS_X), lambda: model.histogram(P.POS_X, 4), lambda: model.select_range(P.POS_X, 0.0, 1.0)):
                with pytest.raises(GsxError) as err:
                    call()
                assert err.value.status == UNS and word in str(err.value)


# ---- 7. repeatability -------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes():
    n = 5000
    with MultiModelViewer(sh=ShKind.Norm8, cov3d=Cov3dKind.Half) as v:
        _filter_model(v, n, 71)
        m = v.models[SRC]
        for prop in (P.POS_Z, P.SATURATION, P.SCALE_MID):
            assert m.property_values(prop).tobytes() == m.property_values(prop).tobytes()
            for bins in (2, 4096):
                a, b = m.histogram(prop, bins, filter=3), m.histogram(prop, bins, filter=3)
                assert a.bins.tobytes() == b.bins.tobytes() and (a.count, a.below, a.above, a.n_nonfinite) == (b.count, b.below, b.above, b.n_nonfinite)
                assert _bits([a.lo, a.hi, a.min, a.max]).tobytes() == _bits([b.lo, b.hi, b.min, b.max]).tobytes()
            first = m.select_range(prop, 0.0, 0.5, P.SET, 3)
            words = m.gaussian_buffers.selection_buffer.download()
            assert m.select_range(prop, 0.0, 0.5, P.SET, 3) == first and np.array_equal(m.gaussian_buffers.selection_buffer.download(), words)


# ---- 8. a workgroup that takes more than one chunk ----------------------------------------------------------------------------------------
def test_more_chunks_than_workgroups():
    """2048 workgroups at most (1024 in the histogram): past 2048 x 1024 Gaussians a workgroup strides over several chunks.  The planes
    are staged on the device (no 224-byte records on the host)."""
    import torch

    n = 2048 * 1024 + 1025
    rng = np.random.default_rng(9)
    pos = rng.standard_normal((n, 3)).astype(F)
    pos[[0, n // 2, n - 1], 0] = [np.nan, np.inf, -np.inf]
    color = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    s = (rng.random((n, 3)).astype(F) * F(0.1)) ** 2
    cov = np.zeros((n, 6), F)
    cov[:, 0], cov[:, 3], cov[:, 5] = s[:, 0], s[:, 1], s[:, 2]  # axis-aligned: the scales are the roots of the diagonal
    mask = rng.random(n) < 0.5
    with MultiModelViewer(sh=ShKind.Remove) as v:
        v.add_model(SRC, n)
        m = v.models[SRC]
        dev = [torch.from_numpy(a).cuda() for a in (pos, color.view(np.int32), cov)]
        torch.cuda.synchronize()
        m.gaussian_buffers.gaussians_buffer.update_range_pod_device(0, n, dev[0].data_ptr(), dev[1].data_ptr(), None, dev[2].data_ptr())
        v.poll()
        m.gaussian_buffers.mask_buffer.upload(X.words(mask, True))
        x, opacity, smax = m.property_values(P.POS_X), m.property_values(P.OPACITY), m.property_values(P.SCALE_MAX)
        _same(x, pos[:, 0])
        _same(opacity, (color >> np.uint32(24)).astype(F) / F(255))
        _same(smax, np.sqrt(s.max(axis=1)))
        for values, prop, bins in ((x, P.POS_X, 4096), (opacity, P.OPACITY, 256), (smax, P.SCALE_MAX, 255)):
            _check_hist(m.histogram(prop, bins, filter=X.MASKED), P.histogram(values, mask, bins), (prop, "auto"))
        _check_hist(m.histogram(P.POS_X, 16, -1.0, 1.0), P.histogram(x, np.ones(n, bool), 16, -1.0, 1.0), "explicit")
        hit = P.hits(x, mask, -0.25, 0.5)
        assert m.select_range(P.POS_X, -0.25, 0.5, P.SET, X.MASKED) == (int(hit.sum()), int(hit.sum()))
        assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), P.words(hit))
        hit2 = P.hits(smax, np.ones(n, bool), 0.05, 1.0)
        want = hit | hit2
        assert m.select_range(P.SCALE_MAX, 0.05, 1.0, P.ADD) == (int(hit2.sum()), int(want.sum()))
        assert np.array_equal(m.gaussian_buffers.selection_buffer.download(), P.words(want))
        assert _len(v, SRC) == (_lib.GSX_OK, n)
