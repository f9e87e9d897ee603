"""CPU: the query predicates of spec §7 — rect, brush, texture, hit — in the float32 C oracle (oracle.query_flags / query_hits, the
operation order of the kernels) against their float64 statement (oracle/spec_f64.py query_flags / query_hits, written from the
sentences of the spec).  The two must agree on every Gaussian that is not within float32 rounding of a cut (`ambiguous`), those must
be few, and the tolerance that defines them is measured here, not chosen."""
import numpy as np
import pytest

import oracle
from oracle import spec_f64
from tests import common, query_cases as qc
from wgpu_3dgs_viewer_app_amd import camera, query

W, H = qc.W, qc.H
SCENES = {"identity": (40000, 31, None), "odd": (40000, 32, "odd")}
_cache = {}


def _scene(name):
    """(frame, f32 projection, f64 projection) — computed once, never modified."""
    if name not in _cache:
        n, seed, mt = SCENES[name]
        g = common.small_scene(n, seed, scale_mul=8.0)
        _cache[name] = qc.project_both(g, camera.orbit_pose(qc.POSE), W, H, common.odd_transform() if mt else None)
    return _cache[name]


def _visible(pr):
    return pr["key"] != 0xFFFFFFFF


def test_tolerances_cover_the_f32_projection():
    """QUERY_TOL, QUERY_TOL_Q, QUERY_TOL_ALPHA are 8 x the largest f32-against-f64 difference over every scene the query tests project."""
    worst = np.zeros(3)
    for s in qc.tolerance_scenes():
        worst = np.maximum(worst, qc.measure_scene(s))
    print(f"largest |mean2d| {worst[0]:.3g} px, |q| / k^2 {worst[1]:.3g}, |alpha| {worst[2]:.3g}")
    for name, measured, tol in (("QUERY_TOL", worst[0], spec_f64.QUERY_TOL), ("QUERY_TOL_Q", worst[1], spec_f64.QUERY_TOL_Q),
                                ("QUERY_TOL_ALPHA", worst[2], spec_f64.QUERY_TOL_ALPHA)):
        # (the measurement moves a little with the libm and the compiler of the oracle build: the factor must hold, the constant
        #  must not have drifted to another order of magnitude)
        assert 8.0 * measured <= tol <= 32.0 * measured, f"{name} = {tol} is not 8 x the measured {measured:.3g}"


@pytest.mark.parametrize("kind", ["rect", "brush", "disc", "texture"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_c_oracle_flags_equal_the_f64_flags(scene, kind):
    f, pr, p64 = _scene(scene)
    pod, tex = qc.selection_queries()[kind]
    assert np.array_equal(_visible(pr), p64["visible"]), "the two cull sets differ: the scene has a Gaussian on a cull boundary"
    n = pr["key"].shape[0]
    got = qc.unpack_bits(oracle.query_flags(pr, pod, tex), n)
    want, amb = spec_f64.query_flags(p64, pod, tex)
    nvis = int(p64["visible"].sum())
    print(f"{scene}/{kind}: {int(want.sum())} flagged of {nvis} visible, {int(amb.sum())} ambiguous at {spec_f64.QUERY_TOL} px")
    assert want.sum() > 100 and (p64["visible"] & ~want).sum() > 100, "the query must split the visible Gaussians"
    bad = np.nonzero((got != want) & ~amb)[0]
    assert bad.size == 0, f"{bad.size} flags differ away from every cut, first {bad[:5]}: means {p64['mean2d'][bad[:5]]}"
    assert amb.sum() <= 0.01 * nvis, f"{int(amb.sum())} of {nvis} visible Gaussians are ambiguous"
    assert not (amb & ~p64["visible"]).any() and not (want & ~p64["visible"]).any()


@pytest.mark.parametrize("scene", list(SCENES))
def test_ambiguous_set_grows_with_the_tolerance_and_holds_the_edges(scene):
    """`ambiguous` means what it says: at 1e-3 px it contains the set at QUERY_TOL; a mean put ON a cut is in it."""
    _, _, p64 = _scene(scene)
    for kind, (pod, tex) in qc.selection_queries().items():
        _, a0 = spec_f64.query_flags(p64, pod, tex)
        _, a1 = spec_f64.query_flags(p64, pod, tex, tol=1e-3)
        assert not (a0 & ~a1).any(), kind
        assert a1.sum() <= 0.01 * p64["visible"].sum(), kind
    on = dict(visible=np.ones(6, bool), mean2d=np.array([[20.5, 50.0], [70.0, 90.0], [60.0, 85.0], [60.0, 85.0 + 1e-6], [33.0, 7.5], [33.0 - 1e-6, 7.5]]))
    tex = np.zeros((H, W), np.uint8)
    tex[7, 33] = 1
    qs = qc.selection_queries()
    assert spec_f64.query_flags(on, qs["rect"][0])[1].tolist() == [True, True, False, False, False, False]
    assert spec_f64.query_flags(on, qs["disc"][0])[1].tolist() == [False, False, True, True, False, False]
    assert spec_f64.query_flags(on, qs["disc"][0])[0].tolist() == [False, False, True, False, False, False]
    assert spec_f64.query_flags(on, qs["texture"][0], tex)[1].tolist() == [False, False, False, False, True, True]
    assert spec_f64.query_flags(on, qs["texture"][0], tex)[0].tolist() == [False, False, False, False, True, False]


@pytest.mark.parametrize("coords", qc.HIT_COORDS)
@pytest.mark.parametrize("scene", list(SCENES))
def test_c_oracle_hits_equal_the_f64_hits(scene, coords):
    f, pr, p64 = _scene(scene)
    hits, total = oracle.query_hits(f, pr, coords, with_count=True)
    idx, depth, alpha, amb = spec_f64.query_hits(p64, coords)
    print(f"{scene} {coords}: {hits.size} hits (f64 {idx.size}), {int(amb.sum())} ambiguous")
    assert total == hits.size > 100
    differ = np.setxor1d(hits["index"], idx)
    assert amb[differ].all(), f"hit sets differ away from the cuts: {differ[~amb[differ]][:8]}"
    assert amb.sum() <= max(4, 0.01 * idx.size), f"{int(amb.sum())} ambiguous of {idx.size} hits"
    both, ia, ib = np.intersect1d(hits["index"], idx, return_indices=True)
    np.testing.assert_allclose(hits["depth"][ia], depth[ib], rtol=1e-5)
    np.testing.assert_allclose(hits["alpha"][ia], alpha[ib], rtol=0, atol=spec_f64.QUERY_TOL_ALPHA / 8)
    # sorted by (depth, index) on both sides
    assert np.array_equal(np.lexsort((hits["index"], hits["depth"])), np.arange(hits.size))
    assert np.array_equal(np.lexsort((idx, depth.astype(np.float32))), np.arange(idx.size))


def test_hit_capacity_saturates_and_the_count_does_not():
    f, pr, _ = _scene("identity")
    full, total = oracle.query_hits(f, pr, (88.0, 64.0), with_count=True)
    kept, total2 = oracle.query_hits(f, pr, (88.0, 64.0), capacity=50, with_count=True)
    assert total2 == total == full.size > 50 and kept.size == 50
    assert np.isin(kept["index"], full["index"]).all() and np.array_equal(np.lexsort((kept["index"], kept["depth"])), np.arange(50))
    assert np.array_equal(oracle.query_hits(f, pr, (88.0, 64.0)), full), "the default call still returns the hits alone"


def _both_flags(scene, pod, tex=None):
    _, pr, p64 = _scene(scene)
    got = qc.unpack_bits(oracle.query_flags(pr, pod, tex), pr["key"].shape[0])
    want, amb = spec_f64.query_flags(p64, pod, tex)
    assert np.array_equal(got[~amb], want[~amb])
    return got, want, amb, p64


@pytest.mark.parametrize("scene", list(SCENES))
def test_degenerate_queries(scene):
    Op = query.QuerySelectionOp
    # a rectangle given by its other two corners, or with both corners swapped, is the same rectangle
    ref, _, _, _ = _both_flags(scene, query.QueryPod.rect((20.5, 10.25), (120.0, 90.0), Op.Set))
    for p0, p1 in (((120.0, 90.0), (20.5, 10.25)), ((120.0, 10.25), (20.5, 90.0))):
        got, want, amb, _ = _both_flags(scene, query.QueryPod.rect(p0, p1, Op.Set))
        assert np.array_equal(got, ref) and want.sum() > 100
    # radius 0: a segment or a point has no area
    for p1 in ((150.0, 100.0), (30.0, 30.0)):
        got, want, amb, _ = _both_flags(scene, query.QueryPod.brush((30.0, 30.0), p1, 0.0, Op.Set))
        assert not got.any() and not want.any()
    # a brush stroke entirely outside the viewport (and outside the cull margin around it)
    got, want, amb, _ = _both_flags(scene, query.QueryPod.brush((-300.0, -300.0), (-200.0, -250.0), 20.0, Op.Set))
    assert not got.any() and not want.any() and not amb.any()
    # a texture that is non-zero only in its last row and last column
    tex = np.zeros((H, W), np.uint8)
    tex[H - 1, :] = 1
    tex[:, W - 1] = 255
    got, want, amb, p64 = _both_flags(scene, query.QueryPod.texture(Op.Set), tex)
    m = p64["mean2d"][got]
    assert got.sum() > 20 and ((np.floor(m[:, 0]) == W - 1) | (np.floor(m[:, 1]) == H - 1)).all()
    assert (m[:, 0] < W).all() and (m[:, 1] < H).all() and (m >= 0).all()
    # no texture: nothing
    assert not oracle.query_flags(_scene(scene)[1], query.QueryPod.texture(Op.Set), None).any()
    assert not spec_f64.query_flags(_scene(scene)[2], query.QueryPod.texture(Op.Set), None)[0].any()


def test_mean_on_the_viewport_border_is_outside_the_texture():
    """Texel floor(mu): x = W and y = H name no texel; the last texel ends just below them; -0.0 is texel 0, anything below is outside."""
    means = np.array([[W, 10.5], [np.nextafter(np.float32(W), np.float32(0)), 10.5], [10.5, H], [10.5, np.nextafter(np.float32(H), np.float32(0))],
                      [-0.0, 0.0], [-1e-3, 5.0], [5.0, -1e-3], [W + 20.0, H + 20.0]], np.float32)
    n = means.shape[0]
    pr = dict(key=np.full(n, 0x40000000, np.uint32), mean2d=means)
    p64 = dict(visible=np.ones(n, bool), mean2d=means.astype(np.float64))
    tex = np.full((H, W), 255, np.uint8)
    pod = query.QueryPod.texture()
    want = [False, True, False, True, True, False, False, False]
    assert qc.unpack_bits(oracle.query_flags(pr, pod, tex), n).tolist() == want
    flags, amb = spec_f64.query_flags(p64, pod, tex)
    assert flags.tolist() == want
    assert amb.tolist() == [True, True, True, True, True, False, False, False], "the border under a non-zero texel is a cut"
    # a culled Gaussian is never flagged, whatever its record holds
    pr["key"][1] = 0xFFFFFFFF
    p64["visible"][1] = False
    assert not qc.unpack_bits(oracle.query_flags(pr, pod, tex), n)[1] and not spec_f64.query_flags(p64, pod, tex)[0][1]


@pytest.mark.parametrize("coords", [(float("nan"), 64.0), (88.0, float("nan")), (float("nan"), float("nan")), (-500.0, -500.0)])
def test_hit_coordinates_that_hit_nothing(coords):
    f, pr, p64 = _scene("identity")
    hits, total = oracle.query_hits(f, pr, coords, with_count=True)
    idx, depth, alpha, amb = spec_f64.query_hits(p64, coords)
    assert hits.size == 0 and total == 0 and idx.size == 0 and not amb.any()
