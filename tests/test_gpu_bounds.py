"""GPU: gsx_model_bounds (spec/RENDER_SPEC.md §11; csrc/kernels_bounds.hip) against numpy on the host arrays that were uploaded.
count / min / max / center are exact, the mean is one float32 rounding of the float64 mean, two calls return the same 88 bytes; the
three filters against the downloaded mask, selection and edits; non-finite positions; the trimmed box against the bounds any
trimmed box has to meet (tests/bounds_ref.py); frames are untouched by a call, with one lane and with two; the error statuses."""
import ctypes as C

import numpy as np
import pytest

from tests import bounds_ref as B
from tests import common
from wgpu_3dgs_viewer_app_amd import _lib, camera, query, scene
from wgpu_3dgs_viewer_app_amd import viewer as viewer_mod
from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as F
from wgpu_3dgs_viewer_app_amd.viewer import GaussianDisplayMode, GaussianShDegree, GsxError, MultiModelViewer

pytestmark = pytest.mark.gpu
KEY = "m"
W, H = 176, 128
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4097, 200003]  # lane, wave, workgroup and multi-workgroup tails; the cross-workgroup combine
FLOATS = ("min", "max", "center", "mean", "trim_min", "trim_max")


@pytest.fixture(scope="module")
def big():
    """One scene of 200003 Gaussians; the smaller models are its prefixes.  Never written to."""
    g = scene.synthetic_gaussians(SIZES[-1], 77, 0)
    g.setflags(write=False)
    return g


def _load(v, g, key=KEY):
    v.add_model(key, g.shape[0])
    v.models[key].gaussian_buffers.gaussians_buffer.update_range(0, g)


def _raw(v, key=KEY, flt=0, trim=0) -> bytes:
    """the 88 bytes of one call"""
    desc, out = _lib.BoundsDesc(flt, trim), _lib.ModelBounds()
    _lib.check(v._L.gsx_model_bounds(v._h, key.encode(), C.byref(desc), C.byref(out)))
    return bytes(out)


def _same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def _check_exact(b, ref, what=""):
    """count, n_nonfinite, min, max, center: numpy's, bit for bit; mean: within one float32 rounding of the float64 mean"""
    assert (b.count, b.n_nonfinite) == (ref["count"], ref["n_nonfinite"]), what
    for name in ("min", "max", "center"):
        assert _same_bits(getattr(b, name), ref[name]), (what, name, getattr(b, name), ref[name])
    if ref["count"] == 0:
        assert all(not getattr(b, name).any() for name in FLOATS), what
        return
    tol = 2.0 ** -23 * np.abs(ref["counted"].astype(np.float64)).max(axis=0)
    err = np.abs(b.mean.astype(np.float64) - ref["mean64"])
    print(f"{what} mean error / bound per axis: {err / tol}")
    assert np.all(err <= tol), (what, err, tol)


@pytest.mark.parametrize("n", SIZES)
def test_exact_fields_mean_and_determinism(big, n):
    g = big[:n]
    with MultiModelViewer() as v:
        _load(v, g)
        b = v.models[KEY].bounds()
        _check_exact(b, B.reference(g["pos"], np.ones(n, bool)), f"n={n}")
        assert b.n_nonfinite == 0 and b.count == n
        assert _same_bits(b.trim_min, b.min) and _same_bits(b.trim_max, b.max)
        first = _raw(v)
        assert len(first) == 88 and first == _raw(v), "two calls on the same model return the same 88 bytes"
        assert np.frombuffer(first, np.float32, 3, 16).tobytes() == b.min.tobytes()


def _filter_scene(v, g):
    """mask, selection and stored edits on the model, as the app makes them; returns the three as downloaded (bool[n] each: kept,
    selected, hidden)"""
    n = g.shape[0]
    c5 = common.cfg5_scene()
    tr = c5["tr"]["a"]
    bufs = v.models[KEY].gaussian_buffers
    v.update_model_transform(KEY, tr.pos, tr.quat(), tr.scale)
    v.update_camera(camera.orbit_pose(12), (W, H))
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(0), False)
    # a rectangle selection made on the device
    v.update_query(query.QueryPod.rect((20.0, 15.0), (150.0, 110.0), query.QuerySelectionOp.Set))
    v.preprocessor.preprocess(KEY)
    v.postprocessor.postprocess(KEY)
    v.update_query(query.QueryPod.none())
    # stored edits: ENABLED | HIDDEN on every third Gaussian, ENABLED alone on the ones after them
    edits = query.default_edits(n)
    edits["flag"][0::3] = int(F.ENABLED | F.HIDDEN)
    edits["flag"][1::3] = int(F.ENABLED)
    edits["flag"][5::7] |= int(F.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    bufs.gaussians_edit_buffer.upload(edits)
    # the `0 - 1` mask of cfg5 (box minus ellipsoid), evaluated on the device
    MaskEvaluator(v).evaluate(c5["mask_op"], KEY, c5["mask_shapes"])
    kept = B.bits(bufs.mask_buffer.download(), n)
    selected = B.bits(bufs.selection_buffer.download(), n)
    flag = bufs.gaussians_edit_buffer.download()["flag"]
    hidden = ((flag & int(F.ENABLED)) != 0) & ((flag & int(F.HIDDEN)) != 0)
    assert 0 < kept.sum() < n and 0 < selected.sum() < n and 0 < hidden.sum() < n, "every filter must drop something and keep something"
    return kept, selected, hidden


@pytest.mark.parametrize("n", [4097, 200003])
def test_filters(big, n):
    g = big[:n]
    everything = B.reference(g["pos"], np.ones(n, bool))
    with MultiModelViewer() as v:
        _load(v, g)
        m = v.models[KEY]
        # absent buffers: no selection = none, no mask = all, no edits = all
        empty = m.bounds(selected=True)
        assert (empty.count, empty.n_nonfinite) == (0, 0) and all(not getattr(empty, name).any() for name in FLOATS)
        assert _raw(v, flt=B.SELECTED)[16:] == bytes(72)  # every float field 0.0f
        _check_exact(m.bounds(masked=True), everything, "no mask")
        _check_exact(m.bounds(skip_hidden=True), everything, "no edits")
        kept, selected, hidden = _filter_scene(v, g)
        cases = {"masked": kept, "skip_hidden": ~hidden, "selected": selected}
        for name, keep in cases.items():
            _check_exact(m.bounds(**{name: True}), B.reference(g["pos"], keep), name)
        both = kept & ~hidden & selected
        assert both.any()
        _check_exact(m.bounds(masked=True, skip_hidden=True, selected=True), B.reference(g["pos"], both), "all three")
        _check_exact(m.bounds(), everything, "no filter")
        # the stored buffers are read as they are: showing the model unedited changes nothing
        before = [_raw(v, flt=f) for f in range(8)]
        v.show_unedited(KEY, True)
        assert [_raw(v, flt=f) for f in range(8)] == before
        v.show_unedited(KEY, False)
        # an uploaded mask whose last word has garbage above n: indices >= n never count
        rng = np.random.default_rng(n)
        words = rng.integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
        assert n % 32 != 0
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
        m.gaussian_buffers.mask_buffer.upload(words)
        _check_exact(m.bounds(masked=True), B.reference(g["pos"], B.bits(words, n)), "uploaded mask, garbage tail")
        words[:] = 0
        words[-1] = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # nothing below n is kept
        m.gaussian_buffers.mask_buffer.upload(words)
        assert m.bounds(masked=True).count == 0 and _raw(v, flt=B.MASKED)[16:] == bytes(72)


def test_non_finite_positions_are_counted_apart(big):
    n = 4097
    g = big[:n].copy()
    g["pos"][10, 0], g["pos"][2000, 1], g["pos"][4000, 2] = np.nan, np.inf, -np.inf
    keep = np.random.default_rng(5).random(n) < 0.7
    keep[[10, 4000]], keep[2000] = True, False  # the mask filters one of the three out
    words = np.zeros((n + 31) // 32, np.uint32)
    np.bitwise_or.at(words, np.nonzero(keep)[0] >> 5, np.uint32(1) << (np.nonzero(keep)[0] & 31).astype(np.uint32))
    with MultiModelViewer() as v:
        _load(v, g)
        v.models[KEY].gaussian_buffers.mask_buffer.upload(words)
        every, masked = v.models[KEY].bounds(), v.models[KEY].bounds(masked=True, trim_permille=20)
        assert (every.n_nonfinite, every.count) == (3, n - 3) and (masked.n_nonfinite, masked.count) == (2, int(keep.sum()) - 2)
        _check_exact(every, B.reference(g["pos"], np.ones(n, bool)), "non-finite")
        _check_exact(masked, B.reference(g["pos"], keep), "non-finite, masked")
        assert np.isfinite(masked.trim_min).all() and np.isfinite(masked.trim_max).all()


def _with_outliers(g, seed):
    """1 % of the positions multiplied by 50 (seeded choice): floaters"""
    g = g.copy()
    far = np.random.default_rng(seed).choice(g.shape[0], g.shape[0] // 100, replace=False)
    g["pos"][far] *= np.float32(50.0)
    return g


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("n", [4097, 200003])
def test_trimmed_box(big, n, masked):
    g = _with_outliers(big[:n], 1000 + n)
    keep = np.random.default_rng(n + 1).random(n) < 0.7 if masked else np.ones(n, bool)
    with MultiModelViewer() as v:
        _load(v, g)
        if masked:
            words = np.zeros((n + 31) // 32, np.uint32)
            np.bitwise_or.at(words, np.nonzero(keep)[0] >> 5, np.uint32(1) << (np.nonzero(keep)[0] & 31).astype(np.uint32))
            v.models[KEY].gaussian_buffers.mask_buffer.upload(words)
        ref = B.reference(g["pos"], keep)
        for trim in (0, 1, 20, 499):
            b = v.models[KEY].bounds(masked=masked, trim_permille=trim)
            _check_exact(b, ref, f"trim {trim}")
            k = B.trim_k(ref["count"], trim)
            for axis in range(3):
                values = ref["counted"][:, axis]
                (min_lo, min_hi), (max_lo, max_hi) = B.trim_limits(values, k)
                # the one-level 2048-bin method restated in numpy stays inside the limits: a failure below is the kernel's, not the inputs'
                r_min, r_max = B.trimmed_axis(values, k)
                assert min_lo <= r_min <= min_hi and max_lo <= r_max <= max_hi, (trim, axis)
                print(f"n={n} trim={trim} axis={axis}: trim_min {b.trim_min[axis]!r} in [{min_lo!r}, {min_hi!r}] (restated {r_min!r}); "
                      f"trim_max {b.trim_max[axis]!r} in [{max_lo!r}, {max_hi!r}] (restated {r_max!r})")
                assert min_lo <= b.trim_min[axis] <= min_hi and max_lo <= b.trim_max[axis] <= max_hi, (trim, axis)
                assert (values < b.trim_min[axis]).sum() <= k and (values > b.trim_max[axis]).sum() <= k, (trim, axis)
            if trim == 0:
                assert _same_bits(b.trim_min, b.min) and _same_bits(b.trim_max, b.max)
            if trim == 20:  # the floaters are outside, the body is inside
                assert np.all(b.trim_max - b.trim_min < 0.1 * (b.max - b.min))
        assert _raw(v, flt=B.MASKED if masked else 0, trim=20) == _raw(v, flt=B.MASKED if masked else 0, trim=20)


def test_a_model_of_one_point_returns_that_point(big):
    g = big[:65].copy()
    g["pos"][:] = np.float32([1.5, -2.25, 1000.0])
    with MultiModelViewer() as v:
        _load(v, g)
        b = v.models[KEY].bounds(trim_permille=20)
        assert b.count == 65 and all(_same_bits(getattr(b, name), g["pos"][0]) for name in FLOATS)


def _frame(v, pose):
    v.update_camera(camera.orbit_pose(pose), (W, H))
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
    v.render_frame([KEY])


def _two_frames(g, call_bounds, lanes=1):
    """the same pose twice; returns the two frames, the launches of the second and its launch statistics"""
    with MultiModelViewer() as v:
        v.set_render_options(frames_in_flight=lanes)
        _load(v, g)
        sel = np.zeros((g.shape[0] + 31) // 32, np.uint32)
        sel[::2] = 0x0F0F0F0F
        v.models[KEY].gaussian_buffers.selection_buffer.upload(sel)
        v.models[KEY].gaussian_buffers.mask_buffer.upload(~sel)
        _frame(v, 33)
        first = v.download_framebuffer() if lanes == 1 else None  # (with two lanes the call below is what comes between the two frames)
        if call_bounds:
            b = v.models[KEY].bounds(masked=True, skip_hidden=True, selected=True, trim_permille=20)
            assert b.count == 0  # mask = ~selection
            assert v.models[KEY].bounds(selected=True, trim_permille=20).count > 0
        v.launch_stats(reset=True)
        n0 = viewer_mod.launch_count()
        _frame(v, 33)
        n1 = viewer_mod.launch_count()
        second = v.download_framebuffer()
        if lanes > 1:  # the frame that was in flight during the call: lane 0 still holds it
            first = v.debug_download_lane_framebuffer(0)
        return first, second, n1 - n0, v.launch_stats()


def test_frames_are_untouched():
    g = common.small_scene(6000, 31)
    first, second, launches, stats = _two_frames(g, True)
    ref_first, ref_second, ref_launches, ref_stats = _two_frames(g, False)
    assert np.array_equal(first, ref_first) and np.array_equal(second, ref_second) and np.array_equal(first, second)
    assert launches == ref_launches and stats == ref_stats and stats["broken"] == 0
    # two frames in flight, the call between two gsx_render_frame calls: the frames equal the one-lane frames
    lane_first, lane_second, _, _ = _two_frames(g, True, lanes=2)
    assert np.array_equal(lane_first, ref_first) and np.array_equal(lane_second, ref_second)


def test_errors_have_a_status_and_a_message(big):
    with MultiModelViewer() as v:
        _load(v, big[:64])
        for kw, key, status in ((dict(flt=0), "nope", _lib.GSX_ERR_NOT_FOUND), (dict(flt=8), KEY, _lib.GSX_ERR_INVALID_ARG),
                                (dict(trim=500), KEY, _lib.GSX_ERR_INVALID_ARG)):
            with pytest.raises(GsxError) as e:
                _raw(v, key, **kw)
            assert e.value.status == status and "gsx_model_bounds" in str(e.value)
        with pytest.raises(GsxError):
            v.models[KEY].bounds(trim_permille=500)
        assert v.models[KEY].bounds(trim_permille=499).count == 64
