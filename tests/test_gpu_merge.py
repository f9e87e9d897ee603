"""GPU: gsx_model_merge (spec/RENDER_SPEC.md §13; csrc/kernels_merge.hip, csrc/kernels_extract.hip) against gsx_model_extract for
identity sources (bit for bit), against the float64 restatement tests/merge_ref.py for baked sources (derived forward-error bounds),
and against oracle.spec_f64.render for frames.  Device bytes are read as tests/test_gpu_extract.py reads them: the resident planes
through gsx_model_download_pod (the exact dequantisation of the stored values: equal only if the stored bits are), the edit records
through the edit buffer and its retained raw snapshot (an `edited` bit shows as a record that is not the default pod: every set bit
belongs to a record with ENABLED), the shade records through the later, speculated frames of a camera path, which shade from them."""
import ctypes as C

import numpy as np
import pytest

from oracle import spec_f64
from tests import common
from tests import extract_ref as X
from tests import merge_ref as R
from tests.model_ops import H, KIND_IDS, KINDS, W, frames as _frames, load as _load, model_len as _len, pod as _pod
from wgpu_3dgs_viewer_app_amd import _lib, camera, query, scene
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as F
from wgpu_3dgs_viewer_app_amd.viewer import BufferHandle, CommGroup, Cov3dKind, GsxError, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
OW, OH = 80, 48  # the frames that are compared with the float64 spec
FRAME_TOL = 1e-3  # spec §8
AMBIGUITY_TOL = 1e-3  # as the golden fixtures: support decisions |q - k^2| < this go into the oracle's per-pixel allowance
U = 2.0 ** -24
BIG = 263169  # the size tests/test_gpu_extract.py's edge test ends with: the scan of the partials takes more than one pass


def fixture_transform(seed, pos=(0.3, -0.2, 0.5), scale=(1.3, -0.7, 0.9)):
    """a random rotation, a scale with a negative component (a reflection), a translation"""
    q = np.random.default_rng(seed).normal(size=4)
    return np.float32(pos), (q / np.linalg.norm(q)).astype(np.float32), np.float32(scale)


def _edits(v, key):
    return v.models[key].gaussian_buffers.gaussians_edit_buffer.download()


def _same_bytes(a, b, what=""):
    for name, x, y in zip(("pos", "color", "sh", "cov3d"), a, b):
        assert x.shape == y.shape and x.tobytes() == np.ascontiguousarray(y).tobytes(), (what, name)


def _edit_records(n, seed, hide=True):
    rng = np.random.default_rng(seed)
    e = query.default_edits(n)
    e["flag"][0::3] = int(F.ENABLED | F.HIDDEN) if hide else int(F.ENABLED | F.OVERRIDE_COLOR)
    e["flag"][1::3] = int(F.ENABLED)
    e["flag"][5::7] |= int(F.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    e["color"][:, 0] = rng.random(n).astype(np.float32)
    e["contrast"] = rng.random(n).astype(np.float32)
    return e


# ---- 1. identity is extract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_identity_source_is_extract(sh, cov):
    n = 2500
    g = common.small_scene(n, 41)
    rng = np.random.default_rng(41)
    flt = X.MASKED | X.SKIP_HIDDEN | X.SELECTED
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, g, "a")
        bufs = v.models["a"].gaussian_buffers
        bufs.mask_buffer.upload(X.words(rng.random(n) < 0.6, True))
        bufs.selection_buffer.upload(X.words(rng.random(n) < 0.7, True))
        bufs.gaussians_edit_buffer.upload(_edit_records(n, 41))
        count = v.models["a"].extract("x", flt)
        total, counts = v.merge("m", ["a"], flt)
        assert 0 < count < n and (total, counts) == (count, [count])
        assert _len(v, "m") == (_lib.GSX_OK, count)
        _same_bytes(_pod(v, "m"), _pod(v, "x"))
        assert _edits(v, "m").tobytes() == _edits(v, "x").tobytes() and (_edits(v, "m")["flag"] != 0).any()
        assert BufferHandle(v, "m", "edits").download().tobytes() == BufferHandle(v, "x", "edits").download().tobytes()
        # the quaternion (0, 0, 0, -1) is the identity too
        v.update_model_transform("a", np.zeros(3, np.float32), np.float32([0, 0, 0, -1]), np.ones(3, np.float32))
        assert v.merge("m2", ["a"], flt)[0] == count
        _same_bytes(_pod(v, "m2"), _pod(v, "x"))
        want = _frames(v, ["x"])
        assert want[0][..., :3].max() > 0
        for key in ("m", "m2"):
            for a, b in zip(_frames(v, [key]), want):
                assert np.array_equal(a, b), key


# ---- 2. joints ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One SH-0 scene; the sources are its prefixes.  Never written to."""
    g = scene.synthetic_gaussians(BIG, 91, 0)
    g.setflags(write=False)
    return g


def _source_with_kept(v, big, key, kept, seed, edits):
    """a model of more Gaussians than `kept`, a mask with exactly `kept` bits set and garbage above n, edit records or none;
    returns its host Gaussians and the kept indices"""
    n = kept if kept == BIG else 2 * kept + 5
    rng = np.random.default_rng(seed)
    keep = np.zeros(n, bool)
    keep[rng.permutation(n)[:kept]] = True
    g = big[seed:seed + n] if kept != BIG else big
    _load(v, g, key)
    v.models[key].gaussian_buffers.mask_buffer.upload(X.words(keep, True))
    if edits:
        v.models[key].gaussian_buffers.gaussians_edit_buffer.upload(_edit_records(n, seed, hide=False))
    return g, np.nonzero(keep)[0]


JOINTS = [((1, 31), (1, 1)), ((31, 33), (1, 1)), ((33, 1023), (1, 1)), ((1023, 1025), (1, 1)), ((1025, 1), (1, 1)), ((1, 31, 33), (1, 0, 1)),
          ((1023, 1025, 33), (1, 0, 1)), ((33, 1, 1023), (0, 1, 0)), ((31, BIG, 33), (1, 0, 1))]


@pytest.mark.parametrize("kept,edits", JOINTS, ids=["+".join(str(k) for k in j[0]) for j in JOINTS])
def test_joints(big, kept, edits):
    with MultiModelViewer() as v:
        keys, host = [], []
        for s, (k, e) in enumerate(zip(kept, edits)):
            keys.append(f"s{s}")
            host.append(_source_with_kept(v, big, keys[-1], k, 7 + 13 * s, bool(e)))
        parts, records, raw = [], [], []
        for key in keys:  # what extract makes of every source, on the host side by side
            assert v.models[key].extract("x", X.MASKED) == kept[keys.index(key)]
            parts.append(_pod(v, "x"))
            records.append(_edits(v, "x"))  # (the default pod where the source has no edit records)
            v.remove_model("x")
        total, counts = v.merge("m", keys, X.MASKED)
        assert counts == list(kept) and total == sum(kept)
        _same_bytes(_pod(v, "m"), [np.concatenate([p[k] for p in parts]) for k in range(4)])
        # the edit records and, through them, the `edited` words — those at the joints among them, where two sources share a word
        got = _edits(v, "m")
        want = np.concatenate(records)
        assert got.tobytes() == want.tobytes()
        assert BufferHandle(v, "m", "edits").download().tobytes() == want.tobytes()
        offs = np.cumsum([0] + list(kept))
        for s, e in enumerate(edits):
            piece = got[offs[s]:offs[s + 1]]
            if not e:
                assert not (piece["flag"] != 0).any()  # a source without edit records: never edited
            elif kept[s] >= 31:
                assert (piece["flag"] != 0).any()
        if total < 5000:  # the shade records: the frames of a model uploaded from the kept host rows (its later frames are speculated)
            _load(v, np.concatenate([g[idx] for g, idx in host]), "fresh")
            v.models["fresh"].gaussian_buffers.gaussians_edit_buffer.upload(want)
            for a, b in zip(_frames(v, ["m"], sh_deg=0), _frames(v, ["fresh"], sh_deg=0)):
                assert np.array_equal(a, b)


# ---- 3. baked planes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,cov", KINDS, ids=KIND_IDS)
def test_baked_planes(sh, cov):
    """Every baked value against merge_ref's float64 result, within the forward-error bound of a float32 evaluation of its own dot
    products, 16 u sum |a_i b_i| (u = 2^-24; for an SH coefficient one more u sum |M_jk c_k| for the rounding of M to float32), plus,
    where the plane is quantised, half a quantum: 1 / 127 for Norm8, one binary16 ulp of the result for Half."""
    n = 1500
    mt = fixture_transform(43)
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, common.small_scene(n, 43), "a", mt)
        src = _pod(v, "a")
        assert v.merge("m", ["a"]) == (n, [n])
        got = _pod(v, "m")
    ref = R.merge([dict(pos=src[0], color=src[1], sh=src[2], cov=src[3], mt=mt)], 0, 0, int(sh), int(cov))
    (xp, xs, xc), (mp, ms, mc) = ref["exact"], ref["mag"]
    assert np.array_equal(got[1], src[1])  # the colour word: carried

    def worst(err, bound, what):
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{sh.name}/{cov.name} {what}: max error {float(err.max()):.3e}, {ratio:.3f} of its bound")
        assert (err <= bound).all(), (what, ratio)

    worst(np.abs(got[0] - xp), 16 * U * mp, "pos")
    quantum_c = R.half_ulp(xc) if cov == Cov3dKind.Half else 0.0
    worst(np.abs(got[3] - xc), 0.5 * quantum_c + 16 * U * mc, "cov3d")
    if sh == ShKind.Single:
        worst(np.abs(got[2] - xs), 17 * U * ms, "sh")
    elif sh == ShKind.Half:
        worst(np.abs(got[2] - xs), 0.5 * R.half_ulp(xs) + 17 * U * ms, "sh")
    elif sh == ShKind.Norm8:
        q = np.rint(got[2].astype(np.float64) * 127.0)  # the stored integer, decoded exactly
        assert np.abs(q).max() <= 127 and np.abs(q / 127.0 - got[2]).max() <= 1e-7
        worst(np.abs(np.maximum(q / 127.0, -1.0) - np.clip(xs, -1.0, 1.0)), 0.5 / 127.0 + 17 * U * ms, "sh")
    # and merge_ref's own rounding of the same float64 results differs from the device by no more than a unit of the plane
    assert np.abs(got[0] - ref["pos"]).max() <= 32 * U * mp.max()


# ---- 3b. the shade records of baked and of offset sources ------------------------------------------------------------------------
def _upload_pod(v, key, pod):
    """a fresh model from pod planes (gsx_model_upload_pod_device; the planes staged on the device with torch)"""
    import torch

    pos, color, sh, cov = pod
    v.add_model(key, pos.shape[0])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pos, color.view(np.int32), sh, cov)]
    torch.cuda.synchronize()
    v.models[key].gaussian_buffers.gaussians_buffer.update_range_pod_device(0, pos.shape[0], *(t.data_ptr() for t in dev))
    v.poll()


RECORD_KINDS = [(ShKind.Single, Cov3dKind.Single), (ShKind.Single, Cov3dKind.Half), (ShKind.Half, Cov3dKind.Single), (ShKind.Half, Cov3dKind.Half),
                (ShKind.Norm8, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)]


@pytest.mark.parametrize("sh,cov", RECORD_KINDS, ids=[f"{s.name}-{c.name}" for s, c in RECORD_KINDS])
def test_shade_records_agree_with_the_planes(sh, cov):
    """The records k_merge_bake writes (16, 12 and 8 words a record: two staging passes of 8, a pass of 8 and one of 4, one pass), and
    the records the identity path writes at an offset, with SH-3 data at SH degree 3.  A model's first frame shades from the SoA
    planes; the later frames of a camera path are speculated and shade from the shade records.  So the frames of the merged model
    must be, bit for bit, the frames of a model freshly uploaded from the merged model's own downloaded pod: the upload writes
    planes and records from one value, and quantising a decoded Half or Norm8 value again gives the stored bits back.
    Sources: an identity source that keeps 37 (so the baked one starts at an offset that is no multiple of 32), a baked source
    that keeps about 60 % of 2300 Gaussians (three workgroups, ragged rounds), and an identity source behind it (offset records
    with SH words)."""
    rng = np.random.default_rng(57)
    keeps = [np.arange(90) % 5 != 4, rng.random(2300) < 0.6, rng.random(700) < 0.5]
    keeps[0][np.nonzero(keeps[0])[0][37:]] = False
    mts = [None, fixture_transform(57), None]
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        for s, (keep, mt) in enumerate(zip(keeps, mts)):
            _load(v, common.small_scene(keep.size, 57 + s), f"s{s}", mt)
            v.models[f"s{s}"].gaussian_buffers.mask_buffer.upload(X.words(keep, True))
        total, counts = v.merge("m", ["s0", "s1", "s2"], X.MASKED)
        assert counts == [int(k.sum()) for k in keeps] and counts[0] == 37 and (37 + counts[1]) % 32 != 0
        pod = _pod(v, "m")
        _upload_pod(v, "fresh", pod)
        _same_bytes(_pod(v, "fresh"), pod)  # (quantising the decoded values again is the identity)
        got, want = _frames(v, ["m"], poses=(5, 6, 7, 8)), _frames(v, ["fresh"], poses=(5, 6, 7, 8))
        assert want[0][..., :3].max() > 0 and not np.array_equal(want[0], want[2])
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


# ---- 4. the frame ---------------------------------------------------------------------------------------------------------------
FRAME_SEED, FRAME_N, FRAME_POSE = 129, 400, 5  # chosen on the CPU: spec_f64.render reports no allowance for either configuration


def _spec_model(pod, mt=None):
    m = dict(pos=pod[0], color=pod[1], sh=pod[2] if pod[2].shape[1] else None, cov3d=pod[3])
    if mt is not None:
        m.update(m_pos=mt[0], m_quat=mt[1], m_scale=mt[2])
    return m


def _spec_frame(models, pose=FRAME_POSE):
    cam = camera.orbit_pose(pose)
    return spec_f64.render(cam.view(), cam.projection(OW / OH), OW, OH, models, ambiguity_tol=AMBIGUITY_TOL)


def test_frame_of_the_merged_model_is_the_frame_of_the_transformed_source():
    """Single + Single: the merged model under the identity against the source under its transform, both on the device, within the
    framebuffer tolerance (the float64 spec's two frames differ by 3.0e-6 for this fixture with the planes the device baked, by
    2.7e-6 with merge_ref's float64 planes rounded to float32)."""
    mt = fixture_transform(FRAME_SEED)
    with MultiModelViewer() as v:
        _load(v, common.small_scene(FRAME_N, FRAME_SEED), "a", mt)
        src = _pod(v, "a")
        assert v.merge("m", ["a"])[0] == FRAME_N
        dst = _pod(v, "m")
        transformed = _frames(v, ["a"], poses=(FRAME_POSE,), size=(OW, OH))[0]
        merged = _frames(v, ["m"], poses=(FRAME_POSE,), size=(OW, OH))[0]
    # the fixture holds no support decision near the cut that matters, in either configuration (so none is allowed for below)
    f_src, amb_src = _spec_frame([_spec_model(src, mt)])
    f_dst, amb_dst = _spec_frame([_spec_model(dst)])
    assert max(amb_src.max(), amb_dst.max()) <= FRAME_TOL
    assert f_src[..., :3].max() > 0.5 and (f_src[..., 3] < 0.99).mean() > 0.5
    diff = float(np.abs(merged.astype(np.float64) - transformed).max())
    print(f"merged frame against the transformed source's: {diff:.3e}; against the float64 spec: merged {np.abs(merged - f_dst).max():.3e}, "
          f"transformed {np.abs(transformed - f_src).max():.3e}; the spec's two frames: {np.abs(f_src - f_dst).max():.3e}")
    assert diff <= FRAME_TOL
    assert np.abs(merged - f_dst).max() <= FRAME_TOL and np.abs(transformed - f_src).max() <= FRAME_TOL


@pytest.mark.parametrize("sh,cov", [(ShKind.Half, Cov3dKind.Half), (ShKind.Norm8, Cov3dKind.Half)], ids=["Half-Half", "Norm8-Half"])
def test_frame_of_a_requantised_model(sh, cov):
    """The merged model's frame against the float64 spec's frame of merge_ref's requantised planes — not against the transformed
    source: quantising twice moves the frame by more than the tolerance in the float64 spec itself (§13)."""
    mt = fixture_transform(FRAME_SEED)
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        _load(v, common.small_scene(FRAME_N, FRAME_SEED), "a", mt)
        src = _pod(v, "a")
        assert v.merge("m", ["a"])[0] == FRAME_N
        merged = _frames(v, ["m"], poses=(FRAME_POSE,), size=(OW, OH))[0]
    ref = R.merge([dict(pos=src[0], color=src[1], sh=src[2], cov=src[3], mt=mt)], 0, 0, int(sh), int(cov))
    want, amb = _spec_frame([_spec_model((ref["pos"], ref["color"], ref["sh"], ref["cov"]))])
    over = np.maximum(np.abs(merged - want) - amb[..., None], 0.0)
    moved = np.abs(want - _spec_frame([_spec_model(src, mt)])[0]).max()
    print(f"{sh.name}/{cov.name}: merged frame against the spec of the requantised planes {np.abs(merged - want).max():.3e} "
          f"(beyond the allowance: {over.max():.3e}); requantising moves the spec's frame by {moved:.3e}")
    assert want[..., :3].max() > 0.5 and over.max() <= FRAME_TOL


# ---- 5. interpenetration --------------------------------------------------------------------------------------------------------
def test_interpenetrating_models_sort_gaussian_by_gaussian():
    """Two models that overlap in depth, one of them moved: merged, they are ONE depth order — the float64 spec's single-model frame of
    merge_ref's concatenation — where the layered frame composites them model by model (chosen on the CPU: the spec's two frames
    differ by 0.30)."""
    n, seed = 300, 60
    mt = fixture_transform(seed, pos=(0.4, 0.1, -0.3), scale=(1.1, 0.8, 1.2))
    with MultiModelViewer() as v:
        _load(v, common.small_scene(n, seed), "a")
        _load(v, common.small_scene(n, seed + 1000), "b", mt)
        a, b = _pod(v, "a"), _pod(v, "b")
        assert v.merge("m", ["a", "b"]) == (2 * n, [n, n])
        merged = _frames(v, ["m"], poses=(FRAME_POSE,), size=(OW, OH))[0]
        layered = _frames(v, ["a", "b"], poses=(FRAME_POSE,), size=(OW, OH))[0]
    ref = R.merge([dict(pos=a[0], color=a[1], sh=a[2], cov=a[3]), dict(pos=b[0], color=b[1], sh=b[2], cov=b[3], mt=mt)])
    want, amb = _spec_frame([_spec_model((ref["pos"], ref["color"], ref["sh"], ref["cov"]))])
    want_layered = _spec_frame([_spec_model(a), _spec_model(b, mt)])[0]
    assert np.abs(want - want_layered).max() > 1e-2
    over = np.maximum(np.abs(merged - want) - amb[..., None], 0.0)
    print(f"merged against the spec's single model: {np.abs(merged - want).max():.3e} (beyond the allowance {over.max():.3e}); "
          f"against the layered frame: {np.abs(merged - layered).max():.3f}")
    assert over.max() <= FRAME_TOL
    assert np.abs(merged - layered).max() > 1e-2


# ---- 6. sources untouched, result usable ----------------------------------------------------------------------------------------
def _lane_sequence(lanes):
    n = 2500
    mt = fixture_transform(47)
    out = []
    with MultiModelViewer() as v:
        v.set_render_options(frames_in_flight=lanes)
        _load(v, common.small_scene(n, 47), "a")
        _load(v, common.small_scene(n, 48), "b", mt)
        for pose in (1, 2, 3, 4):
            out += _frames(v, ["a", "b"], poses=(pose,))
        assert v.merge("m", ["a", "b"])[0] == 2 * n  # behind the frames in flight on the lanes
        for pose in (5, 6, 7, 8):
            out += _frames(v, ["m"], poses=(pose,))
            out += _frames(v, ["a", "b"], poses=(pose,))
    return out


def test_lanes():
    two, one = _lane_sequence(2), _lane_sequence(1)
    assert len(two) == 12 and two[4][..., :3].max() > 0
    for k, (a, b) in enumerate(zip(two, one)):
        assert np.array_equal(a, b), k


def test_sources_untouched_bounds_and_determinism():
    n = 3000
    mt = fixture_transform(49)
    rng = np.random.default_rng(49)
    masks = [rng.random(n) < 0.6 for _ in range(2)]
    with MultiModelViewer() as v, MultiModelViewer() as twin:
        for vv in (v, twin):
            _load(vv, common.small_scene(n, 49), "a")
            _load(vv, common.small_scene(n, 50), "b", mt)
            _load(vv, common.small_scene(n // 3, 52), "c", fixture_transform(52))  # baked, and without edit records
            for key, mask in zip(("a", "b"), masks):
                bufs = vv.models[key].gaussian_buffers
                bufs.mask_buffer.upload(X.words(mask, True))
                bufs.selection_buffer.upload(X.words(~mask))
                bufs.gaussians_edit_buffer.upload(_edit_records(n, 51))

        def state(vv):
            out = []
            for key in ("a", "b", "c"):
                bufs = vv.models[key].gaussian_buffers
                out += [a.tobytes() for a in _pod(vv, key)] + [bufs.mask_buffer.download().tobytes(), bufs.selection_buffer.download().tobytes(),
                                                               bufs.gaussians_edit_buffer.download().tobytes()]
            return out

        before = state(v)
        for a, b in zip(_frames(v, ["a", "b", "c"], poses=(5,)), _frames(twin, ["a", "b", "c"], poses=(5,))):
            assert np.array_equal(a, b)
        flt = X.MASKED | X.SKIP_HIDDEN
        total, counts = v.merge("one", ["a", "b", "c"], flt)
        assert v.merge("two", ["a", "b", "c"], flt) == (total, counts) and min(counts) > 0
        assert state(v) == before == state(twin)
        # the sources' next frames are the frames of the twin that was never merged from (and they kept their transforms)
        for a, b in zip(_frames(v, ["a", "b", "c"], poses=(6, 7)), _frames(twin, ["a", "b", "c"], poses=(6, 7))):
            assert np.array_equal(a, b)
        # determinism: two calls, identical bytes and frames
        one, two = _pod(v, "one"), _pod(v, "two")
        _same_bytes(one, two)
        assert _edits(v, "one").tobytes() == _edits(v, "two").tobytes()
        for a, b in zip(_frames(v, ["one"]), _frames(v, ["two"])):
            assert np.array_equal(a, b)
        # a new model: no mask, no selection; its bounds are the box of the baked positions it holds.  (Those are float32 results:
        # the box of merge_ref's float64 positions rounded to float32 is not reachable exactly, so the box is compared with the
        # positions dst holds, and those with the float64 positions within the float32 bound, below.)
        bufs = v.models["one"].gaussian_buffers
        assert np.all(bufs.mask_buffer.download() == 0xFFFFFFFF) and not bufs.selection_buffer.download().any()
        box = v.models["one"].bounds()
        assert box.count == total and box.n_nonfinite == 0
        assert np.array_equal(box.min, one[0].min(axis=0)) and np.array_equal(box.max, one[0].max(axis=0))
        # ... which are merge_ref's float64 positions rounded to float32, give or take the float32 evaluation
        src = [_pod(v, key) for key in ("a", "b", "c")]
        stored = [_edits(v, key)["flag"] for key in ("a", "b")] + [None]
        ref = R.merge([dict(pos=p[0], color=p[1], sh=p[2], cov=p[3], mt=t, mask=m, edit_flags=f)
                       for p, t, m, f in zip(src, (None, mt, fixture_transform(52)), masks + [None], stored)], flt)
        assert counts[2] == n // 3
        assert ref["counts"] == counts
        baked = ref["baked"]
        assert not baked[:counts[0]].any() and baked[counts[0]:].all()
        assert np.array_equal(one[0][~baked], ref["pos"][~baked])
        assert (np.abs(one[0][baked] - ref["exact"][0][baked]) <= 16 * U * ref["mag"][0][baked]).all()
        # DROP_EDITS: no records; otherwise the kept ones of both sources (edits are colour operations: the bake leaves them alone)
        want = np.concatenate([_edits(v, key)[k] for key, k in zip(("a", "b", "c"), ref["kept"])])
        assert _edits(v, "one").tobytes() == want.tobytes() and BufferHandle(v, "one", "edits").download().tobytes() == want.tobytes()
        assert (want["flag"][:counts[0] + counts[1]] != 0).any() and not (want["flag"][counts[0] + counts[1]:] != 0).any()
        assert v.merge("dropped", ["a", "b", "c"], flt, drop_edits=True)[0] == total
        assert _edits(v, "dropped").tobytes() == query.default_edits(total).tobytes()


# ---- 7. errors and empties ------------------------------------------------------------------------------------------------------
def _merge_raw(v, keys, dst, flt=0, flags=0, n_src=None, counts=True):
    arr = (C.c_char_p * max(len(keys), 1))(*[k.encode() if k is not None else None for k in keys])
    desc, total = _lib.ExtractDesc(flt, flags), C.c_uint64(12345)
    out = (C.c_uint64 * max(len(keys), 1))() if counts else None
    _lib.check(v._L.gsx_model_merge(v._h, arr, len(keys) if n_src is None else n_src, dst.encode(), C.byref(desc), out, C.byref(total)))
    return int(total.value), (list(out)[:len(keys)] if counts else None)


def test_errors_and_empties():
    """Every row of the error list but the allocation failure, which a test cannot ask of a shared device."""
    n = 700
    g = common.small_scene(n, 53)
    with MultiModelViewer() as v, MultiModelViewer(sh=ShKind.Norm8, cov3d=Cov3dKind.Half) as other:
        _load(v, g, "a")
        _load(v, g[:300], "b", fixture_transform(53))
        reference = _frames(v, ["a", "b"], poses=(9,))[0]
        many = ["a"] * (R.MAX_SOURCES + 1)
        cases = [(["a", "b"], "a", 0, 0, None, _lib.GSX_ERR_INVALID_ARG),      # dst equals a source
                 (["a", "b"], "b", 0, 0, None, _lib.GSX_ERR_INVALID_ARG),
                 (["a", "nope", "b"], "new", 0, 0, None, _lib.GSX_ERR_NOT_FOUND),  # unknown source
                 (["a"], "new", 8, 0, None, _lib.GSX_ERR_INVALID_ARG),          # unknown filter bits
                 (["a"], "new", 0, 4, None, _lib.GSX_ERR_INVALID_ARG),          # unknown flag bits
                 (["a"], "new", 0, 0, 0, _lib.GSX_ERR_INVALID_ARG),             # n_src = 0
                 (many, "new", 0, 0, None, _lib.GSX_ERR_INVALID_ARG),           # n_src = 65
                 (["a", None], "new", 0, 0, None, _lib.GSX_ERR_INVALID_ARG)]    # a null key
        for keys, dst, flt, flags, n_src, status in cases:
            with pytest.raises(GsxError) as e:
                _merge_raw(v, keys, dst, flt, flags, n_src)
            assert e.value.status == status and "gsx_model_merge" in str(e.value), (keys, dst)
            assert _len(v, "new")[0] == _lib.GSX_ERR_NOT_FOUND
        with pytest.raises(GsxError) as e:
            _merge_raw(v, ["a", "nope"], "new")
        assert "'nope'" in str(e.value)  # the message names the unknown source
        assert _merge_raw(v, many[:-1], "sixty-four")[0] == R.MAX_SOURCES * n  # 64 sources, one key 64 times: allowed
        v.remove_model("sixty-four")
        assert v.merge("exists", ["a"])[0] == n
        with pytest.raises(GsxError) as e:
            v.merge("exists", ["a"])  # dst exists
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG
        # null arguments
        L, desc, total = v._L, _lib.ExtractDesc(0, 0), C.c_uint64()
        keys = (C.c_char_p * 1)(b"a")
        assert L.gsx_model_merge(v._h, None, 1, b"new", C.byref(desc), None, C.byref(total)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_merge(v._h, keys, 1, None, C.byref(desc), None, C.byref(total)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_merge(v._h, keys, 1, b"new", None, None, C.byref(total)) == _lib.GSX_ERR_INVALID_ARG
        assert L.gsx_model_merge(v._h, keys, 1, b"new", C.byref(desc), None, None) == _lib.GSX_ERR_INVALID_ARG
        assert _len(v, "new")[0] == _lib.GSX_ERR_NOT_FOUND
        # a transform with a non-finite component, or a zero quaternion
        good = fixture_transform(53)
        for bad in ((np.float32([np.nan, 0, 0]), good[1], good[2]), (good[0], np.float32([0, np.inf, 0, 1]), good[2]),
                    (good[0], good[1], np.float32([1, -np.inf, 1])), (good[0], np.zeros(4, np.float32), good[2])):
            v.update_model_transform("b", *bad)
            with pytest.raises(GsxError) as e:
                v.merge("new", ["a", "b"])
            assert e.value.status == _lib.GSX_ERR_INVALID_ARG and "'b'" in str(e.value)
        v.update_model_transform("b", *good)
        assert np.array_equal(_frames(v, ["a", "b"], poses=(9,))[0], reference)  # the viewer still renders its sources
        # out_counts == NULL
        assert _merge_raw(v, ["a", "b"], "nocounts", counts=False) == (n + 300, None)
        # a key given twice: the model, twice
        total, counts = v.merge("twice", ["b", "a", "b"])
        assert (total, counts) == (n + 600, [300, n, 300])
        twice = _pod(v, "twice")
        _same_bytes([p[:300] for p in twice], [p[n + 300:] for p in twice])
        _same_bytes([p[300:n + 300] for p in twice], _pod(v, "a"))
        # nothing kept anywhere (no selection = none pass): GSX_OK, a total of 0 and no model
        assert v.merge("empty", ["a", "b"], X.SELECTED) == (0, [0, 0]) and "empty" not in v.models
        assert _len(v, "empty")[0] == _lib.GSX_ERR_NOT_FOUND
        # ... and a source that keeps nothing beside one that keeps something
        v.models["a"].gaussian_buffers.selection_buffer.upload(X.words(np.arange(n) % 2 == 0))
        assert v.merge("half", ["b", "a"], X.SELECTED) == ((n + 1) // 2, [0, (n + 1) // 2])
        _same_bytes(_pod(v, "half"), [p[0::2] for p in _pod(v, "a")])
        # a sharded source
        v.shard_set_limits("b", np.full((H + 15) // 16 * ((W + 15) // 16), 0x40400000, np.uint32))
        with pytest.raises(GsxError) as e:
            v.merge("new", ["a", "b"])
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED
        # mixed pod kinds: a model of another viewer cannot be named, so two kinds meet only through models created with other kinds
        _lib.check(L.gsx_model_create(v._h, b"norm8", 10, int(ShKind.Norm8), int(Cov3dKind.Half)))
        with pytest.raises(GsxError) as e:
            v.merge("new", ["a", "norm8"])
        assert e.value.status == _lib.GSX_ERR_INVALID_ARG and "'norm8'" in str(e.value)
        assert _len(v, "new")[0] == _lib.GSX_ERR_NOT_FOUND
        # a viewer with a communicator
        _load(other, g[:50], "a")
        group = CommGroup(1)
        other.comm_init_group(group, 0)
        with pytest.raises(GsxError) as e:
            other.merge("new", ["a"])
        assert e.value.status == _lib.GSX_ERR_UNSUPPORTED
