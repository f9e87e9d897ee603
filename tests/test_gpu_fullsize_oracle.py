"""GPU: the HIP path against the CPU oracle at BASELINE.json's FULL sizes (VERDICT r5 "missing" item 3).

Up to round 5 the largest frame compared with the oracle was cfg1 (50 k Gaussians, 640x480); cfg2 ... cfg5 were checked at
full size through properties and against other schedules of the same kernels only.  The oracle (oracle/gsx_oracle.c, OpenMP)
renders a whole 10 M-Gaussian 1080p frame in seconds on the GPU box's host cores, so here the contract of K1-K3
(src/tab/scene.rs:856-869 preprocess + sort, :2302-2314 render) is checked directly at 8160 / 32 400 tiles:

  * K1: cull set + depth keys + tile rectangles BIT-EXACT against oracle.project; mean / conic / colour within float32 rounding
  * K2: the depth order (ties by Gaussian index) BIT-EXACT against oracle.depth_sort
  * K3: the frame <= 1e-3 per-channel L-infinity (north_star's tolerance) against oracle.rasterize — the reference's algorithm
        shape: back-to-front, splat-major, no tiles, no early termination — from the plainest schedule (speculative = 0,
        progressive = 0) AND from the default schedule's speculated frames (two frames in flight); the observed value is
        printed and bounded by FB_OBSERVED (a regression guard well inside the tolerance)

cfg4 is checked a second time in the application's default pod (Norm8 SH + Half cov3d: the oracle computes with the round-tripped
planes, the device's stored planes equal them bit for bit), and cfg5 in full: four layered models, the mask, the rectangle
selection made on the device and the HSV edit of what it selected — selection words, stored edit records, edited colours, depth
order and the frame, under the staged calls, the default schedule, and after the edit mode was left.
"""
import numpy as np
import pytest

import oracle
from tests import common
from tests.test_gpu_parity import FB_TOL, FLOAT_TOL
from wgpu_3dgs_viewer_app_amd import camera, query, scene
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, GaussianDisplayMode, GaussianShDegree, MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu

# what the frames are expected to differ by: the compositor stops a pixel at T < t_epsilon = 1e-4 (the oracle blends everything) and
# sums front to back where the oracle sums back to front
FB_OBSERVED = 4e-4


def _oracle_model(g, cam, w, h, mt=None, mask=None, fb=None, planes=None):
    f = common.oracle_frame(cam, w, h, mt)
    pos, color, sh, cov = planes if planes is not None else oracle.convert(g)
    pr = oracle.project(f, pos, color, sh, cov, mask)
    del sh, planes
    idx, nvis = oracle.depth_sort(pr["key"])
    if fb is None:
        fb = oracle.new_framebuffer(f)
    oracle.rasterize(f, pr, idx, nvis, fb)
    return pr, idx, nvis, fb


def _assert_projection(gp, pr, what):
    assert np.array_equal(gp["key"], pr["key"]), f"{what}: depth keys / cull set differ"
    assert np.array_equal(gp["rect"], pr["rect"]), f"{what}: tile rectangles differ"
    vis = pr["key"] != 0xFFFFFFFF
    for name in ("mean2d", "conic_opacity", "rgb"):
        a, b = gp[name][vis], pr[name][vis]
        bad = np.abs(a - b) > FLOAT_TOL + FLOAT_TOL * np.abs(b)
        assert not bad.any(), f"{what}: {name} differs on {int(bad.sum())} values, max {float(np.abs(a - b).max())}"


def _check_config(cfg, poses_speculated, pose, pod=None):
    """pod: None (float32 planes) or (ShKind, Cov3dKind): the viewer stores the model in that pod, the oracle computes with the planes
    after the pod's quantise -> dequantise round trip, and the device's stored planes must equal those bit for bit."""
    n, sh, w, h, seed = scene.CONFIGS[cfg]
    g = scene.synthetic_gaussians(n, seed, sh)
    cam = camera.orbit_pose(pose)
    planes = None if pod is None else oracle.convert_pod(g, int(pod[0]), int(pod[1]))
    pr, idx, nvis, fb_ref = _oracle_model(g, cam, w, h, planes=planes)
    assert nvis > n // 2
    out = {}
    with (MultiModelViewer() if pod is None else MultiModelViewer(sh=pod[0], cov3d=pod[1])) as v:
        v.set_render_options(speculative=0, progressive=0)
        v.add_model("m", n)
        v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
        del g
        if pod is not None:
            got = list(v.models["m"].gaussian_buffers.gaussians_buffer.download_pod())
            planes = list(planes)
            for name in ("cov3d", "sh", "color", "pos"):   # plane by plane, the large ones freed first
                a, b = got.pop(), planes.pop()
                assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{cfg}: the stored {name} plane differs from the oracle's round trip"
                del a, b
        v.update_camera(cam, (w, h))
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh), False)
        v.preprocessor.preprocess("m")
        v.radix_sorter.sort("m")
        v.poll()
        gp = v.download_projection("m")
        _assert_projection(gp, pr, cfg)
        del gp
        order = v.download_sorted("m")
        assert order.size == nvis and np.array_equal(order, idx[:nvis]), f"{cfg}: depth order differs from the oracle's"
        v.renderer.render(["m"])
        st = v.frame_stats("m")
        assert st["n_visible"] == nvis and st["overflow_slabs"] == 0
        fb_plain = v.download_framebuffer().copy()
        out["plain"] = float(np.abs(fb_plain - fb_ref).max())
        # the default schedule: progressive slabs + temporal occlusion speculation, two frames in flight, arriving at `pose` along
        # the orbit so that its frame is a speculated one (geometry-only projection, admission, sparse shading, one slab, repair)
        v.set_render_options(frames_in_flight=2)
        for p in poses_speculated:
            v.update_camera(camera.orbit_pose(p), (w, h))
            v.render_frame(["m"])
        assert poses_speculated[-1] == pose
        fb_spec = v.download_framebuffer()
        st = v.frame_stats("m")
        assert st["speculated"] and st["n_sorted"] < st["n_visible"], f"{cfg}: the last frame was not speculated: {st}"
        out["speculated"] = float(np.abs(fb_spec - fb_ref).max())
        out["speculated_equals_plain"] = bool(np.array_equal(fb_spec, fb_plain))
        out["n_visible"], out["n_sorted_speculated"] = nvis, st["n_sorted"]
    print(f"{cfg}{'' if pod is None else ' ' + pod[0].name + '+' + pod[1].name} pose {pose}: HIP vs oracle L-inf plain {out['plain']:.3e}, speculated {out['speculated']:.3e}; "
          f"N_vis {nvis}, depth-sorted on the speculated frame {out['n_sorted_speculated']}")
    assert out["speculated_equals_plain"], f"{cfg}: the speculated frame differs from the plain one"
    for k in ("plain", "speculated"):
        assert out[k] <= FB_TOL, f"{cfg} {k} frame: L-inf {out[k]} > 1e-3 against the oracle"
        assert out[k] <= FB_OBSERVED, f"{cfg} {k} frame: L-inf {out[k]} (expected ~t_epsilon)"


def test_cfg2_full_size_against_the_oracle():
    """BASELINE configs[1]: 1 M Gaussians SH-3 at 1920x1080."""
    _check_config("cfg2", [236, 237, 238, 239, 0], 0)


def test_cfg3_full_size_against_the_oracle():
    """BASELINE configs[2] (garden-sized synthetic, 5.8 M): one pose in the expensive quarter of the orbit."""
    _check_config("cfg3", [96, 97, 98, 99, 100], 100)


def test_cfg4_full_size_against_the_oracle():
    """BASELINE configs[3] on one GPU: 10 M Gaussians SH-3 at 1920x1080 — the frame bench.py's cpu_baseline renders."""
    _check_config("cfg4", [236, 237, 238, 239, 0], 0)


def test_cfg4_full_size_default_pod_against_the_oracle():
    """cfg4 in the application's default pod (Norm8 SH + Half cov3d): stored planes bit-exact, then the float32 run's assertions
    unchanged — FB_OBSERVED was measured on the float32 pod, and both sides dequantise the same values here."""
    _check_config("cfg4", [236, 237, 238, 239, 0], 0, pod=(ShKind.Norm8, Cov3dKind.Half))


def test_cfg5_two_layered_models_with_mask_at_3840x2160_against_the_oracle():
    """BASELINE configs[4] at its resolution: the masked model ('0 - 1': box minus ellipsoid, evaluated on the device and by the
    oracle: mask words bit-exact) with its TRS, layered with a second 6 M-Gaussian model the way the app paints them (far -> near,
    never merged: scene.rs:533-558, 2302-2314); 32 400 tiles, the oracle paints the far model first and the near one over it."""
    from wgpu_3dgs_viewer_app_amd import parallel
    from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator, MaskOp, MaskShape, MaskShapeKind, pack_program

    n_total, sh, w, h, seed = scene.CONFIGS["cfg5"]
    n = n_total // 4
    tr = {"a": camera.ModelTransform(pos=np.array([0.0, 0.0, 2.5], np.float32)),
          "d": camera.ModelTransform(pos=np.array([0.3, -0.2, 0.5], np.float32), rot=np.array([20, -35, 50], np.float32),
                                     scale=np.array([1.2, 0.9, 1.1], np.float32))}
    seeds = {"a": seed, "d": seed + 3}
    shapes = [MaskShape(MaskShapeKind.Box, pos=np.array([0.0, 0.0, 2.5], np.float32), scale=np.array([3.0, 3.0, 3.0], np.float32)),
              MaskShape(MaskShapeKind.Ellipsoid, pos=np.array([0.0, 0.0, 2.5], np.float32), scale=np.array([1.5, 1.5, 1.5], np.float32))]
    op = MaskOp.parse("0 - 1")
    pose = 40
    cam = camera.orbit_pose(pose)
    keys = parallel.model_render_keys(cam.pos, tr)   # far -> near
    assert sorted(keys) == ["a", "d"]
    fb_ref = None
    ref = {}
    with MultiModelViewer() as v:
        v.set_render_options(speculative=0, progressive=0)
        for k in keys:   # the oracle paints in this order; the upload order does not matter
            g = scene.synthetic_gaussians(n, seeds[k], sh)
            mask = None
            if k == "a":
                mask = oracle.mask_evaluate(oracle.convert(g)[0], tr[k].pos, tr[k].quat(), tr[k].scale, *pack_program(op, shapes))
            pr, idx, nvis, fb_ref = _oracle_model(g, cam, w, h, tr[k], mask, fb_ref)
            ref[k] = (pr, idx, nvis, mask)
            v.add_model(k, n)
            v.models[k].gaussian_buffers.gaussians_buffer.update_range(0, g)
            v.update_model_transform(k, tr[k].pos, tr[k].quat(), tr[k].scale)
            del g
        MaskEvaluator(v).evaluate(op, "a", shapes)
        got = v.models["a"].gaussian_buffers.mask_buffer.download()
        want = ref["a"][3]
        tail = (1 << (n & 31)) - 1 if n & 31 else 0xFFFFFFFF
        assert np.array_equal(got[:-1], want[:-1]) and (got[-1] & tail) == (want[-1] & tail), "mask words differ"
        kept = int(np.unpackbits(want.view(np.uint8)).sum())
        assert n // 50 < kept < n, kept
        v.update_camera(cam, (w, h))
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh), False)
        for k in keys:
            v.preprocessor.preprocess(k)
            v.radix_sorter.sort(k)
        v.poll()
        for k in keys:
            pr, idx, nvis, _ = ref[k]
            _assert_projection(v.download_projection(k), pr, f"cfg5 model {k}")
            assert np.array_equal(v.download_sorted(k), idx[:nvis]), f"cfg5 model {k}: depth order differs"
        v.renderer.render(keys)
        fb_plain = v.download_framebuffer().copy()
        # default schedule, speculated frames
        v.set_render_options()
        for p in (36, 37, 38, 39, 40):
            c = camera.orbit_pose(p)
            v.update_camera(c, (w, h))
            v.render_frame(parallel.model_render_keys(c.pos, tr))
        fb_spec = v.download_framebuffer()
        assert any(v.frame_stats(k)["speculated"] for k in keys)
    e_plain, e_spec = float(np.abs(fb_plain - fb_ref).max()), float(np.abs(fb_spec - fb_ref).max())
    print(f"cfg5 (2 of 4 models, mask on one, 3840x2160) pose {pose}: HIP vs oracle L-inf plain {e_plain:.3e}, speculated {e_spec:.3e}; "
          f"N_vis {[ref[k][2] for k in keys]}, mask keeps {kept} of {n}")
    assert np.array_equal(fb_spec, fb_plain)
    assert e_plain <= FB_TOL and e_plain <= FB_OBSERVED, e_plain


def _bits(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def _assert_edited_projection(gp, ref, what):
    """Projection after the colour ops: integers bit-exact, mean / conic within FLOAT_TOL, edited colours and the opacity the edit's
    alpha scales within tests/test_gpu_edit.py's rtol = 1e-5, atol = 1e-6 (2^x and x^y are the only transcendental steps)."""
    assert np.array_equal(gp["key"], ref["key"]), f"{what}: depth keys / cull set differ"
    assert np.array_equal(gp["rect"], ref["rect"]), f"{what}: tile rectangles differ"
    vis = ref["key"] != 0xFFFFFFFF
    for name, a, b, rtol, atol in (("mean2d", gp["mean2d"], ref["mean2d"], FLOAT_TOL, FLOAT_TOL),
                                   ("conic", gp["conic_opacity"][:, :3], ref["conic_opacity"][:, :3], FLOAT_TOL, FLOAT_TOL),
                                   ("opacity", gp["conic_opacity"][:, 3], ref["conic_opacity"][:, 3], 1e-5, 1e-6),
                                   ("rgb", gp["rgb"], ref["rgb"], 1e-5, 1e-6)):
        a, b = a[vis], b[vis]
        bad = np.abs(a - b) > atol + rtol * np.abs(b)
        assert not bad.any(), f"{what}: {name} differs on {int(bad.sum())} values, max {float(np.abs(a - b).max())}"


def test_cfg5_in_full_selection_and_edit_against_the_oracle():
    """BASELINE configs[4] complete, the benchmark's cfg5 scene (tests/common.py cfg5_scene): four 6 M-Gaussian models with their TRS,
    the `0 - 1` mask on `a`, 3840x2160 (240 x 135 tiles), layered far -> near.

      1. selection frame at orbit pose 0 (paint order a d c b), staged calls, speculative = 0, progressive = 0: the rectangle query
         rides on the frame, postprocess applies `Set`.  Selection words of all four models BIT-EXACT against oracle.project ->
         query_flags -> selection_op; mask words of `a` bit-exact; every model has between n/100 and n Gaussians selected.
      2. edited frame at pose 40 (paint order c a d b — another order than the selection pose's), staged: per model keys, rectangles and
         depth order bit-exact, mean / conic within FLOAT_TOL, edited colours and opacity within 1e-5 relative, the stored edit records
         byte-equal to the oracle's; the frame <= FB_TOL and <= FB_OBSERVED of the oracle's (project -> edit_pass -> depth_sort ->
         rasterize per model, in paint order onto one framebuffer).
      3. default schedule (progressive slabs, speculation, two frames in flight), arriving at pose 40 along 36 .. 40 with the edit on:
         some model speculated on the last frame, no slab of that frame overflowed the pair buffers, the frame BIT-IDENTICAL to the
         staged one.  (overflow_slabs counts over the model's lifetime, per lane: measured, the staged progressive = 0 frames at this
         size spill one slab each of `b` and `d` — whole-model per-tile lists of the two nearest models want more than the 16 entries
         per record the pair buffers start with; complete pixels by k_composite_spill, as the oracle comparison of that very frame
         shows — and no default-schedule frame spills any.  So the counter is read after every frame and a frame's own spills are
         the difference to its lane's previous reading: asserted zero for the last frame and for the edit-left frame.)
      4. edit left (selection cleared, GaussianEditPod.default()): one more default-schedule frame at pose 40 — the stored edits keep
         rendering — against the oracle's frame made with edit_pass(pr, None, edits, default) from the same four projections."""
    from wgpu_3dgs_viewer_app_amd import parallel
    from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator, pack_program

    sc = common.cfg5_scene()
    n, sh, w, h, tr, rect, edit = sc["n"], sc["sh"], sc["w"], sc["h"], sc["tr"], sc["rect"], sc["edit"]
    pose_sel, pose = 0, 40
    cam_sel, cam = camera.orbit_pose(pose_sel), camera.orbit_pose(pose)
    keys_sel, keys = parallel.model_render_keys(cam_sel.pos, tr), parallel.model_render_keys(cam.pos, tr)   # far -> near
    assert keys_sel == ["a", "d", "c", "b"] and keys == ["c", "a", "d", "b"], (keys_sel, keys)
    assert keys != keys_sel, "the edited frame must paint in another order than the selection frame"
    words = (n + 31) // 32
    tail = (1 << (n & 31)) - 1 if n & 31 else 0xFFFFFFFF

    def same_words(got, want):
        return got.shape == want.shape and np.array_equal(got[:-1], want[:-1]) and (got[-1] & tail) == (want[-1] & tail)

    sel_ref, pr_ref, mask_ref = {}, {}, None
    with MultiModelViewer() as v:
        v.set_render_options(speculative=0, progressive=0)
        for k in tr:
            g = scene.synthetic_gaussians(n, sc["seeds"][k], sh)
            pos, color, shp, cov = oracle.convert(g)
            mask = None
            if k == "a":
                mask = mask_ref = oracle.mask_evaluate(pos, tr[k].pos, tr[k].quat(), tr[k].scale, *pack_program(sc["mask_op"], sc["mask_shapes"]))
            pr0 = oracle.project(common.oracle_frame(cam_sel, w, h, tr[k]), pos, color, shp, cov, mask)   # (never rasterised)
            sel_ref[k] = oracle.selection_op(rect.op, oracle.query_flags(pr0, rect), np.zeros(words, np.uint32))
            del pr0
            pr_ref[k] = oracle.project(common.oracle_frame(cam, w, h, tr[k]), pos, color, shp, cov, mask)
            del pos, color, shp, cov
            v.add_model(k, n)
            v.models[k].gaussian_buffers.gaussians_buffer.update_range(0, g)
            v.update_model_transform(k, tr[k].pos, tr[k].quat(), tr[k].scale)
            del g
        MaskEvaluator(v).evaluate(sc["mask_op"], "a", sc["mask_shapes"])
        assert same_words(v.models["a"].gaussian_buffers.mask_buffer.download(), mask_ref), "mask words differ"
        kept = _bits(mask_ref)
        assert n // 50 < kept < n, kept

        def staged(c, order):
            v.update_camera(c, (w, h))
            v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh), False)
            for k in order:
                v.preprocessor.preprocess(k)
                v.radix_sorter.sort(k)
            v.poll()

        # 1. the selection frame
        v.update_query(rect)
        staged(cam_sel, keys_sel)
        v.renderer.render(keys_sel)
        for k in keys_sel:
            v.postprocessor.postprocess(k)
        v.poll()
        v.update_query(query.QueryPod.none())
        selected = {}
        for k in tr:
            got = v.models[k].gaussian_buffers.selection_buffer.download()
            selected[k] = _bits(sel_ref[k])
            assert n // 100 < selected[k] < n, f"model {k}: the rectangle selects {selected[k]} of {n}"
            if not same_words(got, sel_ref[k]):
                d = np.nonzero(got != sel_ref[k])[0]
                raise AssertionError(f"model {k}: selection words differ from the oracle's on {d.size} words, first at Gaussian {int(d[0]) * 32}, "
                                     f"device selects {_bits(got)}, oracle {selected[k]}")
        # 2. the edited frame, staged
        v.update_selection_edit_with_pod(edit)
        staged(cam, keys)
        fb_ref, edits_ref, nvis_ref = None, {}, {}
        for k in keys:
            f = common.oracle_frame(cam, w, h, tr[k])
            ref = {name: (a.copy() if isinstance(a, np.ndarray) else a) for name, a in pr_ref[k].items()}
            edits_ref[k] = query.default_edits(n)
            nv = oracle.edit_pass(ref, sel_ref[k], edits_ref[k], edit)
            idx, nvis = oracle.depth_sort(ref["key"])
            assert nvis == nv
            nvis_ref[k] = nvis
            if fb_ref is None:
                fb_ref = oracle.new_framebuffer(f)
            oracle.rasterize(f, ref, idx, nvis, fb_ref)
            _assert_edited_projection(v.download_projection(k), ref, f"cfg5 model {k}, edited")
            assert (ref["rgb"] != pr_ref[k]["rgb"]).any(), f"model {k}: the edit changes no colour"
            assert np.array_equal(v.download_sorted(k), idx[:nvis]), f"cfg5 model {k}: depth order differs"
            assert v.frame_stats(k)["n_visible"] == nvis
            assert v.models[k].gaussian_buffers.gaussians_edit_buffer.download().tobytes() == edits_ref[k].tobytes(), f"model {k}: stored edit records differ"
            del ref, idx
        v.renderer.render(keys)
        fb_staged = v.download_framebuffer().copy()
        e_staged = float(np.abs(fb_staged - fb_ref).max())
        # 3. the default schedule, two frames in flight, the edit still on
        v.set_render_options(frames_in_flight=2)

        def frame(p):
            c = camera.orbit_pose(p)
            v.update_camera(c, (w, h))
            v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh), False)
            v.render_frame(parallel.model_render_keys(c.pos, tr))

        def overflow():
            """Slabs spilled so far, per model.  gsx_frame_stats counts them over the LIFETIME of the model as the lane of the newest frame
            holds it (two frames in flight: two lanes taking turns), so what a frame itself spilled is the difference to the reading
            after that lane's frame before: two frames earlier."""
            return {k: v.frame_stats(k)["overflow_slabs"] for k in tr}

        ov = [overflow()]   # after the staged frames
        for p in (36, 37, 38, 39):
            frame(p)
            ov.append(overflow())
        frame(pose)
        fb_spec = v.download_framebuffer().copy()
        stats = {k: v.frame_stats(k) for k in keys}
        ov.append(overflow())
        assert any(st["speculated"] for st in stats.values()), f"no model speculated on the last frame: {stats}"
        assert ov[-1] == ov[-3], f"slabs of the last frame did not fit the pair buffers: {ov}"
        e_spec = float(np.abs(fb_spec - fb_ref).max())
        spec_equals_staged = bool(np.array_equal(fb_spec, fb_staged))
        del fb_ref
        # 4. the edit mode left: no selection, the default edit pod; the stored records keep rendering
        for k in tr:
            v.models[k].gaussian_buffers.selection_buffer.upload(None)
        v.update_selection_edit_with_pod(query.GaussianEditPod.default())
        frame(pose)
        fb_left = v.download_framebuffer().copy()
        ov.append(overflow())
        for k in tr:
            assert v.models[k].gaussian_buffers.gaussians_edit_buffer.download().tobytes() == edits_ref[k].tobytes(), f"model {k}: stored edit records changed"
    fb_ref2 = None
    for k in keys:
        f = common.oracle_frame(cam, w, h, tr[k])
        ref = pr_ref.pop(k)     # (the last use of the unedited projection: edited in place)
        nv = oracle.edit_pass(ref, None, edits_ref[k], query.GaussianEditPod.default())
        assert nv == nvis_ref[k], "this edit hides nothing"
        idx, nvis = oracle.depth_sort(ref["key"])
        if fb_ref2 is None:
            fb_ref2 = oracle.new_framebuffer(f)
        oracle.rasterize(f, ref, idx, nvis, fb_ref2)
        del ref, idx
    e_left = float(np.abs(fb_left - fb_ref2).max())
    print(f"cfg5 in full (4 models, mask on a, rect selection + HSV edit, 3840x2160) pose {pose}: HIP vs oracle L-inf staged {e_staged:.3e}, "
          f"speculated {e_spec:.3e}, edit left {e_left:.3e}; N_vis {[nvis_ref[k] for k in keys]} in paint order {keys}, "
          f"selected {selected}, edit records stored {[int((edits_ref[k]['flag'] != 0).sum()) for k in keys]}, mask keeps {kept} of {n}; "
          f"slabs spilled (lifetime, per lane) after the staged frames, poses 36 .. 40 and the edit-left frame {[list(o.values()) for o in ov]}; speculated on the last frame {[k for k in keys if stats[k]['speculated']]}")
    assert spec_equals_staged, "the default schedule's frame differs from the staged one"
    assert ov[-1] == ov[-3], f"slabs of the edit-left frame did not fit the pair buffers: {ov}"
    for name, e in (("staged", e_staged), ("speculated", e_spec), ("edit left", e_left)):
        assert e <= FB_TOL, f"cfg5 {name} frame: L-inf {e} > 1e-3 against the oracle"
        assert e <= FB_OBSERVED, f"cfg5 {name} frame: L-inf {e} (expected ~t_epsilon)"
