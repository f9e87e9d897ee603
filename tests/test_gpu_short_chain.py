"""GPU: GSX_SHORT_CHAIN — a speculated frame's shading rides in the depth sort's launches — renders the same frames as the serial order.

With the switch on (the default) the admitted records of a speculated frame are shaded by rider workgroups of k_msd_sweep and
k_bucket_sort (csrc/shade_quads.h) instead of a k_shade_quads launch in front of them, in the main round and in the repair round.
The same instructions run on the same inputs, so the bar is equality: every case below runs once per side, each in a process of its
own (the switch is read when a viewer is created), and the framebuffers are compared with np.array_equal and the frame statistics
field by field.  The cases also report the shade pass's launch count, so that the test knows the riders really carried the shading
(no shade launch on a speculated frame without colour ops) and that the other side really is the serial order.
The suites that pin the default side run again with GSX_SHORT_CHAIN=0: the side that stays must stay right."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_FIELDS = ("n_visible", "n_sorted", "n_tile_entries", "n_repair_tiles", "overflow_slabs")
POD_KINDS = [(sh, cov, deg) for sh in (0, 1, 2) for cov in (0, 1) for deg in (0, 1, 2, 3)]


# ---- the cases: run in the child process; each returns (frames, stats per frame, shade launches per frame, speculated per frame) ----
def _fixture_frames(name, schedule_opts, lanes=1, prior=False):
    from tests import golden_util
    from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator, MaskOp
    from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, DepthCompare, GaussianDisplayMode, GaussianShDegree, MultiModelViewer, ShKind

    fx = golden_util.Fixture([p for p in golden_util.GOLDEN if name in p][0])
    keys = [f"m{k}" for k in range(fx.n_models)]
    out = []
    with MultiModelViewer(sh=ShKind(fx.pod[0]), cov3d=Cov3dKind(fx.pod[1])) as v:
        v.set_render_options(frames_in_flight=lanes, **schedule_opts)
        if fx.params:
            v.set_spec_params(**fx.params)
        for k in range(fx.n_models):
            g = fx.gaussians(k)
            v.add_model(keys[k], g.shape[0])
            bufs = v.models[keys[k]].gaussian_buffers
            bufs.gaussians_buffer.update_range(0, g)
            v.update_model_transform(keys[k], *fx.transform(k))
            if fx.mask_expr:
                MaskEvaluator(v).evaluate(MaskOp.parse(fx.mask_expr), keys[k], fx.mask_shapes())
            if fx.selection_words(k) is not None:
                bufs.selection_buffer.upload(fx.selection_words(k))
        if fx.sel_edit is not None:
            v.update_selection_edit_with_pod(fx.edit_pod())
        if fx.highlight is not None:
            v.update_selection_highlight(fx.highlight)
        if fx.depth is not None:
            v.set_depth_test(DepthCompare.Less)
            v.update_depth_buffer(fx.depth)
        v.update_gaussian_transform(fx.size, GaussianDisplayMode(fx.display_mode), GaussianShDegree.new(fx.sh_deg), bool(fx.no_sh0))
        order = [keys[k] for k in fx.paint_order]
        if prior:  # every lane gets windows that belong to another camera: the repair round has work
            for _ in range(lanes):
                v.update_camera_with_matrices(*fx.prior, (fx.w, fx.h))
                v.render_frame(order)
            v.poll()
        v.get_pass_timing()
        for _ in range(2 * lanes + 1):
            v.update_camera_with_matrices(fx.view, fx.proj, (fx.w, fx.h))
            v.render_frame(order)
            out.append(_observe(v, order))
    return out


def _observe(v, order):
    fb = v.download_framebuffer()
    stats = [v.frame_stats(k) for k in order]
    return fb, stats, v.get_pass_timing()["shade"]["launches"]


def _orbit_frames(n, seed, size, sh=0, cov=0, deg=3, poses=(10, 11, 12, 13), edit=False, scale_mul=10.0):
    from tests import common
    from wgpu_3dgs_viewer_app_amd import camera, query
    from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, GaussianDisplayMode, GaussianShDegree, MultiModelViewer, ShKind

    g = common.small_scene(n, seed, scale_mul=scale_mul)
    out = []
    with MultiModelViewer(sh=ShKind(sh), cov3d=Cov3dKind(cov)) as v:
        v.set_render_options(min_slab=2048)
        v.add_model("m", n)
        bufs = v.models["m"].gaussian_buffers
        bufs.gaussians_buffer.update_range(0, g)
        if edit:  # stored edits on every third Gaussian, and the highlight of a selection
            rng = np.random.default_rng(seed)
            edits = query.default_edits(n)
            edits["flag"][::3] = int(query.GaussianEditFlag.ENABLED | query.GaussianEditFlag.OVERRIDE_COLOR)
            edits["color"][::3] = (0.9, 0.2, 0.1)
            edits["exposure"][::3] = 0.5
            edits["alpha"][::3] = 0.8
            bufs.gaussians_edit_buffer.upload(edits)
            bufs.selection_buffer.upload(rng.integers(0, 2 ** 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32))
            v.update_selection_highlight((1.0, 0.5, 0.0, 0.5))
        v.get_pass_timing()
        for pose in poses:
            v.update_camera(camera.orbit_pose(pose), size)
            v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(deg), False)
            v.render_frame(["m"])
            out.append(_observe(v, ["m"]))
    return out


def _case(name):
    from tests import golden_util

    default = dict(progressive=1, speculative=1, min_slab=64, first_slab_divisor=4)
    if name == "fixtures":
        return {fid: _fixture_frames(fid, default) for fid in golden_util.IDS}
    if name.startswith("repair"):
        return {name: _fixture_frames("large_2models_320x240", dict(min_slab=1024, first_slab_divisor=8), lanes=int(name[-1]), prior=True)}
    if name == "pods":
        return {f"sh{sh}_cov{cov}_deg{deg}": _orbit_frames(30000, 401 + 10 * sh + cov, (256, 176), sh, cov, deg) for sh, cov, deg in POD_KINDS}
    if name == "edit_highlight":
        out = {fid: _fixture_frames(fid, default) for fid in golden_util.IDS if "edit" in fid}
        out["orbit"] = _orbit_frames(30000, 402, (256, 176), edit=True)
        return out
    if name == "wide":  # 260 x 3 tiles: above 255 tiles in one dimension the projection writes whole `a` records, no rect8
        return {name: _orbit_frames(20000, 403, (260 * 16, 48), scale_mul=4.0)}
    raise SystemExit(f"unknown case {name}")


def _child(name, out_path):
    arrays, meta = {}, {}
    for sub, frames in _case(name).items():
        meta[sub] = []
        for k, (fb, stats, shade_launches) in enumerate(frames):
            arrays[f"{sub}/{k}"] = fb
            meta[sub].append(dict(stats=stats, shade_launches=shade_launches))
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


# ---- the test: both sides, compared ----
def _run_side(name, side, tmp_path):
    out = os.path.join(str(tmp_path), f"{name}_{side}.npz")
    env = dict(os.environ, GSX_SHORT_CHAIN=str(side))
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_short_chain", name, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, f"GSX_SHORT_CHAIN={side}, case {name}: " + p.stdout[-1500:] + p.stderr[-1500:]
    z = np.load(out)
    return z, json.loads(str(z["meta"]))


def _compare(name, tmp_path):
    (z0, m0), (z1, m1) = _run_side(name, 0, tmp_path), _run_side(name, 1, tmp_path)
    assert sorted(z0.files) == sorted(z1.files) and m0.keys() == m1.keys()
    for f in z0.files:
        if f != "meta":
            assert np.array_equal(z0[f], z1[f]), f"{name}: frame {f} differs between the two sides: L-inf {np.abs(z0[f] - z1[f]).max()}"
    for sub in m0:
        for k, (a, b) in enumerate(zip(m0[sub], m1[sub])):
            for sa, sb in zip(a["stats"], b["stats"]):
                assert sa["speculated"] == sb["speculated"]
                for field in STAT_FIELDS:
                    assert sa[field] == sb[field], f"{name}/{sub} frame {k}: {field} {sa[field]} (off) != {sb[field]} (on)"
    return m0, m1


def test_float64_fixtures_through_the_default_schedule(tmp_path):
    m0, m1 = _compare("fixtures", tmp_path)
    speculated = 0
    for sub in m1:
        for a, b in zip(m0[sub][1:], m1[sub][1:]):   # frames 2 and 3
            if all(s["speculated"] for s in b["stats"]):
                speculated += 1
                assert a["shade_launches"] > 0, f"{sub}: the serial side of a speculated frame shades in launches of its own"
                if "edit" not in sub:   # (frames with colour ops keep the serial order on both sides)
                    assert b["shade_launches"] == 0, f"{sub}: a speculated frame still launched a shading kernel with the switch on"
    assert speculated >= len(m1), "frames 2 and 3 of the fixtures should have been speculated"


@pytest.mark.parametrize("lanes", [1, 2])
def test_repair_round_with_work(lanes, tmp_path):
    m0, m1 = _compare(f"repair{lanes}", tmp_path)
    frames = m1[f"repair{lanes}"]
    assert sum(s["n_repair_tiles"] for f in frames[:lanes] for s in f["stats"]) > 0, "the windows came from another camera: tiles must need the repair round"
    assert all(s["speculated"] for f in frames for s in f["stats"])
    assert all(f["shade_launches"] == 0 for f in frames), "main and repair round shade in the sort's launches"
    assert all(f["shade_launches"] > 0 for f in m0[f"repair{lanes}"])


def test_every_pod_kind_on_speculated_frames(tmp_path):
    m0, m1 = _compare("pods", tmp_path)
    assert len(m1) == len(POD_KINDS)
    for sub in m1:
        assert all(s["speculated"] for f in m1[sub][1:] for s in f["stats"]), f"{sub}: frames after the first are speculated"
        assert all(f["shade_launches"] == 0 for f in m1[sub][1:]), sub
        assert all(f["shade_launches"] > 0 for f in m0[sub][1:]), sub


def test_stored_edit_and_highlight(tmp_path):
    _compare("edit_highlight", tmp_path)


def test_viewport_above_255_tiles(tmp_path):
    m0, m1 = _compare("wide", tmp_path)
    assert all(s["speculated"] for f in m1["wide"][1:] for s in f["stats"])
    assert all(f["shade_launches"] == 0 for f in m1["wide"][1:]) and all(f["shade_launches"] > 0 for f in m0["wide"][1:])


def test_serial_order_behind_the_switch():
    """the suites that pin the default side, with GSX_SHORT_CHAIN=0 (tests/test_gpu_switches.py does the same for the other switches)"""
    if os.environ.get("GSX_SWITCH_RERUN"):
        pytest.skip("already inside the rerun")
    env = dict(os.environ, GSX_SWITCH_RERUN="1", GSX_SHORT_CHAIN="0")
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "tests/test_gpu_golden.py", "tests/test_gpu_overflow.py",
                        "tests/test_gpu_speculation.py", "-k", "not long_run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, "GSX_SHORT_CHAIN=0: " + p.stdout[-1500:] + p.stderr[-500:]


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
