#!/usr/bin/env python3
"""What the depth test (gsx_viewer_set_depth_test) costs on cfg4's orbit (10 M Gaussians, SH-3, 1920x1080), one process, one GPU.

Eight modes, in alternating blocks of --block frames so that drift of the box hits them alike:
  off              no depth test (the headline schedule)
  cleared          GSX_DEPTH_LESS against a cleared buffer (all 1.0): the same pixels, the extra work of the test
  occluder         GSX_DEPTH_LESS against a box at view depth --box-depth over the middle quarter of the screen (half the width, half the height)
  occluder_upload  the same box, handed over from host memory EVERY frame (gsx_viewer_upload_depth_buffer: a copy and a wait)
  lines16          GSX_DEPTH_LESS against 16 measurement lines drawn by the library (gsx_viewer_set_overlay_lines), no caller buffer: what
                   a host that shows measurement lines does instead of occluder_upload.  On a viewer of its own (a second copy of the
                   model): an uploaded buffer stays with its viewer, and this row is the one without any
  gizmo_box1       GSX_DEPTH_LESS against one mask gizmo drawn by the library (gsx_viewer_set_mask_gizmos): a box around the scene with the
                   orbit's camera inside it, no caller buffer — what a host that shows a mask shape does instead of occluder_upload.  On
                   a viewer of its own, like lines16 (a third copy of the model)
  gizmo32          the same with 16 boxes and 16 ellipsoids spread through the scene (3264 records)
  gizmo32_flat     gizmo32 on a viewer created under GSX_OVERLAY_BATCH_BOXES=0: the raster walks every batch of records in every tile (a
                   fourth copy of the model)
The gizmo rows are left out when the library has no gsx_viewer_set_mask_gizmos (GSX_LIB names a build from before it).
cleared and occluder read a device buffer in place (gsx_viewer_set_depth_buffer_device, set once), as an app whose depth attachment is
device memory does: the buffer is read by every frame's first preprocess whether or not it changed.
The host waits for every frame (gsx_render_frame + gsx_sync), as the app does.  Prints ONE JSON line: fps per mode (median of its
blocks, and every block), and the ratios to `off`.

--inflight adds the loop that never waits (bench.py's `value` loop: a block of gsx_render_frame calls, one gsx_sync behind it) with one
and with two frames in flight, for off / cleared / occluder: rows `<mode>_unsync_fif1` and `<mode>_unsync_fif2`, their ratios to the
`off` row of the same loop, and what two frames in flight gain over one.  --inflight-only leaves the synchronised rows out.
GSX_LIB selects another build of the library (the parent commit's, for a same-box A/B: tools/ab_depth.sh interleaves the two).

    python tools/bench_depth.py [--blocks 6] [--block 120] [--warmup 60] [--inflight | --inflight-only]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wgpu_3dgs_viewer_app_amd import _lib, camera, mask, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import DepthCompare, GaussianDisplayMode, GaussianShDegree, HitPair, MultiModelViewer  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--blocks", type=int, default=6, help="blocks per mode")
    ap.add_argument("--block", type=int, default=120, help="frames per block")
    ap.add_argument("--warmup", type=int, default=60, help="frames per mode before the first timed block")
    ap.add_argument("--box-depth", type=float, default=3.0, help="view depth of the occluding box (the orbit's radius is 6; the scene saturates at ~4-5)")
    ap.add_argument("--inflight", action="store_true", help="add the unsynchronised rows with one and two frames in flight")
    ap.add_argument("--inflight-only", action="store_true", help="only those rows")
    a = ap.parse_args()
    a.inflight |= a.inflight_only

    import torch

    torch.zeros(1, device="cuda")   # (torch's lazy device initialisation fails behind gigabytes of libgsx allocations: first)
    _lib.MAY_LACK = frozenset({"gsx_viewer_set_mask_gizmos"})   # (a build from before the gizmos runs the other rows)
    gizmo_rows = hasattr(_lib.load(), "gsx_viewer_set_mask_gizmos") and not a.inflight_only
    n, sh, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh)
    viewers = []
    for k in range(1 if a.inflight_only else 4 if gizmo_rows else 2):   # (the second one is lines16's, then gizmo_box1's and gizmo32's, then gizmo32_flat's)
        if k == 3:
            os.environ["GSX_OVERLAY_BATCH_BOXES"] = "0"   # (read when the viewer is created)
        v = MultiModelViewer()
        os.environ.pop("GSX_OVERLAY_BATCH_BOXES", None)
        v.add_model("m", n)
        v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh), False)
        viewers.append(v)
    del g
    v, vl = viewers[0], viewers[min(1, len(viewers) - 1)]
    rng = np.random.default_rng(16)
    lines16 = np.concatenate([HitPair(p, p + rng.uniform(-1.5, 1.5, 3), rng.integers(60, 256, 4), 30.0) for p in rng.uniform(-2.0, 2.0, (16, 3))])
    B, E = mask.MaskShapeKind.Box, mask.MaskShapeKind.Ellipsoid

    def shape(kind, pos, scale, color):
        q = rng.normal(size=4)
        return mask.MaskShape(kind, np.float32(pos), np.float32(q / np.linalg.norm(q)), np.float32(scale), np.float32(color))

    gizmo_sets = {   # (the orbit's radius is 6: the box's half-extent of 8 keeps the camera inside it)
        "gizmo_box1": mask.gizmo_records([[mask.MaskShape(B, scale=np.float32([8.0, 8.0, 8.0]), color=np.float32([1.0, 0.8, 0.2, 0.6]))]], 30.0),
        "gizmo32": mask.gizmo_records([[shape(k, rng.uniform(-2.0, 2.0, 3), rng.uniform(0.3, 0.8, 3), rng.uniform(0.3, 1.0, 4))
                                        for k in (B, E) for _ in range(16)]], 30.0),
    }
    gizmo_sets["gizmo32_flat"] = gizmo_sets["gizmo32"]
    orbit = [camera.PrecomputedCamera(camera.orbit_pose(k), w / h) for k in range(240)]
    p = np.asarray(orbit[0].projection(w / h), np.float32).reshape(16)
    box = np.float32(np.float32(p[14]) / np.float32(a.box_depth) - np.float32(p[10]))   # the NDC depth a surface there writes
    cleared = np.ones((h, w), np.float32)
    occluder = cleared.copy()
    occluder[h // 4: 3 * h // 4, w // 4: 3 * w // 4] = box
    dev = {"cleared": torch.from_numpy(cleared).cuda(), "occluder": torch.from_numpy(occluder).cuda()}
    torch.cuda.synchronize()
    modes = {"off": None, "cleared": cleared, "occluder": occluder, "occluder_upload": occluder, "lines16": None}
    if gizmo_rows:
        modes.update({m: None for m in gizmo_sets})
    buffers = dict(modes)
    frame = [0]

    def select(mode: str):
        if mode == "lines16" or mode in gizmo_sets:
            vo = vl if mode == "lines16" else viewers[3] if mode == "gizmo32_flat" else viewers[2]
            vo.set_depth_test(DepthCompare.Less)
            if mode == "lines16":
                vo.update_hit_pairs(lines16)
            else:
                vo.set_mask_gizmos(gizmo_sets[mode])
            return vo
        v.set_depth_test(DepthCompare.Always if buffers[mode] is None else DepthCompare.Less)
        if mode in dev:
            v.set_depth_buffer_device(dev[mode].data_ptr(), w, h, 4 * w)
        elif buffers[mode] is not None:
            v.update_depth_buffer(buffers[mode])
        return v

    def run(mode: str, frames: int) -> float:
        viewers[0].set_render_options(frames_in_flight=1)   # (the --inflight rows leave two)
        v = select(mode)
        upload = mode == "occluder_upload"
        v.poll()
        t0 = time.perf_counter()
        for _ in range(frames):
            if upload:
                v.update_depth_buffer(occluder)
            v.update_camera(orbit[frame[0] % 240], (w, h))
            v.render_frame(["m"])
            v.poll()
            frame[0] += 1
        return frames / (time.perf_counter() - t0)

    def run_unsync(mode: str, fif: int, frames: int) -> float:
        viewers[0].set_render_options(frames_in_flight=fif)
        v = select(mode)
        v.poll()
        t0 = time.perf_counter()
        for _ in range(frames):
            v.update_camera(orbit[frame[0] % 240], (w, h))
            v.render_frame(["m"])
            frame[0] += 1
        v.poll()
        return frames / (time.perf_counter() - t0)

    unsync = [(m, fif) for fif in (1, 2) for m in ("off", "cleared", "occluder")] if a.inflight else []
    if a.inflight_only:
        modes = {}
    for m in modes:
        run(m, a.warmup)
    for m, fif in unsync:
        run_unsync(m, fif, a.warmup)
    fps = {m: [] for m in modes}
    fps_u = {f"{m}_unsync_fif{fif}": [] for m, fif in unsync}
    for _ in range(a.blocks):
        for m in modes:
            fps[m].append(run(m, a.block))
        for m, fif in unsync:
            fps_u[f"{m}_unsync_fif{fif}"].append(run_unsync(m, fif, a.block))
    viewers[0].set_render_options(frames_in_flight=1)
    stats = {}
    for m in modes:
        sv = select(m)
        sv.update_camera(orbit[0], (w, h))
        sv.render_frame(["m"])
        sv.poll()
        stats[m] = sv.frame_stats("m")
    viewers[0].set_depth_buffer_device(None, 0, 0, 0)
    for v in viewers:
        v.close()
    med = {m: statistics.median(x) for m, x in fps.items()}
    out = {
        "tool": "bench_depth", "config": a.config, "gaussians": n, "size": [w, h], "host_waits_per_frame": True,
        "lib": os.environ.get("GSX_LIB", "in-tree"),
        "fps": {m: round(x, 1) for m, x in med.items()},
        "fps_blocks": {m: [round(y, 1) for y in x] for m, x in fps.items()},
        "ratio_to_off": {m: round(med[m] / med["off"], 4) for m in modes},
        "lines16_over_cleared": round(med["lines16"] / med["cleared"], 4) if "lines16" in med else None,
        "lines16_over_occluder_upload": round(med["lines16"] / med["occluder_upload"], 4) if "lines16" in med else None,
        "pose0_stats": stats,
    }
    for m in gizmo_sets if gizmo_rows else ():
        for base in ("occluder_upload", "cleared", "lines16"):
            out[f"{m}_over_{base}"] = round(med[m] / med[base], 4)
    if gizmo_rows:
        out["gizmo32_over_gizmo32_flat"] = round(med["gizmo32"] / med["gizmo32_flat"], 4)
    if unsync:
        mu = {r: statistics.median(x) for r, x in fps_u.items()}
        out["unsync_fps"] = {r: round(x, 1) for r, x in mu.items()}
        out["unsync_fps_blocks"] = {r: [round(y, 1) for y in x] for r, x in fps_u.items()}
        out["unsync_ratio_to_off"] = {r: round(x / mu[f"off_unsync_fif{r[-1]}"], 4) for r, x in mu.items()}
        out["unsync_two_over_one"] = {m: round(mu[f"{m}_unsync_fif2"] / mu[f"{m}_unsync_fif1"], 4) for m in ("off", "cleared", "occluder")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
