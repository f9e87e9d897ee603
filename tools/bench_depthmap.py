#!/usr/bin/env python3
"""What gsx_render_depth_map costs on cfg4's model (10 M Gaussians, SH 3, 1920x1080), f32 and Norm8 + Half, one GPU, beside the
two kernels that walk the same complete per-tile lists: k_composite (a `progressive = 0` gsx_render_frame) and k_vis_tiles
(gsx_model_visibility).  Every round is a fresh child process (this program starts them) that builds the scene, warms up and times
host to host with a device synchronise behind every call; every sample is listed.

      frame/ms         one progressive = 0 gsx_render_frame([key]) — what the call runs first, per model
      frame/composite  the composite pass of that frame (k_composite over the complete per-tile lists; gsx_set_pass_timing)
      vis/walk         k_vis_tiles over the same lists, as the composite pass of gsx_model_visibility
      depth/none       gsx_render_depth_map with nothing downloaded (the planes stay on the device)
      depth/ndc        ... with GSX_DEPTH_MAP_NDC
      depth/walk       the walk alone (k_depth_tiles over the same lists), as the composite pass of the call
      depth/planes     the call with all six planes on the host (24 bytes a pixel)
      map              covered and crossed pixels, the surface range
Prints ONE JSON line.

    python tools/bench_depthmap.py [--config cfg4] [--reps 5] [--rounds 2]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (("f32", 0, 0), ("norm8+half", 2, 1))
KEY = "m"


def note(*what) -> None:
    print("[bench_depthmap]", *what, file=sys.stderr, flush=True)


def timed(v, reps, call):
    ms = []
    for _ in range(reps):
        v.poll()
        t0 = time.perf_counter()
        call()
        v.poll()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])


def pass_timed(v, reps, call):
    """the composite pass of `call`, by the library's own event pairs"""
    v.set_pass_timing(True, ["composite"])
    v.get_pass_timing()
    ms = []
    for _ in range(reps):
        call()
        ms.append(round(v.get_pass_timing()["composite"]["ms"], 4))
    v.set_pass_timing(False)
    return dict(ms=statistics.median(ms), ms_all=ms)


def child(a) -> dict:
    sys.path.insert(0, HERE)
    from wgpu_3dgs_viewer_app_amd import camera, scene
    from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, GaussianDisplayMode, GaussianShDegree, MultiModelViewer, ShKind

    out = {}
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    for name, sh, cov in KINDS:
        v = MultiModelViewer(sh=ShKind(sh), cov3d=Cov3dKind(cov))  # raises without a GPU: there is nothing to measure then
        with v:
            v.add_model(KEY, n)
            v.models[KEY].gaussian_buffers.gaussians_buffer.update_range(0, g)
            v.update_camera(camera.orbit_pose(0), (w, h))
            v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh_deg), False)
            v.set_render_options(progressive=0)
            m = v.models[KEY]
            for _ in range(2):
                v.render_frame([KEY])
                m.visibility(rows=False)
                v.render_depth_map([KEY], planes=False)
            row = {"frame/ms": timed(v, a.reps, lambda: v.render_frame([KEY])),
                   "frame/composite": pass_timed(v, a.reps, lambda: v.render_frame([KEY])),
                   "vis/walk": pass_timed(v, a.reps, lambda: m.visibility(rows=False)),
                   "depth/none": timed(v, a.reps, lambda: v.render_depth_map([KEY], planes=False)),
                   "depth/ndc": timed(v, a.reps, lambda: v.render_depth_map([KEY], ndc=True, planes=False)),
                   "depth/walk": pass_timed(v, a.reps, lambda: v.render_depth_map([KEY], planes=False)),
                   "depth/planes": timed(v, a.reps, lambda: v.render_depth_map([KEY]))}
            dm = v.render_depth_map([KEY], planes=False)
            vis = m.visibility(rows=False)
            row["map"] = dict(n_covered=dm.n_covered, n_crossed=dm.n_crossed, surface_min=float(dm.surface_min), surface_max=float(dm.surface_max),
                              pixels=w * h, n_pairs=vis.n_pairs, n_visible=vis.n_visible)
        out[name] = row
        note(name, row)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row and process")
    ap.add_argument("--rounds", type=int, default=2, help="child processes, one after the other")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a)))
        return
    out = dict(tool="bench_depthmap", config=a.config, reps=a.reps, rounds=[])
    for _ in range(a.rounds):
        # a fresh child process each (never a replaced one), under a time limit of its own; a failure ends the run
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", "--config", a.config, "--reps", str(a.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=HERE)
        sys.stderr.write(p.stderr)
        if p.returncode != 0:
            raise SystemExit(f"the child exited with {p.returncode}")
        out["rounds"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
