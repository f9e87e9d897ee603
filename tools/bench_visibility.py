#!/usr/bin/env python3
"""What gsx_model_visibility costs on cfg4's model (10 M Gaussians, SH 3, 1920x1080), f32 and Norm8 + Half, one GPU, beside a
`progressive = 0` gsx_render_frame of the same model ON THE PARENT COMMIT.  The two run in alternating child processes (this
program starts them: frame, calls, frame, calls, ...), each of which builds the scene, warms up and times host to host with a device
synchronise behind every call; every sample is listed.

  frame (the checkout given by --parent; only calls from before section 24)
      frame/ms        one progressive = 0 gsx_render_frame([key]) — what the visibility call runs first
      frame/composite the composite pass of that frame (k_composite over the complete per-tile lists; gsx_set_pass_timing)
  calls (this checkout)
      one/stats       gsx_model_visibility, the statistics alone (nothing of n bytes crosses)
      one/rows        ... with peak, weight and pixels on the host (16 n bytes)
      one/walk        the tile walk alone (k_vis_tiles over the same lists), as the composite pass of the call
      orbit8          visibility_orbit over 8 cameras: reset + 8 accumulated views, the statistics alone
      select          gsx_model_select_visibility, "never seen"
      seen            n_seen of the orbit, n_pairs and L_max of the last view
  host (this process, --host-n Gaussians at 1080p)
      the host route: a progressive = 0 frame, projection and tile lists downloaded, tests/visibility_ref.py's numpy walk
Prints ONE JSON line.

    python tools/bench_visibility.py --parent PATH [--config cfg4] [--reps 5] [--rounds 2] [--host-n 20000]
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
    print("[bench_visibility]", *what, file=sys.stderr, flush=True)


def timed(v, reps, call):
    ms = []
    for _ in range(reps):
        v.poll()
        t0 = time.perf_counter()
        call()
        v.poll()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])


def open_viewer(root, config, sh, cov, n_override=0):
    """a viewer of the checkout at `root` holding the config's model, camera set, progressive = 0 where a frame is drawn"""
    sys.path.insert(0, root)
    from wgpu_3dgs_viewer_app_amd import camera, scene
    from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, GaussianDisplayMode, GaussianShDegree, MultiModelViewer, ShKind

    n, sh_deg, w, h, seed = scene.CONFIGS[config]
    n = n_override or n
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    v = MultiModelViewer(sh=ShKind(sh), cov3d=Cov3dKind(cov))  # raises without a GPU: there is nothing to measure then
    v.add_model(KEY, n)
    v.models[KEY].gaussian_buffers.gaussians_buffer.update_range(0, g)
    v.update_camera(camera.orbit_pose(0), (w, h))
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh_deg), False)
    return v, camera, (w, h)


def child_frame(a) -> dict:
    out = {}
    for name, sh, cov in KINDS:
        v, camera, size = open_viewer(a.root, a.config, sh, cov)
        with v:
            v.set_render_options(progressive=0)
            for _ in range(2):
                v.render_frame([KEY])
            row = {"frame/ms": timed(v, a.reps, lambda: v.render_frame([KEY]))}
            v.set_pass_timing(True, ["composite"])
            v.get_pass_timing()
            ms = []
            for _ in range(a.reps):
                v.render_frame([KEY])
                ms.append(round(v.get_pass_timing()["composite"]["ms"], 4))
            row["frame/composite"] = dict(ms=statistics.median(ms), ms_all=ms)
        out[name] = row
        note("frame", a.root, name, row)
    return out


def child_calls(a) -> dict:
    out = {}
    for name, sh, cov in KINDS:
        v, camera, size = open_viewer(a.root, a.config, sh, cov)
        with v:
            from wgpu_3dgs_viewer_app_amd import _lib

            m = v.models[KEY]
            for _ in range(2):
                m.visibility(rows=False)
            row = {"one/stats": timed(v, a.reps, lambda: m.visibility(rows=False)), "one/rows": timed(v, a.reps, lambda: m.visibility())}
            v.set_pass_timing(True, ["composite"])
            v.get_pass_timing()
            ms = []
            for _ in range(a.reps):
                m.visibility(rows=False)
                ms.append(round(v.get_pass_timing()["composite"]["ms"], 4))
            v.set_pass_timing(False)
            row["one/walk"] = dict(ms=statistics.median(ms), ms_all=ms)
            cams = [camera.orbit_pose(30 * k) for k in range(8)]
            row["orbit8"] = timed(v, max(1, a.reps // 2), lambda: m.visibility_orbit(cams, size, rows=False))
            last = m.visibility_orbit(cams, size, rows=False)
            row["select"] = timed(v, a.reps, lambda: m.select_visibility(_lib.GSX_VIS_PEAK, 0.0, 0.0))
            row["seen"] = dict(n_seen=last.n_seen, views=last.views, n_pairs_last=last.n_pairs, n_visible_last=last.n_visible,
                               never=m.select_visibility(_lib.GSX_VIS_PEAK, 0.0, 0.0)[0])
        out[name] = row
        note("calls", name, row)
    return out


def host_route(a) -> dict:
    """the host route on a model small enough to finish: what an app without the call would do"""
    sys.path.insert(0, HERE)
    import oracle
    from tests import common
    from tests import visibility_ref as R

    v, camera, (w, h) = open_viewer(HERE, a.config, 0, 0, a.host_n)
    with v:
        v.set_render_options(progressive=0)
        t0 = time.perf_counter()
        v.render_frame([KEY])
        pr = v.download_projection(KEY)
        off, lst = v.download_tile_lists(KEY)
        t1 = time.perf_counter()
        f = common.oracle_frame(camera.orbit_pose(0), w, h)
        ref = R.walk(pr["mean2d"], pr["conic_opacity"], off, lst, w, h, f.k2, f.alpha_max, f.alpha_min, 1e-4, 0)
        t2 = time.perf_counter()
    del oracle
    return dict(n=a.host_n, route="progressive = 0 frame, projection and tile lists downloaded, numpy walk (tests/visibility_ref.py)",
                download_ms=round((t1 - t0) * 1e3, 1), walk_ms=round((t2 - t1) * 1e3, 1), entries=int(lst.size), l_max=ref.l_max, pairs=ref.n_pairs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row and process")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of (parent frame, this tree's calls)")
    ap.add_argument("--parent", default="", help="a checkout of the parent commit, built (empty: the frame rows come from this tree)")
    ap.add_argument("--host-n", type=int, default=20000)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)  # internal: frame | calls
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--child-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_frame(a) if a.child == "frame" else child_calls(a)))
        return
    out = dict(tool="bench_visibility", config=a.config, reps=a.reps, rounds=[], parent=bool(a.parent))
    for r in range(a.rounds):
        row = {}
        for mode, root in (("frame", a.parent or HERE), ("calls", HERE)):
            # a fresh child process each (never a replaced one), under a time limit of its own; a failure ends the run
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--config", a.config,
                   "--reps", str(a.reps)]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
            sys.stderr.write(p.stderr)
            if p.returncode != 0:
                raise SystemExit(f"{mode} child of {root} exited with {p.returncode}")
            row[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        out["rounds"].append(row)
    if a.host_n:
        out["host"] = host_route(a)
        note("host", out["host"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
