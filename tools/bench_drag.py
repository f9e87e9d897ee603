#!/usr/bin/env python3
"""What a selection drag in texture mode (the app's default, app.rs:1454) costs on cfg4's orbit (10 M Gaussians, SH-3, 1920x1080), one
process, one GPU, in the loop that never waits (bench.py's `value` loop: a block of frames, one gsx_sync behind it).

Rows, in alternating blocks of --block frames so that drift of the box hits them alike, each with one and with two frames in flight:
  plain                no toolset
  drag_host            query.QueryToolset paints the stroke on the host and gsx_update_query_texture hands the texture over EVERY frame:
                       what a host that shows the stroke while it is drawn has to do without the library's toolset (the parent commit's
                       behaviour: that entry point is unchanged — GSX_LIB=<a parent build> runs this row and `plain` on the parent's library)
  drag_device          gsx_toolset_update_pos + gsx_toolset_render every frame
  plain_resolve        plain + gsx_resolve_rgba8_device every frame: what the resolve itself costs in this loop (it is ordered after the
                       lanes' frames, and their next frames after it)
  drag_host_resolve    drag_host + gsx_resolve_rgba8_device every frame (the host would still have to draw the stroke itself)
  drag_device_resolve  drag_device + gsx_resolve_rgba8_device every frame with the stroke overlay drawn by the resolve
The pointer runs round an ellipse in the middle of the viewport with the default 40 px brush; every block is one stroke (start, then one
update_pos per frame; the stroke is not ended, so every frame's query is None, as during the app's drag).  Prints ONE JSON line: fps per
row (median of its blocks, and every block) and the ratios.

    python tools/bench_drag.py [--blocks 6] [--block 120] [--warmup 60] [--rows plain,drag_host,...]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wgpu_3dgs_viewer_app_amd import _lib, camera, query, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import GaussianDisplayMode, GaussianShDegree, MultiModelViewer  # noqa: E402

ROWS = ("plain", "drag_host", "drag_device", "plain_resolve", "drag_host_resolve", "drag_device_resolve")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--blocks", type=int, default=6, help="blocks per row")
    ap.add_argument("--block", type=int, default=120, help="frames per block")
    ap.add_argument("--warmup", type=int, default=60, help="frames per row before the first timed block")
    ap.add_argument("--rows", default=",".join(ROWS))
    a = ap.parse_args()
    rows = [r for r in a.rows.split(",") if r]
    assert set(rows) <= set(ROWS), rows
    if "GSX_LIB" in os.environ and not any(r.startswith("drag_device") for r in rows):
        # the host rows on a build from before the toolset: it lacks the toolset's calls, and these rows make none of them
        _lib.MAY_LACK = frozenset(s for s in _lib.EXPORTS if s.startswith("gsx_toolset_") or s == "gsx_download_query_texture")

    import torch

    torch.zeros(1, device="cuda")   # (torch's lazy device initialisation fails behind gigabytes of libgsx allocations: first)
    n, sh, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh)
    v = MultiModelViewer()
    v.add_model("m", n)
    v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
    v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh), False)
    del g
    orbit = [camera.PrecomputedCamera(camera.orbit_pose(k), w / h) for k in range(240)]
    rgba8 = torch.empty((h, w), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bg = (C.c_float * 3)(0.1, 0.1, 0.1)
    host = query.QueryToolset((w, h))
    dev = query.DeviceQueryToolset(v) if any(r.startswith("drag_device") for r in rows) else None
    frame = [0]

    def pointer(k: int):
        t = 2.0 * math.pi * k / 120.0
        return (0.5 * w + 0.3 * w * math.cos(t), 0.5 * h + 0.3 * h * math.sin(t))

    def run(row: str, fif: int, frames: int) -> float:
        v.set_render_options(frames_in_flight=fif)
        resolve = row.endswith("_resolve")
        tool = host if row.startswith("drag_host") else dev if row.startswith("drag_device") else None
        if dev is not None:
            v.set_toolset_overlay((1.0, 0.4, 0.0, 0.5) if row == "drag_device_resolve" else (0, 0, 0, 0), (0, 0, 0, 0), 1.0)
        if tool is not None:
            tool.start(query.QueryToolsetTool.Brush, query.QuerySelectionOp.Add, pointer(0))
        v.poll()
        t0 = time.perf_counter()
        for k in range(frames):
            if tool is host:
                host.update_pos(pointer(k + 1))
                v.update_query_texture(host.texture)
            elif tool is not None:
                dev.update_pos(pointer(k + 1))
                dev.render()
            v.update_camera(orbit[frame[0] % 240], (w, h))
            v.render_frame(["m"])
            if resolve:
                _lib.check(v._L.gsx_resolve_rgba8_device(v._h, bg, 0, h, rgba8.data_ptr()))
            frame[0] += 1
        v.poll()
        fps = frames / (time.perf_counter() - t0)
        if tool is not None and tool is dev:   # the stroke is over: no overlay, no cursor for the rows that follow
            dev.end()
            dev.query()
        return fps

    cells = [(r, fif) for fif in (1, 2) for r in rows]
    for r, fif in cells:
        run(r, fif, a.warmup)
    fps = {f"{r}_fif{fif}": [] for r, fif in cells}
    for _ in range(a.blocks):
        for r, fif in cells:
            fps[f"{r}_fif{fif}"].append(run(r, fif, a.block))
    v.close()
    med = {k: statistics.median(x) for k, x in fps.items()}
    out = {
        "tool": "bench_drag", "config": a.config, "gaussians": n, "size": [w, h], "host_waits_per_frame": False,
        "lib": os.environ.get("GSX_LIB", "in-tree"), "blocks": a.blocks, "block": a.block,
        "fps": {k: round(x, 1) for k, x in med.items()},
        "fps_blocks": {k: [round(y, 1) for y in x] for k, x in fps.items()},
        "ratio_to_plain": {k: round(x / med[f"plain_fif{k[-1]}"], 4) for k, x in med.items()} if "plain" in rows else None,
        "ratio_to_plain_resolve": {k: round(x / med[f"plain_resolve_fif{k[-1]}"], 4) for k, x in med.items() if "_resolve_" in k} if "plain_resolve" in rows else None,
    }
    for fif in (1, 2):
        for suffix in ("", "_resolve"):
            d, hst = f"drag_device{suffix}_fif{fif}", f"drag_host{suffix}_fif{fif}"
            if d in med and hst in med:
                out[f"drag_device{suffix}_over_drag_host{suffix}_fif{fif}"] = round(med[d] / med[hst], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
