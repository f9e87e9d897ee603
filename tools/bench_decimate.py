#!/usr/bin/env python3
"""What gsx_model_decimate costs on cfg4's model (10 M Gaussians), one process, one GPU.

For the f32 pod and for the Norm8 + Half pod:
  edges      gsx_model_decimate_edge for about 5 M, 1 M, 100 k and 1 k cells: the edge, its cell count, the search's time (20 count-only
             passes), once each
  rows       per edge: the whole gsx_model_decimate call into a new model, host to host, followed by a device synchronise; one
             warm-up call, then the median of --reps (the new model is removed between calls, outside the timed part); the count-only
             call the same way; the statistics
  floor      on the same model in the same process: gsx_model_select_neighbors with the finest edge as radius and a cap of 1 (the
             grid's four passes, a query that stops at the first neighbour, the select pass: the closest public call to "the grid
             alone") and gsx_model_extract of everything; a decimate whose cells are all singletons does the work of the grid and of
             the extract
  host       the host route for the 1 M edge, once, with its parts: gsx_model_download_pod, numpy over sorted cells (float32
             reduceat sums of the same moments), gsx_model_upload_pod_device
Prints ONE JSON line.

    python tools/bench_decimate.py [--config cfg4] [--reps 5] [--no-host-route]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wgpu_3dgs_viewer_app_amd import _lib, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402

TARGETS = (5_000_000, 1_000_000, 100_000, 1_000)
F = np.float32


def note(*what) -> None:
    print("[bench_decimate]", *what, file=sys.stderr, flush=True)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def numpy_decimate(pos, color, sh, cov, cell):
    """the host's way: cells from float32 coordinates, a stable sort by cell, reduceat over the runs; float32 moments as spec §22's
    (mass weights only: the bench scene has no empty cell masses)"""
    u = ((pos - pos.min(axis=0)) * (F(1) / F(cell))).astype(np.int64).clip(0, 32767)
    key = u[:, 0] | (u[:, 1] << 15) | (u[:, 2] << 30)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    starts = np.nonzero(np.concatenate([[True], skey[1:] != skey[:-1]]))[0]
    p, c, s = pos[order], cov[order], sh[order]
    rgba = np.stack([(color[order] >> (8 * k)) & 0xFF for k in range(4)], axis=1).astype(F)
    det = c[:, 0] * (c[:, 3] * c[:, 5] - c[:, 4] * c[:, 4]) - c[:, 1] * (c[:, 1] * c[:, 5] - c[:, 4] * c[:, 2]) + c[:, 2] * (c[:, 1] * c[:, 4] - c[:, 3] * c[:, 2])
    m = (rgba[:, 3] / F(255)) * np.sqrt(np.maximum(det, 0))
    run = np.repeat(np.arange(starts.size), np.diff(np.append(starts, skey.size)))
    d = p - p[starts][run]
    total = lambda a: np.add.reduceat(a, starts, axis=0)  # noqa: E731
    W = total(m)
    inv = (F(1) / np.where(W > 0, W, 1)).astype(F)
    e = total(m[:, None] * d) * inv[:, None]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov_out = np.stack([total(m * (c[:, q] + d[:, a] * d[:, b])) * inv - e[:, a] * e[:, b] for q, (a, b) in enumerate(pairs)], axis=1)
    rgb = np.clip(np.floor(total(m[:, None] * rgba[:, :3]) * inv[:, None] + F(0.5)), 0, 255).astype(np.uint32)
    sh_out = total(m[:, None] * s) * inv[:, None]
    d2 = cov_out[:, 0] * (cov_out[:, 3] * cov_out[:, 5] - cov_out[:, 4] ** 2) - cov_out[:, 1] * (cov_out[:, 1] * cov_out[:, 5] - cov_out[:, 4] * cov_out[:, 2]) + \
        cov_out[:, 2] * (cov_out[:, 1] * cov_out[:, 4] - cov_out[:, 3] * cov_out[:, 2])
    a = np.floor(np.minimum(1, W / np.sqrt(np.maximum(d2, 1e-38))) * F(255) + F(0.5)).astype(np.uint32)
    word = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16) | (a << 24)
    return (p[starts] + e).astype(F), word.astype(np.uint32), sh_out.astype(F), cov_out.astype(F)


def host_route(v, cell) -> dict:
    import torch

    buf = v.models["m"].gaussian_buffers.gaussians_buffer
    (pos, color, sh, cov), download_ms = timed(buf.download_pod)
    (p, w, s, c), numpy_ms = timed(lambda: numpy_decimate(pos, color, sh, cov, cell))

    def upload():
        v.add_model("host", p.shape[0])
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p, w.view(np.int32), s, c)]
        torch.cuda.synchronize()
        v.models["host"].gaussian_buffers.gaussians_buffer.update_range_pod_device(0, p.shape[0], *(t.data_ptr() for t in dev))
        v.poll()
    _, upload_ms = timed(upload)
    v.remove_model("host")
    return dict(host_ms=round(download_ms + numpy_ms + upload_ms, 1), host_download_ms=round(download_ms, 1), host_numpy_ms=round(numpy_ms, 1),
                host_upload_ms=round(upload_ms, 1), host_cells=int(p.shape[0]))


def median_ms(v, fn, reps, after=None):
    ms = []
    for k in range(reps + 1):  # (the first call warms the workspace and the code objects up)
        v.poll()
        t0 = time.perf_counter()
        r = fn()
        v.poll()
        ms.append((time.perf_counter() - t0) * 1e3)
        if after:
            after()
    return r, round(statistics.median(ms[1:]), 3), [round(x, 3) for x in ms]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row and pod")
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    import torch  # (its HIP context comes up before the library's first viewer: the host route stages planes with it)

    torch.zeros(1, device="cuda")
    n, sh_deg, _, _, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    out = dict(tool="bench_decimate", config=a.config, n=n, reps=a.reps, pods={})
    for pod, sh, cov in (("f32", ShKind.Single, Cov3dKind.Single), ("norm8_half", ShKind.Norm8, Cov3dKind.Half)):
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            m = v.models["m"]
            m.gaussian_buffers.gaussians_buffer.update_range(0, g)
            v.poll()
            edges, rows = {}, {}
            for target in TARGETS:
                (cell, cells), ms = timed(lambda: m.decimate_edge(target))
                edges[str(target)] = dict(cell=float(cell), cells=cells, search_ms=round(ms, 1))
                note(pod, "edge", target, edges[str(target)])
            for target in TARGETS:
                cell = F(edges[str(target)]["cell"])
                r, call_ms, every = median_ms(v, lambda: m.decimate("d", cell), a.reps, after=lambda: v.remove_model("d"))
                _, count_ms, _ = median_ms(v, lambda: m.decimate_count(cell), a.reps)
                rows[str(target)] = dict(cell=float(cell), cells=r.cells, singletons=r.singletons, largest_cell=r.largest_cell, call_ms=call_ms, call_ms_all=every,
                                         count_only_ms=count_ms)
                note(pod, "row", target, rows[str(target)])
            fine = float(edges[str(TARGETS[0])]["cell"])
            _, grid_ms, grid_all = median_ms(v, lambda: m.select_neighbors(fine, 0, 0, max_count=1), a.reps)
            _, extract_ms, extract_all = median_ms(v, lambda: m.extract("x"), a.reps, after=lambda: v.remove_model("x"))
            floor = dict(select_neighbors_cap1_ms=grid_ms, select_neighbors_all=grid_all, extract_ms=extract_ms, extract_all=extract_all,
                         floor_ms=round(grid_ms + extract_ms, 3))
            note(pod, "floor", floor)
            host = {} if a.no_host_route else host_route(v, F(edges["1000000"]["cell"]))
            note(pod, "host", host)
            out["pods"][pod] = dict(edges=edges, rows=rows, floor=floor, host_1M=host)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
