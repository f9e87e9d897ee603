#!/usr/bin/env python3
"""What the nearest search across models costs at 10 M queries against 10 M targets, one process, one GPU: gsx_model_nearest,
gsx_model_select_nearest and one gsx_model_align_step whole, host to host followed by a device synchronise, median of --reps with
every sample listed.

  kinds/*       f32 and Norm8 + Half (the position plane is float32 in both: the rows say whether anything else of the pod matters)
  order/*       the queries in the source's index order, for a source whose Gaussians lie in a random order ("shuffled": what a
                synthetic model is) and for the same Gaussians reordered on the host by the cell of a grid of the first search radius
                ("cells": what ordering the first list by the source's own grid on the device would give the walk, without the grid
                build it would cost).  The search itself is the same code in both: only the coherence of a wave's 64 queries differs
  calls         nearest/stats (nothing of n bytes crosses), nearest/rows (8 n bytes to the host), select/range, select/transfer,
                align/step; with each, what ran: first_radius, rounds, n_brute, n_found
  capped        the same with the source shifted by half the targets' box and max_distance = 4 x the first radius: half the queries have
                no target in reach and end as "none" in the last grid round.  (Without the cap this input is the worst there is: millions
                of queries beyond the box, too many for the fallback's budget, walk grids of growing cells until one reaches the box,
                10^13 distance tests a round; it is not timed here)
  host          the host route at --host-n (1 M), in numpy on the positions (gsx_model_export of both models is not timed): the targets
                sorted by grid cell, 27 cells a query, brute force for the queries no cell answers
Prints ONE JSON line.

    python tools/bench_nearest.py [--n 10000000] [--reps 3] [--host-n 1000000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_neighbors as BN  # noqa: E402
from wgpu_3dgs_viewer_app_amd import scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402


def note(*what) -> None:
    print("[bench_nearest]", *what, file=sys.stderr, flush=True)


def ran(st):
    return dict(count=st.count, targets=st.targets, n_found=st.n_found, mean=st.mean, d_max=float(st.d_max), first_radius=float(st.first_radius),
                rounds=st.rounds, n_brute=st.n_brute)


def calls(v, src, reps, **kw):
    row = {}
    row["nearest/stats"] = BN.timed(v, reps, lambda: src.nearest("dst", rows=False, **kw))
    row["nearest/rows"] = BN.timed(v, reps, lambda: src.nearest("dst", **kw))
    st = src.nearest("dst", rows=False, **kw)
    row["select/range"] = BN.timed(v, reps, lambda: src.select_nearest("dst", lo=0.0, hi=st.mean, **kw))
    row["select/transfer"] = BN.timed(v, reps, lambda: src.select_nearest("dst", transfer=True, **kw))
    row["align/step"] = BN.timed(v, reps, lambda: src.align_step("dst", **kw))
    row["ran"] = ran(st)
    return row


def by_cells(g, radius):
    """the Gaussians reordered by the cell of a grid of edge `radius` over their own box (x slowest)"""
    pos = g["pos"]
    c = np.floor((pos - pos.min(axis=0)) / np.float32(radius)).astype(np.int64)
    return g[np.lexsort((c[:, 2], c[:, 1], c[:, 0]))]


def host_nearest(q, t):
    """(index, d2, queries answered by brute force): every q's nearest t in numpy.  The targets are sorted by the cell of a grid whose
    edge h holds about eight of them; a query looks at the 27 cells around its own, one member of every cell a pass; a best distance
    within h is exact (anything nearer lies in the 27 cells), the rest are answered against all targets in chunks."""
    q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    lo, ext = t.min(axis=0), t.max(axis=0) - t.min(axis=0)
    h = np.float32(2.0 * (float(np.prod(ext.astype(np.float64))) / t.shape[0]) ** (1.0 / 3.0))
    dims = np.floor(ext / h).astype(np.int64) + 1
    key = lambda c: (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]  # noqa: E731
    tk = key(np.floor((t - lo) / h).astype(np.int64))
    order = np.argsort(tk, kind="stable")
    ts, tk = t[order], tk[order]
    cq = np.floor((q - lo) / h).astype(np.int64)
    best, index = np.full(q.shape[0], np.inf, np.float32), np.full(q.shape[0], -1, np.int64)
    for off in np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3):
        c = cq + off
        ok = ((c >= 0) & (c < dims)).all(axis=1)
        k = key(np.where(ok[:, None], c, 0))
        start, end = np.searchsorted(tk, k, "left"), np.searchsorted(tk, k, "right")
        end = np.where(ok, end, start)
        for j in range(int((end - start).max(initial=0))):
            live = np.nonzero(start + j < end)[0]
            at = start[live] + j
            d = ((q[live] - ts[at]) ** 2).sum(axis=1)
            better = d < best[live]
            best[live[better]], index[live[better]] = d[better], order[at[better]]
    left = np.nonzero(~(best <= h * h))[0]
    for a0 in range(0, left.size, 64):
        rows = left[a0:a0 + 64]
        d = ((q[rows, None, :] - t[None, :, :]) ** 2).sum(axis=2)
        index[rows] = d.argmin(axis=1)
        best[rows] = d[np.arange(rows.size), index[rows]]
    return index, best, int(left.size)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3, help="timed calls per row")
    ap.add_argument("--host-n", type=int, default=1_000_000)
    a = ap.parse_args()
    n, seed = a.n, scene.CONFIGS["cfg4"][4]
    src_g, dst_g = scene.synthetic_gaussians(n, seed, 0), scene.synthetic_gaussians(n, seed + 1, 0)
    out = dict(tool="bench_nearest", n=n, reps=a.reps, kinds={})
    sorted_g = None
    for name, sh, cov in (("f32", ShKind.Single, Cov3dKind.Single), ("norm8+half", ShKind.Norm8, Cov3dKind.Half)):
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            for key, g in (("src", src_g), ("dst", dst_g)):
                v.add_model(key, n)
                v.models[key].gaussian_buffers.gaussians_buffer.update_range(0, g)
            src = v.models["src"]
            v.models["dst"].select_nearest("src", lo=0.0, hi=src.nearest("dst", rows=False).mean)  # something to transfer
            row = {"shuffled": calls(v, src, a.reps)}
            note(name, "shuffled", row["shuffled"])
            first = row["shuffled"]["ran"]["first_radius"]
            if sorted_g is None:
                sorted_g = by_cells(src_g, first)
            src.gaussian_buffers.gaussians_buffer.update_range(0, sorted_g)
            row["cells"] = calls(v, src, a.reps)
            note(name, "cells", row["cells"])
            if name == "f32":
                box = float((dst_g["pos"].max(axis=0) - dst_g["pos"].min(axis=0)).max())
                move = np.eye(3, 4, dtype=np.float32)
                move[0, 3] = 0.5 * box
                out["capped"] = calls(v, src, a.reps, xform=move, max_distance=4.0 * first)
                note("capped", out["capped"])
            out["kinds"][name] = row
    m = a.host_n
    t0 = time.perf_counter()
    index, d2, left = host_nearest(src_g["pos"][:m], dst_g["pos"][:m])
    out["host"] = dict(n=m, route="numpy: targets sorted by cell, 27 cells a query, float32; chunked brute force for what no cell answers",
                       ms=round((time.perf_counter() - t0) * 1e3, 1), brute=left, mean=float(np.sqrt(d2).mean()))
    note("host", out["host"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
