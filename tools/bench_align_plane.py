#!/usr/bin/env python3
"""What a point-to-plane registration step costs at 10 M Gaussians against 10 M (cfg4's count, bench_nearest's two synthetic models),
one process, one GPU: every call whole, host to host followed by a device synchronise, median of --reps with every sample listed.

  normals       gsx_model_normals' statistics alone at k = 8 (nothing of n bytes crosses) against gsx_model_normals_keep: the same
                computation, and two device-to-device copies of 16 n bytes into the plane that stays
  step          one gsx_model_align_step (the yardstick: the same search, 12 doubles a pair) against one gsx_model_align_plane_step
                (two more gathers a pair: the 12-byte normal and the variation; 29 doubles), and the plane step with max_variation at
                the kept variations' median; with each, what ran: n_pairs, n_unfitted, rank, rounds, n_brute; ratio = plane / point
  kept          the bytes the plane adds (gsx_debug_device_bytes before and after the keep)
Prints ONE JSON line.

    python tools/bench_align_plane.py [--n 10000000] [--reps 5] [--k 8]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_neighbors as BN  # noqa: E402
import bench_normals as BNR  # noqa: E402
from wgpu_3dgs_viewer_app_amd import scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind, device_bytes  # noqa: E402


def note(*what) -> None:
    print("[bench_align_plane]", *what, file=sys.stderr, flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row")
    ap.add_argument("--k", type=int, default=8)
    a = ap.parse_args()
    n, seed = a.n, scene.CONFIGS["cfg4"][4]
    out = dict(tool="bench_align_plane", n=n, reps=a.reps, k=a.k)
    with MultiModelViewer(sh=ShKind.Remove, cov3d=Cov3dKind.Half) as v:  # raises without a GPU: there is nothing to measure then
        for key, s in (("src", seed), ("dst", seed + 1)):
            v.add_model(key, n)
            v.models[key].gaussian_buffers.gaussians_buffer.update_range(0, scene.synthetic_gaussians(n, s, 0))
        src, dst = v.models["src"], v.models["dst"]
        row = {"normals/stats": BN.timed(v, a.reps, lambda: BNR.stats_only(v, b"dst", a.k))}
        BNR.stats_only(v, b"dst", a.k)
        before = device_bytes()
        row["normals/keep"] = BN.timed(v, a.reps, lambda: dst.keep_normals(a.k))
        row["ratio"] = round(row["normals/keep"]["ms"] / row["normals/stats"]["ms"], 3)
        out["normals"] = row
        out["kept"] = dict(bytes=device_bytes() - before, per_gaussian=round((device_bytes() - before) / n, 2))
        note("normals", row, out["kept"])
        kept = dst.kept_normals()
        median = float(np.median(kept.variation[np.isfinite(kept.variation)]))
        del kept
        row = {"align/step": BN.timed(v, a.reps, lambda: src.align_step("dst")),
               "align_plane/step": BN.timed(v, a.reps, lambda: src.align_plane_step("dst")),
               "align_plane/step max_variation": BN.timed(v, a.reps, lambda: src.align_plane_step("dst", max_variation=median))}
        row["ratio"] = round(row["align_plane/step"]["ms"] / row["align/step"]["ms"], 3)
        st, sv = src.align_plane_step("dst"), src.align_plane_step("dst", max_variation=median)
        row["ran"] = dict(n_pairs=st.n_pairs, n_unfitted=st.n_unfitted, rank=st.rank, rounds=st.nearest.rounds, n_brute=st.nearest.n_brute,
                          rms_before=st.rms_before, rms_plane_before=st.rms_plane_before, max_variation=median, n_pairs_max_variation=sv.n_pairs,
                          n_unfitted_max_variation=sv.n_unfitted)
        out["step"] = row
        note("step", row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
