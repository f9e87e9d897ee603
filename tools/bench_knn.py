#!/usr/bin/env python3
"""What the nearest neighbours cost on cfg4's model (10 M Gaussians), one process, one GPU: gsx_model_knn and gsx_model_select_knn
whole, host to host followed by a device synchronise, median of --reps with every sample listed.

  calls/*       per k in 3, 8, 16: the scores alone (4 n bytes to the host), the statistics alone, the rows as well (4 k n more
                bytes), the outlier selection (nothing of n bytes crosses); with each, what ran: first_radius, rounds, n_brute
  outliers/*    the same model with one position in a thousand moved out to 100 x the box: the library's first radius comes from
                the box, so far outliers inflate it and with it the cells' population; the row says what that costs
  hint/*        k = 8 with the first radius halved and doubled: how flat the optimum is
  budget        a model of 2^17 Gaussians sent to the exact fallback whole (a tiny radius hint, max_rounds 1): U x P = 2^34
                distance tests, the most the budget rule lets a knob start: the longest kernel a call can be made to launch
                while a radius is left
Prints ONE JSON line.

    python tools/bench_knn.py [--config cfg4] [--reps 5]
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
from wgpu_3dgs_viewer_app_amd import _lib, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402


def note(*what) -> None:
    print("[bench_knn]", *what, file=sys.stderr, flush=True)


def stats_only(v, key, k, hint=0.0, max_rounds=0):
    desc, out = _lib.KnnDesc(0, 0, int(k), _lib.GSX_KNN_SCORE_MEAN, float(hint), 0, int(max_rounds), 0), _lib.KnnStats()
    _lib.check(v._L.gsx_model_knn(v._h, key, C.byref(desc), None, None, C.byref(out)))
    return out


def ran(st):
    return dict(count=int(st.count), n_scored=int(st.n_scored), mean=float(st.mean), std=float(st.std), first_radius=float(st.first_radius),
                rounds=int(st.rounds), n_brute=int(st.n_brute))


def rows_of(v, m, key, reps, ks, with_rows=True):
    out = {}
    for k in ks:
        row = {}
        row["knn/stats"] = BN.timed(v, reps, lambda: stats_only(v, key, k))
        row["knn/scores"] = BN.timed(v, reps, lambda: m.knn(k))
        if with_rows:
            row["knn/scores+rows"] = BN.timed(v, reps, lambda: m.knn(k, rows=True))
        row["select/outliers/2"] = BN.timed(v, reps, lambda: m.select_knn(k, std_ratio=2.0))
        row["ran"] = ran(stats_only(v, key, k))
        out[str(k)] = row
        note(k, row)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row")
    a = ap.parse_args()
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    out = dict(tool="bench_knn", config=a.config, n=n, reps=a.reps)
    key = b"m"
    with MultiModelViewer(sh=ShKind.Remove, cov3d=Cov3dKind.Half) as v:  # raises without a GPU: there is nothing to measure then
        v.add_model("m", n)
        m = v.models["m"]
        m.gaussian_buffers.gaussians_buffer.update_range(0, g)
        out["calls"] = rows_of(v, m, key, a.reps, (3, 8, 16))
        first = out["calls"]["8"]["ran"]["first_radius"]
        out["hint"] = {}
        for mul in (0.5, 2.0):
            st = stats_only(v, key, 8, first * mul)
            out["hint"][str(mul)] = dict(BN.timed(v, a.reps, lambda: stats_only(v, key, 8, first * mul)), ran=ran(st))
        note("hint", out["hint"])
        # one position in a thousand out at 100 x the box
        pos = g["pos"]
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        rng = np.random.default_rng(1)
        far = rng.choice(n, n // 1000, replace=False)
        g["pos"][far] = ((lo + hi) / 2 + (rng.random((far.size, 3)) - 0.5) * (hi - lo) * 100.0).astype(np.float32)
        m.gaussian_buffers.gaussians_buffer.update_range(0, g)
        out["outliers"] = rows_of(v, m, key, a.reps, (3, 8), with_rows=False)
        # the budget: 2^17 Gaussians, all through the exact fallback
        bn = 1 << 17
        v.add_model("b", bn)
        v.models["b"].gaussian_buffers.gaussians_buffer.update_range(0, scene.synthetic_gaussians(bn, seed, 0))
        st = stats_only(v, b"b", 16, 1e-20, 1)
        out["budget"] = dict(BN.timed(v, 3, lambda: stats_only(v, b"b", 16, 1e-20, 1)), ran=ran(st), tests=int(st.n_brute) * int(st.count))
        note("budget", out["budget"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
