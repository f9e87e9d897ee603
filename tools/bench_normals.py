#!/usr/bin/env python3
"""What the model normals cost on cfg4's model (10 M Gaussians), one process, one GPU, against gsx_model_knn at the same k on the
same model in the same process: every call whole, host to host followed by a device synchronise, median of --reps with every sample
listed.

  calls/*       per k in 8, 16: gsx_model_knn's statistics alone (the yardstick: the same grid, rounds and fallback, values instead of
                keys, no fit), gsx_model_normals' statistics alone (nothing of n bytes crosses), with the normals and variations (16 n
                bytes to the host), with the indices as well (4 k n more bytes), the selection of the flat neighbourhoods; with each,
                what ran: first_radius, rounds, n_brute; and ratio = normals/stats over knn/stats
  toward        k = 8 oriented toward a point: the sign rule costs nothing that shows
Prints ONE JSON line.

    python tools/bench_normals.py [--config cfg4] [--reps 5] [--ks 8,16]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_knn as BK  # noqa: E402
import bench_neighbors as BN  # noqa: E402
from wgpu_3dgs_viewer_app_amd import _lib, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402


def note(*what) -> None:
    print("[bench_normals]", *what, file=sys.stderr, flush=True)


def stats_only(v, key, k, toward=None):
    desc = _lib.NormalsDesc(0, 0, int(k), 0 if toward is None else 1, 0.0, 0, 0, 0, (C.c_float * 3)(*(toward or (0.0, 0.0, 0.0))), 0)
    out = _lib.NormalsStats()
    _lib.check(v._L.gsx_model_normals(v._h, key, C.byref(desc), None, None, None, C.byref(out)))
    return out


def ran(st):
    return dict(count=int(st.count), n_fitted=int(st.n_fitted), mean=float(st.mean), first_radius=float(st.first_radius), rounds=int(st.rounds),
                n_brute=int(st.n_brute))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row")
    ap.add_argument("--ks", default="8,16")
    a = ap.parse_args()
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    out = dict(tool="bench_normals", config=a.config, n=n, reps=a.reps, calls={})
    key = b"m"
    with MultiModelViewer(sh=ShKind.Remove, cov3d=Cov3dKind.Half) as v:  # raises without a GPU: there is nothing to measure then
        v.add_model("m", n)
        m = v.models["m"]
        m.gaussian_buffers.gaussians_buffer.update_range(0, g)
        for k in (int(x) for x in a.ks.split(",")):
            row = {}
            row["knn/stats"] = BN.timed(v, a.reps, lambda: BK.stats_only(v, key, k))
            row["normals/stats"] = BN.timed(v, a.reps, lambda: stats_only(v, key, k))
            row["normals/arrays"] = BN.timed(v, a.reps, lambda: m.normals(k))
            row["normals/arrays+indices"] = BN.timed(v, a.reps, lambda: m.normals(k, indices=True))
            row["select/variation"] = BN.timed(v, a.reps, lambda: m.select_normals(k, 0.0, 0.01))
            row["ratio"] = round(row["normals/stats"]["ms"] / row["knn/stats"]["ms"], 3)
            row["ran"] = dict(normals=ran(stats_only(v, key, k)), knn=BK.ran(BK.stats_only(v, key, k)))
            out["calls"][str(k)] = row
            note(k, row)
        out["toward"] = BN.timed(v, a.reps, lambda: stats_only(v, key, 8, (0.0, 0.0, 100.0)))
        note("toward", out["toward"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
