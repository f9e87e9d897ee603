#!/usr/bin/env python3
"""What the plane of a model costs at 10 M Gaussians (cfg4's count and seed, a floor planted into the synthetic cloud: every third
Gaussian within 0.002 of z = 0), one process, one GPU: every call whole, host to host followed by a device synchronise, median of
--reps with every sample listed.  Per pod kind (the calls read the 16-byte position + colour element alone, whatever the kind):

  fit           gsx_model_fit_plane at H = 64, 256 and 1024 candidates, sampled from triples and from kept normals, without and with
                min_cos, with refine_iters 0 and 2; with each row what ran (n_valid, candidate_inliers, n_inliers, refine_done)
  score         the score alone: fit(H, TRIPLES, refine 0) minus fit(1, TRIPLES, refine 0), which runs the same participant and
                candidate passes and one plane; tests/s = n * (H - 1) / that
  select        gsx_model_select_plane, beside gsx_model_select_range over one coordinate: the one-pass streaming floor
  host          the same through the host: gsx_model_download_pod, then numpy's float32 residuals of H planes (f32 pod only; H = 64,
                one repetition: it takes seconds)
Prints ONE JSON line.

    python tools/bench_plane.py [--n 10000000] [--reps 5] [--k 8]
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
from wgpu_3dgs_viewer_app_amd import _lib, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402

TOL = 0.006
F = np.float32


def note(*what) -> None:
    print("[bench_plane]", *what, file=sys.stderr, flush=True)


def host_counts(pos, planes, tolerance):
    """the float32 residual rule of H planes over the downloaded positions, operation by operation"""
    out = np.zeros(len(planes), np.uint32)
    x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
    for h, (nx, ny, nz, off) in enumerate(planes):
        r = ((nx * x + ny * y) + nz * z) - off
        out[h] = int((np.abs(r) <= F(tolerance)).sum())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row")
    ap.add_argument("--k", type=int, default=8, help="the neighbours of the kept normals")
    a = ap.parse_args()
    n, seed = a.n, scene.CONFIGS["cfg4"][4]
    out = dict(tool="bench_plane", n=n, reps=a.reps, tolerance=TOL)
    g = scene.synthetic_gaussians(n, seed, 0)
    rng = np.random.default_rng(seed)
    floor = np.arange(n) % 3 == 0
    g["pos"][floor, 2] = rng.normal(0.0, 0.002, int(floor.sum())).astype(F)
    for name, sh, cov in (("f32", ShKind.Single, Cov3dKind.Single), ("norm8_half", ShKind.Norm8, Cov3dKind.Half)):
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            m = v.models["m"]
            m.gaussian_buffers.gaussians_buffer.update_range(0, g)
            row = {"keep_normals": BN.timed(v, 1, lambda: m.keep_normals(a.k))}
            fit = lambda **kw: m.fit_plane(TOL, rows=False, seed=7, **kw)  # noqa: E731
            fit(n_candidates=1024, refine_iters=2)  # (sizes the workspace)
            one = BN.timed(v, a.reps, lambda: fit(n_candidates=1, refine_iters=0))
            row["fit H=1 triples refine=0"] = one
            for H in (64, 256, 1024):
                for sample, sname in ((_lib.GSX_PLANE_SAMPLE_TRIPLES, "triples"), (_lib.GSX_PLANE_SAMPLE_NORMALS, "normals")):
                    for min_cos in (0.0, 0.9):
                        for refine in (0, 2):
                            kw = dict(n_candidates=H, sample=sample, min_cos=min_cos, refine_iters=refine)
                            t = BN.timed(v, a.reps, lambda: fit(**kw))
                            r = fit(**kw)
                            t["ran"] = dict(n_valid=r.n_valid, candidate_inliers=r.candidate_inliers, n_inliers=r.n_inliers, refine_done=r.refine_done,
                                            normal=[round(float(x), 5) for x in r.plane[:3]])
                            row[f"fit H={H} {sname} min_cos={min_cos} refine={refine}"] = t
                            if sample == _lib.GSX_PLANE_SAMPLE_TRIPLES and refine == 0:
                                ms = t["ms"] - one["ms"]
                                row[f"score H={H} min_cos={min_cos}"] = dict(ms=round(ms, 4), tests_per_s=round(n * (H - 1) / (ms * 1e-3), 0))
            best = fit(n_candidates=256, refine_iters=2)
            row["select_plane"] = BN.timed(v, a.reps, lambda: m.select_plane(best.plane, -TOL, TOL))
            row["select_plane min_cos=0.9"] = BN.timed(v, a.reps, lambda: m.select_plane(best.plane, -TOL, TOL, min_cos=0.9))
            row["select_range pos z"] = BN.timed(v, a.reps, lambda: m.select_range(_lib.GSX_PROP_POS_Z, -TOL, TOL))
            row["hit"] = dict(select_plane=m.select_plane(best.plane, -TOL, TOL)[0], n_inliers=best.n_inliers)
            if name == "f32":
                t0 = time.perf_counter()
                pos = m.gaussian_buffers.gaussians_buffer.download_pod()[0]
                t1 = time.perf_counter()
                cand = m.fit_plane(TOL, 64, seed=7, refine_iters=0)
                t2 = time.perf_counter()
                counts = host_counts(pos, cand.candidates, TOL)
                t3 = time.perf_counter()
                row["host H=64"] = dict(download_ms=round((t1 - t0) * 1e3, 1), numpy_ms=round((t3 - t2) * 1e3, 1), equal_counts=bool(np.array_equal(counts, cand.counts)))
                del pos
            out[name] = row
            note(name, row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
