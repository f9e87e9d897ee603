#!/usr/bin/env python3
"""What the model clusters cost on cfg4's model (10 M Gaussians), one process tree, one GPU: gsx_model_clusters and
gsx_model_select_clusters whole, their passes alone beside gsx_model_neighbors' uncapped query on the same inputs, and the host
route of today.

  radii         tools/bench_neighbors.py's three radii: the median saturated neighbour count is about 2, 16 and 128
  calls/*       per radius, host to host followed by a device synchronise, median of --reps with every sample listed:
                gsx_model_clusters with labels and sizes (8 n bytes to the host), with the stats alone, gsx_model_select_clusters
                in its three modes (by size 1..4: debris; the largest; seeded, Add, from one selected Gaussian in 1024, uploaded
                outside the timed part), and gsx_model_neighbors with max_count 4095 and no counts; the stats of each radius
  passes        tools/bench_clusters_kernels (tools/bench_clusters.hip: the kernel files compiled as source, a HIP event between
                every two passes) on the scene's position elements: reset, reduce, cell, scan, scatter, the neighbours' query with
                max_count 4095, init, hook, label, stats, the three selects; hook_over_query per radius
  host/*        the host route at --host-n Gaussians (the first of the scene), in the same process on the same box:
                gsx_model_download_pod + tests/clusters_ref.py (grid_edges, components) + gsx_model_upload_selection of the largest
                cluster, beside both device calls on a model of those same Gaussians with the same radius (median count about 2)
Every GPU child is wrapped in `timeout`.  Prints ONE JSON line; `bars` holds host_ms / call_ms per host row (the bar: each device
call is faster than its host route in every row).

    python tools/bench_clusters.py [--config cfg4] [--reps 5] [--host-n 200000:3,1000000:1]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_neighbors as BN  # noqa: E402
from tests import clusters_ref as K  # noqa: E402
from tests import neighbors_ref as N  # noqa: E402
from wgpu_3dgs_viewer_app_amd import _lib, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402

KERNELS = os.path.join(ROOT, "tools", "bench_clusters_kernels")


def build_native() -> None:
    """the native half, on first use (a profiling tool must not fail the product's build)"""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    src = os.path.join(ROOT, "tools", "bench_clusters.hip")
    deps = [src] + [os.path.join(csrc, f) for f in ("kernels_clusters.hip", "kernels_neighbors.hip", "kernels_extract.hip", "clusters_math.h",
                                                    "neighbors_math.h", "extract_math.h", "pod_planes.h", "gsx_internal.h", "wave_reduce.h",
                                                    "selection_write.h", "neighbors_grid.h")]
    if os.path.exists(KERNELS) and all(os.path.getmtime(KERNELS) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                           "-I" + os.path.join(ROOT, "include"), "-o", KERNELS])


def note(*what) -> None:
    print("[bench_clusters]", *what, file=sys.stderr, flush=True)


def stats_only(v, key, radius):
    desc, out = _lib.ClusterDesc(0, 0, float(radius), 0), _lib.ClusterStats()
    _lib.check(v._L.gsx_model_clusters(v._h, key, C.byref(desc), None, None, C.byref(out)))
    return out


def seed_words(n):
    words = np.zeros((n + 31) // 32, np.uint32)
    words[::32] = 1  # one Gaussian in 1024
    return words


def timed_seeded(v, m, n, reps, r):
    """the seeded select, the seeds uploaded before every timed call"""
    words = seed_words(n)
    ms = []
    for _ in range(reps):
        m.gaussian_buffers.selection_buffer.upload(words)
        v.poll()
        t0 = time.perf_counter()
        m.select_clusters(r, K.SEEDED, op=K.ADD)
        v.poll()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row")
    ap.add_argument("--host-n", default="200000:3,1000000:1", help="n:reps of the host route, comma separated")
    ap.add_argument("--kernel-timeout", type=int, default=300, help="seconds the native half may take")
    a = ap.parse_args()
    build_native()
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    out = dict(tool="bench_clusters", config=a.config, n=n, reps=a.reps, radii={}, calls={}, host={})
    key = b"m"
    with MultiModelViewer(sh=ShKind.Remove, cov3d=Cov3dKind.Half) as v:  # raises without a GPU: there is nothing to measure then
        v.add_model("m", n)
        m = v.models["m"]
        m.gaussian_buffers.gaussians_buffer.update_range(0, g)
        pos, color = BN.download_positions(v, key, n)
        fin = pos[np.isfinite(pos).all(axis=1)]
        extent = np.percentile(fin, 95, axis=0) - np.percentile(fin, 5, axis=0)
        start = float(np.cbrt(np.prod(extent.astype(np.float64)) / n))  # the spacing of a uniform fill of the middle of the scene
        radii = {}
        for target in BN.TARGETS:
            r, med = BN.find_radius(v, key, start * (target / 4.0) ** (1.0 / 3.0), target)
            radii[target] = r
            out["radii"][str(target)] = dict(radius=r, median=med)
            note(f"target median {target}: radius {r:.6g}, median saturated count {med}")
        for target, r in radii.items():
            row = {}
            row["clusters/labels+sizes"] = BN.timed(v, a.reps, lambda: m.clusters(r))
            row["clusters/stats"] = BN.timed(v, a.reps, lambda: stats_only(v, key, r))
            row["select/by_size/1..4"] = BN.timed(v, a.reps, lambda: m.select_clusters(r, K.BY_SIZE, 1, 4))
            row["select/largest"] = BN.timed(v, a.reps, lambda: m.select_clusters(r, K.LARGEST))
            row["select/seeded"] = timed_seeded(v, m, n, a.reps, r)
            row["neighbors/hist/4095"] = BN.timed(v, a.reps, lambda: BN.stats_only(v, key, r, N.MAX_COUNT))
            st = stats_only(v, key, r)
            row["stats"] = dict(count=int(st.count), n_clusters=int(st.n_clusters), largest_size=int(st.largest_size), largest_label=int(st.largest_label))
            out["calls"][str(target)] = row
            note(target, row)
        # ---- the passes alone ----
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "pc.bin")
            np.concatenate([pos.view(np.uint32), color[:, None]], axis=1).astype(np.uint32).tofile(path)
            jobs = [f"{r:.9g}:0" for r in radii.values()]
            out["passes"] = json.loads(BN.run_native([KERNELS, path, str(n), str(a.reps), *jobs], a.kernel_timeout).strip().splitlines()[-1])
            note("passes", out["passes"])
        # ---- the host route, and the device calls at its n ----
        for spec in a.host_n.split(","):
            hn, hreps = (int(x) for x in spec.split(":"))
            hk = f"h{hn}"
            v.add_model(hk, hn)
            hm = v.models[hk]
            hm.gaussian_buffers.gaussians_buffer.update_range(0, g[:hn])
            hr, hmed = BN.find_radius(v, hk.encode(), start * (n / hn) ** (1.0 / 3.0) * 0.8, 2)
            last = {}

            def host_labels():
                p, _ = BN.download_positions(v, hk.encode(), hn)
                part = N.participates(p)
                last["c"] = K.of_labels(*K.components(hn, part, *K.grid_edges(p, part, hr)))
                return last["c"]

            def host_select():
                c = host_labels()
                pad = np.zeros(((hn + 31) // 32) * 32, bool)
                pad[:hn] = K.hits(c, K.LARGEST)
                hm.gaussian_buffers.selection_buffer.upload(np.packbits(pad, bitorder="little").view(np.uint32))

            row = dict(n=hn, radius=hr, median=hmed)
            row["host/clusters"] = BN.timed(v, hreps, host_labels)
            row["host/select"] = BN.timed(v, hreps, host_select)
            host_words = hm.gaussian_buffers.selection_buffer.download()
            row["clusters/labels+sizes"] = BN.timed(v, a.reps, lambda: hm.clusters(hr))
            row["select/largest"] = BN.timed(v, a.reps, lambda: hm.select_clusters(hr, K.LARGEST))
            # the device's answer and the host's agree
            got = hm.clusters(hr)
            row["labels_equal_host"] = bool(np.array_equal(got.labels, last["c"].labels) and np.array_equal(got.sizes, last["c"].sizes))
            row["selection_equals_host"] = bool(np.array_equal(hm.gaussian_buffers.selection_buffer.download(), host_words))
            out["host"][str(hn)] = row
            note("host", row)
    ratios = {}
    for hn, row in out["host"].items():
        ratios[f"{hn}/clusters"] = round(row["host/clusters"]["ms"] / row["clusters/labels+sizes"]["ms"], 1)
        ratios[f"{hn}/select"] = round(row["host/select"]["ms"] / row["select/largest"]["ms"], 1)
    out["bars"] = {"call_vs_host": dict(ratio=ratios, smallest=min(ratios.values()), met=bool(min(ratios.values()) > 1.0),
                                        missed=[k for k, x in ratios.items() if x <= 1.0])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
