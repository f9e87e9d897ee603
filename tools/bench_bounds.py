#!/usr/bin/env python3
"""What gsx_model_bounds costs on cfg4's model (10 M Gaussians), one process tree, one GPU, one call.

Six rows, each measured in two runs of alternating blocks (the spread between the two runs of a row is what a difference has to beat):
  1 reduce         k_bounds_reduce with filter 0                                                } HIP events around the launches,
  2 reduce_all     the same with mask, selection and stored edits present, all three flags set  } in tools/bench_bounds_kernels
  3 trim           the trimmed passes alone (k_bounds_hist + k_bounds_trim, 20 permille)         } (tools/bench_bounds.hip: the kernel
  4 mask_evaluate  k_mask_evaluate with a one-box program on the same plane: the yardstick      } files compiled as source; it
                                                                                                } adds `finish`: k_bounds_finish alone)
  5 bounds_call    the whole gsx_model_bounds call, host to host (filter 0, no trimming)
  6 download_numpy what a host does today for the same answer: gsx_model_download_pod + numpy min / max
Rows 1-4 run on the position plane of the model rows 5-6 use (downloaded from the library into a temporary file).  Every GPU step is
wrapped in `timeout`.  Prints ONE JSON line: milliseconds per row and run, the fraction of the 8 TB/s peak rows 1-3 reach on
16 B x n (plus the three bit planes for row 2), and the two bars:
  reduce_vs_mask_evaluate   row 1 is no slower than row 4 by more than the spread between the two runs of row 4
  call_vs_download          row 5 beats row 6 by more than both spreads

    python tools/bench_bounds.py [--config cfg4] [--blocks 6] [--reps 20] [--host-reps 2]
"""
from __future__ import annotations

import argparse
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

from wgpu_3dgs_viewer_app_amd import scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewer  # noqa: E402

KERNELS = os.path.join(ROOT, "tools", "bench_bounds_kernels")


def build_kernels() -> None:
    """the native half, on first use (a profiling tool must not fail the product's build)"""
    src = os.path.join(ROOT, "tools", "bench_bounds.hip")
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("kernels_bounds.hip", "kernels_mask.hip", "bounds_math.h", "extract_math.h", "gsx_internal.h")]
    if os.path.exists(KERNELS) and all(os.path.getmtime(KERNELS) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                           "-I" + os.path.join(ROOT, "include"), "-o", KERNELS])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--blocks", type=int, default=6, help="blocks per row and run")
    ap.add_argument("--reps", type=int, default=20, help="calls per block of the kernel rows")
    ap.add_argument("--host-reps", type=int, default=2, help="calls per block of rows 5 and 6")
    ap.add_argument("--kernel-timeout", type=int, default=240, help="seconds the native half may take")
    a = ap.parse_args()
    build_kernels()
    n, sh, _, _, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh)
    out = dict(tool="bench_bounds", config=a.config, n=n, blocks=a.blocks)
    with MultiModelViewer() as v:  # raises without a GPU: there is nothing to measure then
        v.add_model("m", n)
        buf = v.models["m"].gaussian_buffers.gaussians_buffer
        buf.update_range(0, g)
        del g
        # ---- rows 1-4: the resident position plane, handed to the native half ----
        pos, color, _, _ = buf.download_pod()
        pc = np.empty((n, 4), np.float32)
        pc[:, :3] = pos
        pc[:, 3] = color.view(np.float32)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "pc.bin")
            pc.tofile(path)
            del pc
            r = subprocess.run(["timeout", "-k", "10", str(a.kernel_timeout), KERNELS, path, str(n), str(a.blocks), str(a.reps)],
                               capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"bench_bounds_kernels exited with {r.returncode}: {r.stderr.strip()}")
        kernels = json.loads(r.stdout.strip().splitlines()[-1])
        out.update({k: val for k, val in kernels.items() if k not in ("tool", "n", "blocks")})
        # ---- rows 5-6: host to host, alternating blocks, two runs ----
        model = v.models["m"]

        def bounds_call():
            return model.bounds()

        def download_numpy():
            p, _, _, _ = buf.download_pod()
            return p.min(axis=0), p.max(axis=0)

        b = bounds_call()
        lo, hi = download_numpy()
        assert np.array_equal(b.min, lo) and np.array_equal(b.max, hi) and b.count == n, "the two rows must give the same answer"
        assert np.allclose(kernels["box"], [*lo, *hi], rtol=1e-5), "the native half ran on another plane"
        rows = {"bounds_call": bounds_call, "download_numpy": download_numpy}
        med = {k: [] for k in rows}
        for _ in range(2):
            ms = {k: [] for k in rows}
            for _ in range(a.blocks):
                for k, fn in rows.items():
                    t0 = time.perf_counter()
                    for _ in range(a.host_reps):
                        fn()
                    ms[k].append((time.perf_counter() - t0) * 1e3 / a.host_reps)
            for k in rows:
                med[k].append(statistics.median(ms[k]))
        for k in rows:
            out[f"{k}_ms"] = [round(x, 5) for x in med[k]]
    spread = lambda k: abs(out[f"{k}_ms"][0] - out[f"{k}_ms"][1])  # noqa: E731
    best = lambda k: min(out[f"{k}_ms"])  # noqa: E731
    mean = lambda k: 0.5 * sum(out[f"{k}_ms"])  # noqa: E731
    out["spread_ms"] = {k: round(spread(k), 5) for k in ("reduce", "reduce_all", "trim", "mask_evaluate", "finish", "bounds_call", "download_numpy")}
    out["bars"] = {
        "reduce_vs_mask_evaluate": dict(reduce_ms=round(mean("reduce"), 5), mask_evaluate_ms=round(mean("mask_evaluate"), 5),
                                        allowed_ms=round(spread("mask_evaluate"), 5),
                                        met=bool(mean("reduce") <= mean("mask_evaluate") + spread("mask_evaluate"))),
        "call_vs_download": dict(bounds_call_ms=best("bounds_call"), download_numpy_ms=best("download_numpy"),
                                 margin_ms=round(spread("bounds_call") + spread("download_numpy"), 5),
                                 met=bool(max(out["bounds_call_ms"]) + spread("bounds_call") + spread("download_numpy") < best("download_numpy"))),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
