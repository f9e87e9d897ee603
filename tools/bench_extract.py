#!/usr/bin/env python3
"""What gsx_model_extract costs on cfg4's model (10 M Gaussians), one process tree, one GPU, one call.

For the f32 pod and for the Norm8 + Half pod, and for four keep patterns (`all`: everything, a plain copy; `first_half`: contiguous;
`p50`, `p03`: each Gaussian with probability 0.5 / 0.03):
  call_ms      the whole gsx_model_extract call with filter MASKED, host to host, followed by a device synchronise (the call itself
               returns once the copy is enqueued); median of --reps, the new model removed outside the timed window
  keep / scan / scatter_us and scatter_TBps
               each kernel alone, HIP events around its launches, in tools/bench_extract_kernels (tools/bench_extract.hip: the
               kernel file compiled as source), on planes of the same sizes; the scatter's algorithmic bytes per second = kept rows
               read plus kept rows written over every carried plane
  memcpy       the runtime's device-to-device copy of the same planes, and the copy rows of tools/bench_hbm, run in the same job
For the f32 pod only:
  host_ms      what a host does today for the same model: gsx_model_download_pod, numpy take, gsx_model_create,
               gsx_model_upload_pod_device (the planes staged on the device with torch); one run per pattern
Every GPU child is wrapped in `timeout`.  Prints ONE JSON line; `bars.call_vs_host` holds host_ms / call_ms per pattern (the bar: the
device call is faster for every pattern) and the smallest ratio.

    python tools/bench_extract.py [--config cfg4] [--reps 3] [--kernel-reps 10]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wgpu_3dgs_viewer_app_amd import _lib, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402

KERNELS = os.path.join(ROOT, "tools", "bench_extract_kernels")
HBM = os.path.join(ROOT, "tools", "bench_hbm")
PATTERNS = ("all", "first_half", "p50", "p03")


def build_native() -> None:
    """the native halves, on first use (a profiling tool must not fail the product's build)"""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    jobs = ((KERNELS, os.path.join(ROOT, "tools", "bench_extract.hip"), [os.path.join(csrc, f) for f in ("kernels_extract.hip", "extract_math.h", "merge_math.h", "pod_planes.h", "gsx_internal.h")]),
            (HBM, os.path.join(ROOT, "tools", "bench_hbm.hip"), []))
    for exe, src, deps in jobs:
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in [src] + deps):
            continue
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                               "-I" + os.path.join(ROOT, "include"), "-o", exe])


def keep_pattern(name: str, n: int) -> np.ndarray:
    if name == "all":
        return np.ones(n, bool)
    if name == "first_half":
        return np.arange(n) < n // 2
    return np.random.default_rng(PATTERNS.index(name)).random(n) < (0.5 if name == "p50" else 0.03)


def mask_words(keep: np.ndarray) -> np.ndarray:
    padded = np.zeros(((keep.size + 31) // 32) * 32, np.uint8)
    padded[:keep.size] = keep
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def host_round_trip(v, keep: np.ndarray) -> float:
    """download_pod -> numpy take -> gsx_model_create -> gsx_model_upload_pod_device; milliseconds, host to host"""
    import torch

    buf = v.models["m"].gaussian_buffers.gaussians_buffer
    t0 = time.perf_counter()
    pos, color, sh, cov = buf.download_pod()
    idx = np.nonzero(keep)[0]
    planes = [np.ascontiguousarray(a[idx]) for a in (pos, color.view(np.int32), sh, cov)]
    dst = v.add_model("host", idx.size)
    dev = [torch.from_numpy(a).cuda() for a in planes]
    torch.cuda.synchronize()
    dst.gaussian_buffers.gaussians_buffer.update_range_pod_device(0, idx.size, *(t.data_ptr() for t in dev))
    v.poll()
    ms = (time.perf_counter() - t0) * 1e3
    v.remove_model("host")
    return ms


def run_native(cmd, timeout_s: int) -> str:
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s), *cmd], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{cmd[0]} exited with {r.returncode}: {r.stderr.strip()}")
    return r.stdout


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per pattern and pod")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-timeout", type=int, default=240, help="seconds each native half may take")
    a = ap.parse_args()
    build_native()
    import torch  # (its HIP context comes up before the library's first viewer: the host round trip stages planes with it)

    torch.zeros(1, device="cuda")
    n, sh_deg, _, _, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    out = dict(tool="bench_extract", config=a.config, n=n, reps=a.reps, pods={})
    keeps = {name: keep_pattern(name, n) for name in PATTERNS}
    for pod, sh, cov in (("f32", ShKind.Single, Cov3dKind.Single), ("norm8_half", ShKind.Norm8, Cov3dKind.Half)):
        rows = {}
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            m = v.models["m"]
            m.gaussian_buffers.gaussians_buffer.update_range(0, g)
            for name in PATTERNS:
                m.gaussian_buffers.mask_buffer.upload(mask_words(keeps[name]))
                m.extract("warm", _lib.GSX_BOUNDS_MASKED)  # (the workspace, the code objects)
                v.remove_model("warm")
                ms = []
                for _ in range(a.reps):
                    v.poll()
                    t0 = time.perf_counter()
                    count = m.extract("d", _lib.GSX_BOUNDS_MASKED)
                    v.poll()
                    ms.append((time.perf_counter() - t0) * 1e3)
                    v.remove_model("d")
                assert count == int(keeps[name].sum())
                rows[name] = dict(kept=count, call_ms=round(statistics.median(ms), 4), call_ms_all=[round(x, 4) for x in ms])
                if pod == "f32":
                    rows[name]["host_ms"] = round(host_round_trip(v, keeps[name]), 2)
        kernels = json.loads(run_native([KERNELS, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
        for name in PATTERNS:
            rows[name].update({k: kernels[name][k] for k in ("keep_us", "scan_us", "scatter_us", "scatter_TBps")})
            rows[name]["kernels_kept"] = kernels[name]["kept"]  # (the native half draws its own random patterns)
        out["pods"][pod] = dict(bytes_per_gaussian=kernels["bytes_per_gaussian"], memcpy=kernels["memcpy"], **rows)
    out["bench_hbm_copy"] = [" ".join(ln.split()) for ln in run_native([HBM, str(n)], a.kernel_timeout).splitlines() if "copy" in ln]
    ratios = {name: round(out["pods"]["f32"][name]["host_ms"] / out["pods"]["f32"][name]["call_ms"], 1) for name in PATTERNS}
    out["bars"] = {"call_vs_host": dict(ratio=ratios, smallest=min(ratios.values()), met=bool(min(ratios.values()) > 1.0))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
