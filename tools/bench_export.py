#!/usr/bin/env python3
"""What gsx_model_export costs on cfg4's model (10 M Gaussians, SH 3), one process tree, one GPU.

For the f32 pod and for the Norm8 + Half pod, both row formats, keeping everything (`all`) and keeping 3 in 100 at random (`p03`, a
mask):
  kernels      (a) tools/bench_export_kernels (tools/bench_export.hip: the kernel files compiled as source, HIP events around the
               launch): k_export_rows alone, one launch over the model, rows into device memory; microseconds and algorithmic bytes
               per second (the SoA planes of the kept Gaussians read plus their rows written).  Beside it, from the same job:
               tools/bench_extract_kernels' scatter for the same patterns (the yardstick) and the copy rows of tools/bench_hbm
  call_ms      (b) the whole gsx_model_export call, host to host, into a pageable destination and into a pinned one (torch host tensors),
               median of --reps; `copy_ms`: the bare device-to-host copy of the same byte count into the same kind of memory
               (torch, one copy from a device tensor).  The bar: call_ms <= 1.15 x copy_ms
  host_ms      (c) the route the call replaces: gsx_model_download_pod, numpy.linalg.eigh of every covariance and the canonical
               quaternion (tests/export_ref.py's float64 path), the records, gsx_ply_write; one run, with its parts.  `all` is
               run for the f32 pod only unless --host-all-pods (it takes about a minute a pod)
Every GPU child is wrapped in `timeout`.  Prints ONE JSON line; `bars.kernel_vs_extract_scatter` holds (a) over the extract scatter's
rate per pod, pattern and format (the bar: at least 0.7), `bars.call_vs_copy` holds call_ms / copy_ms (the bar: at most 1.15).

    python tools/bench_export.py [--config cfg4] [--reps 3] [--kernel-reps 10] [--skip-host]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wgpu_3dgs_viewer_app_amd import _lib, ply, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402

KERNELS = os.path.join(ROOT, "tools", "bench_export_kernels")
HBM = os.path.join(ROOT, "tools", "bench_hbm")
EXTRACT = os.path.join(ROOT, "tools", "bench_extract_kernels")
FORMATS = {"gaussians": (_lib.GSX_EXPORT_GAUSSIANS, 224), "ply": (_lib.GSX_EXPORT_PLY_VERTICES, 248)}


def build_native() -> None:
    """the native halves, on first use (a profiling tool must not fail the product's build)"""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("kernels_extract.hip", "kernels_export.hip", "extract_math.h", "export_math.h", "edit_math.h", "pod_quant.h", "pod_planes.h",
                                            "gsx_internal.h")]
    for exe, src, dep in ((KERNELS, os.path.join(ROOT, "tools", "bench_export.hip"), deps), (EXTRACT, os.path.join(ROOT, "tools", "bench_extract.hip"), deps),
                          (HBM, os.path.join(ROOT, "tools", "bench_hbm.hip"), [])):
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in [src] + dep):
            continue
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                               "-I" + os.path.join(ROOT, "include"), "-o", exe])


def note(*what) -> None:
    print("[bench_export]", *what, file=sys.stderr, flush=True)


def run_native(cmd, timeout_s: int) -> str:
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s), *cmd], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{cmd[0]} exited with {r.returncode}: {r.stderr.strip()}")
    return r.stdout


def timed_calls(v, key, flt, fmt, dst_ptr, capacity, reps):
    desc = _lib.ExportDesc(flt, 0, fmt, 0, 0)
    count = C.c_uint64()
    call = lambda: _lib.check(v._L.gsx_model_export(v._h, key.encode(), C.byref(desc), dst_ptr, capacity, C.byref(count)))  # noqa: E731
    call()  # (the staging buffers, the code object, the destination's pages)
    ms = []
    for _ in range(reps):
        v.poll()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return int(count.value), ms


def timed_copies(torch, dev, dst, reps):
    """the bare device-to-host copy of dev (a uint8 device tensor) into dst (a uint8 host tensor, pageable or pinned)"""
    dst.copy_(dev)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dst.copy_(dev)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def host_route(v, key, mask_words):
    """download_pod -> eigh and the canonical form in float64 -> gsx_gaussian records -> gsx_ply_write (mask applied there)"""
    from tests import export_ref as E  # the float64 path the export is measured against

    t0 = time.perf_counter()
    pos, color, sh, cov = v.models[key].gaussian_buffers.gaussians_buffer.download_pod()
    t1 = time.perf_counter()
    rot, scale = E.solve_f64(cov)
    t2 = time.perf_counter()
    g = np.empty(pos.shape[0], scene.GAUSSIAN_DTYPE)
    g["rot"], g["pos"], g["scale"] = rot, pos, scale
    g["color"] = color.view(np.uint8).reshape(-1, 4)
    g["sh"] = sh.reshape(-1, 15, 3)
    t3 = time.perf_counter()
    data = ply.Gaussians(g).write_ply_array(mask_words)
    t4 = time.perf_counter()
    return dict(host_ms=round((t4 - t0) * 1e3, 1), host_download_ms=round((t1 - t0) * 1e3, 1), host_eigh_ms=round((t2 - t1) * 1e3, 1),
                host_records_ms=round((t3 - t2) * 1e3, 1), host_ply_write_ms=round((t4 - t3) * 1e3, 1), bytes=int(data.size))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per row")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-timeout", type=int, default=240, help="seconds each native half may take")
    ap.add_argument("--host-all-pods", action="store_true", help="run the host route on the whole model for every pod")
    ap.add_argument("--skip-host", action="store_true", help="leave the host route out (it does not depend on the library's kernels)")
    a = ap.parse_args()
    build_native()
    import torch  # (its HIP context comes up before the library's first viewer: the bare copies are its)

    torch.zeros(1, device="cuda")
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    keep = np.random.default_rng(103).random(n) < 0.03
    mask_words = np.packbits(np.pad(keep, (0, -n % 32)), bitorder="little").view(np.uint32)
    out = dict(tool="bench_export", config=a.config, n=n, reps=a.reps, pods={})
    cap = 248 * n
    pageable = torch.empty(cap, dtype=torch.uint8)
    pinned = torch.empty(cap, dtype=torch.uint8).pin_memory()
    dev = torch.empty(cap, dtype=torch.uint8, device="cuda")
    for pod, sh, cov in (("f32", ShKind.Single, Cov3dKind.Single), ("norm8_half", ShKind.Norm8, Cov3dKind.Half)):
        rows = {}
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
            v.models["m"].gaussian_buffers.mask_buffer.upload(mask_words)
            for pattern, flt in (("all", 0), ("p03", _lib.GSX_BOUNDS_MASKED)):
                for fname, (fmt, rb) in FORMATS.items():
                    row = {}
                    for kind, dst in (("pageable", pageable), ("pinned", pinned)):
                        count, ms = timed_calls(v, "m", flt, fmt, dst.data_ptr(), cap, a.reps)
                        copy = timed_copies(torch, dev[: count * rb], dst[: count * rb], a.reps)
                        row[kind] = dict(call_ms=round(statistics.median(ms), 3), call_ms_all=[round(x, 3) for x in ms],
                                         copy_ms=round(statistics.median(copy), 3), copy_ms_all=[round(x, 3) for x in copy])
                    row["kept"], row["bytes"] = count, count * rb
                    rows[f"{pattern}_{fname}"] = row
                    note(pod, pattern, fname, row)
                if not a.skip_host and (pattern == "p03" or pod == "f32" or a.host_all_pods):
                    rows[f"{pattern}_host"] = host_route(v, "m", mask_words if flt else None)
                    note(pod, pattern, "host route", rows[f"{pattern}_host"])
        kernels = json.loads(run_native([KERNELS, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
        extract = json.loads(run_native([EXTRACT, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
        out["pods"][pod] = dict(kernels=kernels, bench_extract={k: extract[k] for k in ("all", "p03")}, **rows)
    out["bench_hbm_copy"] = [" ".join(ln.split()) for ln in run_native([HBM, str(n)], a.kernel_timeout).splitlines() if "copy" in ln]
    kernel_ratio = {f"{pod}/{p}_{f}": round(out["pods"][pod]["kernels"][f"{p}_{f}"]["TBps"] / out["pods"][pod]["bench_extract"][p]["scatter_TBps"], 3)
                    for pod in out["pods"] for p in ("all", "p03") for f in FORMATS}
    call_ratio = {f"{pod}/{p}_{f}/{kind}": round(out["pods"][pod][f"{p}_{f}"][kind]["call_ms"] / out["pods"][pod][f"{p}_{f}"][kind]["copy_ms"], 3)
                  for pod in out["pods"] for p in ("all", "p03") for f in FORMATS for kind in ("pageable", "pinned")}
    out["bars"] = {"kernel_vs_extract_scatter": dict(ratio=kernel_ratio, smallest=min(kernel_ratio.values()), met=bool(min(kernel_ratio.values()) >= 0.7)),
                   "call_vs_copy": dict(ratio=call_ratio, largest=max(call_ratio.values()), met=bool(max(call_ratio.values()) <= 1.15))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
