#!/usr/bin/env python3
"""What the model properties cost on cfg4's model (10 M Gaussians), one process tree, one GPU: gsx_model_property_values,
gsx_model_histogram and gsx_model_select_range whole, beside the host route of today, and their kernel frame alone.

Two legs, a Single/Single and a Norm8/Half model.  Per leg, each call host to host followed by a device synchronise, median of --reps
with every sample listed:
  values/*      gsx_model_property_values (the kernel, the wait, 4 n bytes to the host)
  histogram/*   gsx_model_histogram: explicit range (one pass) and GSX_HIST_AUTO_RANGE (two), 256 and 4096 bins, the pc class and the scales
  select/*      gsx_model_select_range, Set
  host/*        the host route, in the same process on the same box: gsx_model_download_pod (positions, colour words, covariances: no SH)
                + numpy (np.histogram; a compare and np.packbits) + gsx_model_upload_selection.  For the scales the host route is
                charged the download alone: the eigen-solve of 10 M covariances on the host is left out, to the route's advantage
  kernels       tools/bench_property_kernels (tools/bench_property.hip: the kernel file compiled as source, HIP events around the
                launches): every mode of the frame for the pc class and the two covariance kinds, the histogram over a uniform
                property beside one whose values all fall into one bin
Every GPU child is wrapped in `timeout`.  Prints ONE JSON line; `bars` holds host_ms / call_ms per leg and call (the bar: the device
call is faster than its host route in every row).

    python tools/bench_property.py [--config cfg4] [--reps 5] [--kernel-reps 10]
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

KERNELS = os.path.join(ROOT, "tools", "bench_property_kernels")
VARIANTS = {"": []}
LEGS = {"single_single": (ShKind.Single, Cov3dKind.Single), "norm8_half": (ShKind.Norm8, Cov3dKind.Half)}
P = _lib


def build_native() -> None:
    """the native half, on first use (a profiling tool must not fail the product's build)"""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    src = os.path.join(ROOT, "tools", "bench_property.hip")
    deps = [src] + [os.path.join(csrc, f) for f in ("kernels_property.hip", "property_math.h", "export_math.h", "edit_math.h", "extract_math.h",
                                                    "pod_planes.h", "gsx_internal.h", "wave_reduce.h", "selection_write.h")]
    for suffix, flags in VARIANTS.items():
        exe = KERNELS + suffix
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            continue
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                               "-I" + os.path.join(ROOT, "include"), *flags, "-o", exe])


def note(*what) -> None:
    print("[bench_property]", *what, file=sys.stderr, flush=True)


def run_native(cmd, timeout_s: int) -> str:
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s), *cmd], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{cmd[0]} exited with {r.returncode}: {r.stderr.strip()}")
    return r.stdout


def timed(v, reps, call):
    ms = []
    for _ in range(reps):
        v.poll()
        t0 = time.perf_counter()
        call()
        v.poll()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])


def download(v, n):
    """gsx_model_download_pod without the SH plane: positions, colour words, covariances"""
    import ctypes as C

    pos, color, cov = np.empty((n, 3), np.float32), np.empty(n, np.uint32), np.empty((n, 6), np.float32)
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    _lib.check(v._L.gsx_model_download_pod(v._h, b"m", f32p(pos), color.ctypes.data_as(C.POINTER(C.c_uint32)), None, f32p(cov)))
    return pos, color, cov


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-timeout", type=int, default=120, help="seconds each build of the native half may take")
    a = ap.parse_args()
    build_native()
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    out = dict(tool="bench_property", config=a.config, n=n, reps=a.reps, legs={}, kernels={})
    for leg, (sh, cov) in LEGS.items():
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            m = v.models["m"]
            m.gaussian_buffers.gaussians_buffer.update_range(0, g)
            sb = m.gaussian_buffers.selection_buffer
            m.property_values(P.GSX_PROP_SCALE_MAX), m.histogram(P.GSX_PROP_POS_X, 4096), m.select_range(P.GSX_PROP_OPACITY, 0.0, 0.1)  # (workspace, code objects)
            row = {}
            for name, prop in (("pos_x", P.GSX_PROP_POS_X), ("hue", P.GSX_PROP_HUE), ("scale_max", P.GSX_PROP_SCALE_MAX)):
                row[f"values/{name}"] = timed(v, a.reps, lambda: m.property_values(prop))
            smax = m.property_values(P.GSX_PROP_SCALE_MAX)
            s_lo, s_hi = float(np.nanmin(smax)), float(np.nanmax(smax[np.isfinite(smax)]))
            for name, prop, lo, hi in (("opacity", P.GSX_PROP_OPACITY, 0.0, 1.0), ("pos_x", P.GSX_PROP_POS_X, -4.0, 4.0), ("scale_max", P.GSX_PROP_SCALE_MAX, s_lo, s_hi)):
                for bins in (256, 4096):
                    row[f"histogram/{name}/{bins}/explicit"] = timed(v, a.reps, lambda: m.histogram(prop, bins, lo, hi))
                    row[f"histogram/{name}/{bins}/auto"] = timed(v, a.reps, lambda: m.histogram(prop, bins))
                row[f"select/{name}"] = timed(v, a.reps, lambda: m.select_range(prop, lo, 0.5 * (lo + hi)))
            # ---- the host route ----
            def host_histogram():
                pos, color, cov = download(v, n)
                return np.histogram((color >> np.uint32(24)).astype(np.float32) / np.float32(255), 256, (0.0, 1.0))

            def host_select():
                pos, color, cov = download(v, n)
                hit = (color >> np.uint32(24)) <= np.uint32(127)
                pad = np.zeros(((n + 31) // 32) * 32, bool)
                pad[:n] = hit
                sb.upload(np.packbits(pad, bitorder="little").view(np.uint32))

            row["host/download_pod"] = timed(v, a.reps, lambda: download(v, n))
            row["host/histogram/opacity/256"] = timed(v, a.reps, host_histogram)
            row["host/select/opacity"] = timed(v, a.reps, host_select)
            # the device's answer and the host's agree
            hd, hh = m.histogram(P.GSX_PROP_OPACITY, 256, 0.0, 1.0), host_histogram()[0]
            row["histogram_count"] = int(hd.count)
            row["histogram_sum_equals_host"] = bool(int(hh.sum()) == int(hd.bins.sum()))
            note(leg, row)
        out["legs"][leg] = row
    for suffix in VARIANTS:
        out["kernels"]["as_built" if not suffix else suffix[1:]] = json.loads(
            run_native([KERNELS + suffix, str(n), str(a.reps), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
    ratios = {}
    for leg, row in out["legs"].items():
        for name, r in row.items():
            if not isinstance(r, dict) or name.startswith("host/"):
                continue
            host = row["host/download_pod"] if name.startswith("values/") or "scale_max" in name else (
                row["host/select/opacity"] if name.startswith("select/") else row["host/histogram/opacity/256"])
            ratios[f"{leg}/{name}"] = round(host["ms"] / r["ms"], 1)
    out["bars"] = {"call_vs_host": dict(ratio=ratios, smallest=min(ratios.values()), met=bool(min(ratios.values()) > 1.0),
                                        missed=[k for k, x in ratios.items() if x <= 1.0])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
