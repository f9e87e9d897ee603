#!/usr/bin/env python3
"""What gsx_model_apply_transform costs on cfg4's model (10 M Gaussians), one process tree, one GPU.

For the f32 pod and for the Norm8 + Half pod, five rows — a kept set and a transform each:
  dense_full       everything kept, a rotation, a scale with a negative component, a translation, a pivot
  dense_translate  everything kept, a translation (positions only)
  random_1pc       a selection of one Gaussian in a hundred at random, the full transform
  run_1pc          a selection of one contiguous run of n / 100, the full transform
  box_half         a box mask over half of the model (evaluated on the device), the full transform
and per row
  call_ms    the whole gsx_model_apply_transform call, host to host, followed by a device synchronise; median of --reps (the
             transform is applied --reps + 1 times to the same model, which stays finite)
  device_ms  the route that exists without the call, once, with its parts: gsx_model_extract of the kept set, gsx_model_extract of
             the rest (inverted), gsx_update_model_transform of the first piece, gsx_model_merge of the two, two gsx_model_remove
             (for a dense row: no second piece).  Its result has another Gaussian order and neither mask nor selection
  host_ms    the host route, once, with its parts: gsx_model_download_pod, the bake of the kept rows in numpy (tools/bench_merge.py's),
             gsx_model_upload_pod_device
  kernels    tools/bench_transform_kernels_direct and _staged (tools/bench_transform.hip built once per record writer): k_transform_inplace
             alone on the four kept sets, beside k_merge_bake on the same Gaussians in the same binary
  merge      tools/bench_merge_kernels (what tools/bench_merge.py reports) in the same job: `baked_TBps` is the bar of the dense row
  bench_hbm  the copy rows of tools/bench_hbm, run in the same job (beside the translate row)
Every GPU child is wrapped in `timeout`.  Prints ONE JSON line; `bars` holds, per pod: in_place_vs_merge_bake (k_transform_inplace's
rate over k_merge_bake's, both everything kept; the bar: at least 0.9), sparse_faster_than_dense (call_ms of each sparse row below
the dense row's), call_vs_device and call_vs_host (the routes' times over the call's per row; the bar: above 1 in every row).

    python tools/bench_transform.py [--config cfg4] [--reps 5] [--kernel-reps 10]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_merge  # noqa: E402  (numpy_bake, the native halves it shares)
from wgpu_3dgs_viewer_app_amd import _lib, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator, MaskOp, MaskShape, MaskShapeKind  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402

KERNELS = {name: os.path.join(ROOT, "tools", "bench_transform_kernels_" + name) for name in ("direct", "staged")}
FULL = (np.float32([0.3, -0.2, 0.5]), bench_merge.QUAT, np.float32([1.3, -0.7, 0.9]))
TRANSLATE = (np.float32([0.3, -0.2, 0.5]), np.float32([0, 0, 0, 1]), np.ones(3, np.float32))
PIVOT = np.float32([0.7, -1.9, 0.3])
ROWS = ("dense_full", "dense_translate", "random_1pc", "run_1pc", "box_half")


def build_native() -> None:
    """the native halves, on first use (a profiling tool must not fail the product's build)"""
    bench_merge.build_native()
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    src = os.path.join(ROOT, "tools", "bench_transform.hip")
    deps = [src] + [os.path.join(csrc, f) for f in ("kernels_transform.hip", "kernels_merge.hip", "kernels_extract.hip", "transform_math.h", "merge_math.h",
                                                      "pod_quant.h", "pod_planes.h", "gsx_internal.h")]
    for staged, name in ((0, "direct"), (1, "staged")):
        exe = KERNELS[name]
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            continue
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", f"-DGSX_TRANSFORM_STAGED={staged}", src,
                               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", exe])


def note(*what) -> None:
    print("[bench_transform]", *what, file=sys.stderr, flush=True)


def words(flags) -> np.ndarray:
    b = np.asarray(flags, bool)
    padded = np.zeros(((b.size + 31) // 32) * 32, np.uint8)
    padded[:b.size] = b
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def device_route(v, flt, mt) -> dict:
    """extract + extract-inverted + update_model_transform + merge + two removes, each part followed by a device synchronise"""
    parts = {}

    def step(name, fn):
        def run():
            r = fn()
            v.poll()
            return r
        r, parts[name + "_ms"] = timed(run)
        return r

    kept = step("extract", lambda: v.models["m"].extract("piece", flt))
    rest = step("extract_inverted", lambda: v.models["m"].extract("rest", flt, invert=True))
    step("update_model_transform", lambda: v.update_model_transform("piece", *mt))
    keys = ["piece"] + (["rest"] if rest else [])
    total, _ = step("merge", lambda: v.merge("routed", keys))

    def removes():
        for key in keys:
            v.remove_model(key)
    step("removes", removes)
    v.remove_model("routed")  # (not part of the route: the result replaces the model)
    assert total == kept + rest
    return dict(device_ms=round(sum(parts.values()), 3), **{k: round(x, 3) for k, x in parts.items()})


def host_route(v, kept_rows, mt) -> dict:
    """download_pod -> the numpy bake of the kept rows -> upload_pod_device into the model; the pivot is not applied (it adds two
    float32 operations a coordinate)"""
    import torch

    buf = v.models["m"].gaussian_buffers.gaussians_buffer
    (pos, color, sh, cov), download_ms = timed(buf.download_pod)

    def bake():
        if kept_rows is None:
            return bench_merge.numpy_bake(pos, sh, cov, mt)
        p, s, c = bench_merge.numpy_bake(pos[kept_rows], sh[kept_rows], cov[kept_rows], mt)
        pos[kept_rows], sh[kept_rows], cov[kept_rows] = p, s, c
        return pos, sh, cov
    (p, s, c), bake_ms = timed(bake)

    def upload():
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p, color.view(np.int32), s, c)]
        torch.cuda.synchronize()
        buf.update_range_pod_device(0, p.shape[0], *(t.data_ptr() for t in dev))
        v.poll()
    _, upload_ms = timed(upload)
    return dict(host_ms=round(download_ms + bake_ms + upload_ms, 1), host_download_ms=round(download_ms, 1), host_bake_ms=round(bake_ms, 1),
                host_upload_ms=round(upload_ms, 1))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row and pod")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-timeout", type=int, default=240, help="seconds each native half may take")
    ap.add_argument("--no-host-route", action="store_true", help="leave the host route out (it takes most of the run)")
    a = ap.parse_args()
    build_native()
    import torch  # (its HIP context comes up before the library's first viewer: the host route stages planes with it)

    torch.zeros(1, device="cuda")
    n, sh_deg, _, _, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    rng = np.random.default_rng(20)
    selections = {"random_1pc": rng.random(n) < 0.01, "run_1pc": (np.arange(n) >= n // 3 + 517) & (np.arange(n) < n // 3 + 517 + n // 100)}
    x = g["pos"][:, 0].astype(np.float64)
    x_lo, x_mid = float(x.min()), float(np.median(x))
    out = dict(tool="bench_transform", config=a.config, n=n, reps=a.reps, pods={})
    for pod, sh, cov in (("f32", ShKind.Single, Cov3dKind.Single), ("norm8_half", ShKind.Norm8, Cov3dKind.Half)):
        rows = {}
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            buf = v.models["m"].gaussian_buffers
            buf.gaussians_buffer.update_range(0, g)
            box = MaskShape(MaskShapeKind.Box, pos=np.float32([(x_lo + x_mid) / 2, 0, 0]), scale=np.float32([(x_mid - x_lo) / 2, 1e6, 1e6]))  # x below the median
            MaskEvaluator(v).evaluate(MaskOp.parse("0"), "m", [box])
            box_rows = np.unpackbits(buf.mask_buffer.download().view(np.uint8), bitorder="little")[:n].astype(bool)
            for name in ROWS:
                mt = TRANSLATE if name == "dense_translate" else FULL
                flt = {"dense_full": 0, "dense_translate": 0, "box_half": _lib.GSX_BOUNDS_MASKED}.get(name, _lib.GSX_BOUNDS_SELECTED)
                kept_rows = None if flt == 0 else box_rows if name == "box_half" else selections[name]
                if name in selections:
                    buf.selection_buffer.upload(words(selections[name]))
                buf.gaussians_buffer.update_range(0, g)  # the planes as uploaded: every row starts from the same model
                model = v.models["m"]
                count = model.apply_transform(*mt, PIVOT, flt)  # (the workspace, the code objects)
                ms = []
                for _ in range(a.reps):
                    v.poll()
                    t0 = time.perf_counter()
                    model.apply_transform(*mt, PIVOT, flt)
                    v.poll()
                    ms.append((time.perf_counter() - t0) * 1e3)
                rows[name] = dict(kept=count, call_ms=round(statistics.median(ms), 4), call_ms_all=[round(x, 4) for x in ms])
                buf.gaussians_buffer.update_range(0, g)
                rows[name].update(device_route(v, flt, mt))
                if not a.no_host_route:
                    rows[name].update(host_route(v, kept_rows, mt))
                note(pod, name, rows[name])
        kernels = {name: json.loads(bench_merge.run_native([exe, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
                   for name, exe in KERNELS.items()}
        merge = json.loads(bench_merge.run_native([bench_merge.KERNELS, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
        out["pods"][pod] = dict(rows=rows, kernels=kernels, bench_merge_kernels=dict(baked_us=merge["baked_us"], baked_TBps=merge["baked_TBps"]))
    out["bench_hbm_copy"] = [" ".join(ln.split()) for ln in bench_merge.run_native([bench_merge.HBM, str(n)], a.kernel_timeout).splitlines() if "copy" in ln]
    library = "staged"  # the record writer the library is built with (csrc/kernels_transform.hip: GSX_TRANSFORM_STAGED)
    bars = {}
    for pod, p in out["pods"].items():
        rows, k = p["rows"], p["kernels"][library]
        vs_merge = round(k["full_all_TBps"] / p["bench_merge_kernels"]["baked_TBps"], 3)
        sparse = {name: bool(rows[name]["call_ms"] < rows["dense_full"]["call_ms"]) for name in ("random_1pc", "run_1pc", "box_half")}
        vs_device = {name: round(rows[name]["device_ms"] / rows[name]["call_ms"], 1) for name in ROWS}
        bars[pod] = dict(in_place_vs_merge_bake=dict(ratio=vs_merge, same_binary_ratio=k["full_vs_merge_bake"], met=bool(vs_merge >= 0.9)),
                         sparse_faster_than_dense=dict(rows=sparse, met=all(sparse.values())),
                         call_vs_device=dict(ratio=vs_device, met=bool(min(vs_device.values()) > 1.0)))
        if not a.no_host_route:
            vs_host = {name: round(rows[name]["host_ms"] / rows[name]["call_ms"], 1) for name in ROWS}
            bars[pod]["call_vs_host"] = dict(ratio=vs_host, met=bool(min(vs_host.values()) > 1.0))
    out["bars"] = bars
    print(json.dumps(out))


if __name__ == "__main__":
    main()
