#!/usr/bin/env python3
"""What gsx_model_merge costs on cfg4's model (10 M Gaussians), one process tree, one GPU.

Setup, for the f32 pod and for the Norm8 + Half pod: the model is cut into four pieces by box masks (four slabs along x, each
evaluated on the device and extracted with gsx_model_extract); the source is removed.  Three transform settings of the pieces:
`identity` (none moved), `three_baked` (three pieces given a rotation, a scale with a negative component and a translation: what a
host that moved pieces has) and `all_baked` (all four).
  call_ms      the whole gsx_model_merge call, host to host, followed by a device synchronise (the call itself returns once the
               copies are enqueued); median of --reps, the new model removed outside the timed window
  host_ms      what a host does today: gsx_model_download_pod of every piece, the bake in numpy (float32; positions, covariances,
               the SH product with matrices fitted in float64), gsx_model_create, gsx_model_upload_pod_device (the planes staged on
               the device with torch); one run per setting, with its download / bake / upload parts
  frame_ms     a frame of the four layered pieces against a frame of the merged model (`three_baked`), the host waiting for every
               frame as tools/bench_rows.py does; median of 10
  kernels      tools/bench_merge_kernels (tools/bench_merge.hip: the kernel files compiled as source, HIP events around the
               launches) on four sources of n / 4 that keep everything: keep, scan, the identity scatter, the bake, and the extract
               scatter of one whole model for the same bytes; bytes moved per second beside the runtime's device-to-device copy
  extract      tools/bench_extract_kernels (what tools/bench_extract.py reports), pattern `all`: k_extract_scatter on one model of n that
               keeps everything — the same bytes as the identity scatter — run in the same job
  bench_hbm    the copy rows of tools/bench_hbm, run in the same job
Every GPU child is wrapped in `timeout`.  Prints ONE JSON line; `bars.call_vs_host` holds host_ms / call_ms per pod and setting (the
bar: the device call is faster in every row), `bars.identity_vs_bench_extract` the identity scatter's rate over the rate
tools/bench_extract_kernels reports for the same bytes (the bar: within 10 %); `same_binary_ratio` beside it is the identity scatter
over `extract_whole`, the same kernel on one source inside bench_merge_kernels (no bar).

    python tools/bench_merge.py [--config cfg4] [--reps 3] [--kernel-reps 10]
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

from wgpu_3dgs_viewer_app_amd import _lib, camera, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.mask import MaskEvaluator, MaskOp, MaskShape, MaskShapeKind  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, GaussianDisplayMode, GaussianShDegree, MultiModelViewer, ShKind  # noqa: E402

KERNELS = os.path.join(ROOT, "tools", "bench_merge_kernels")
HBM = os.path.join(ROOT, "tools", "bench_hbm")
EXTRACT = os.path.join(ROOT, "tools", "bench_extract_kernels")
PIECES = ("p0", "p1", "p2", "p3")
QUAT = np.float32([1, 2, 3, 4]) / np.float32(np.sqrt(30.0))
MOVED = (np.float32([0.3, -0.2, 0.5]), QUAT, np.float32([1.3, -0.7, 0.9]))
IDENTITY = (np.zeros(3, np.float32), np.float32([0, 0, 0, 1]), np.ones(3, np.float32))
SETTINGS = {"identity": 0, "three_baked": 3, "all_baked": 4}  # pieces that are moved
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277, -0.5900435899266435)


def build_native() -> None:
    """the native halves, on first use (a profiling tool must not fail the product's build)"""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("kernels_extract.hip", "kernels_merge.hip", "extract_math.h", "merge_math.h", "pod_quant.h", "pod_planes.h", "gsx_internal.h")]
    for exe, src, dep in ((KERNELS, os.path.join(ROOT, "tools", "bench_merge.hip"), deps), (EXTRACT, os.path.join(ROOT, "tools", "bench_extract.hip"), deps),
                          (HBM, os.path.join(ROOT, "tools", "bench_hbm.hip"), [])):
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in [src] + dep):
            continue
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                               "-I" + os.path.join(ROOT, "include"), "-o", exe])


def quat_matrix(q) -> np.ndarray:
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def sh_basis(d) -> np.ndarray:
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([-SH_C1 * y, SH_C1 * z, -SH_C1 * x, SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy),
                     SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy), SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3 * yy)])


def sh_matrix(q) -> np.ndarray:
    """the 15 x 15 block-diagonal matrix of the three bands, fitted in float64 (spec §13's defining property), as float32"""
    R = quat_matrix(np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64)))
    d = np.random.default_rng(0).normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y, Z = sh_basis(d), sh_basis(d @ R.T)
    M = np.zeros((15, 15))
    for c0, m in ((0, 3), (3, 5), (8, 7)):
        M[c0:c0 + m, c0:c0 + m] = np.linalg.lstsq(Z[c0:c0 + m].T, Y[c0:c0 + m].T, rcond=None)[0]
    return M.astype(np.float32)


def numpy_bake(pos, sh, cov, mt):
    t, q, s = mt
    R = quat_matrix(q).astype(np.float32)
    pos = (pos * s) @ R.T + t
    M = R * s[None, :]
    S = cov[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    S = M @ S @ M.T
    cov = np.ascontiguousarray(S.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]])
    sh = np.einsum("jk,nkc->njc", sh_matrix(q), sh.reshape(-1, 15, 3)).reshape(-1, 45)
    return pos.astype(np.float32), np.ascontiguousarray(sh, np.float32), cov.astype(np.float32)


def host_round_trip(v, moved: int):
    """download_pod of every piece -> numpy bake of the moved ones -> concatenate -> gsx_model_create -> gsx_model_upload_pod_device;
    milliseconds, host to host, and its parts"""
    import torch

    t0 = time.perf_counter()
    pods = [v.models[k].gaussian_buffers.gaussians_buffer.download_pod() for k in PIECES]
    t1 = time.perf_counter()
    out = []
    for k, (pos, color, sh, cov) in enumerate(pods):
        if k < moved:
            pos, sh, cov = numpy_bake(pos, sh, cov, MOVED)
        out.append((pos, color.view(np.int32), sh, cov))
    planes = [np.concatenate([o[k] for o in out]) for k in range(4)]
    t2 = time.perf_counter()
    dst = v.add_model("host", planes[0].shape[0])
    dev = [torch.from_numpy(a).cuda() for a in planes]
    torch.cuda.synchronize()
    dst.gaussian_buffers.gaussians_buffer.update_range_pod_device(0, planes[0].shape[0], *(t.data_ptr() for t in dev))
    v.poll()
    t3 = time.perf_counter()
    v.remove_model("host")
    return dict(host_ms=round((t3 - t0) * 1e3, 1), host_download_ms=round((t1 - t0) * 1e3, 1), host_bake_ms=round((t2 - t1) * 1e3, 1),
                host_upload_ms=round((t3 - t2) * 1e3, 1))


def note(*what) -> None:
    print("[bench_merge]", *what, file=sys.stderr, flush=True)


def run_native(cmd, timeout_s: int) -> str:
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s), *cmd], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{cmd[0]} exited with {r.returncode}: {r.stderr.strip()}")
    return r.stdout


def frame_ms(v, keys, size) -> float:
    cam = camera.orbit_pose(10)

    def frame():
        v.update_camera(cam, size)
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
        v.render_frame(keys)
        v.poll()

    frame()
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        frame()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * statistics.median(ts), 3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per setting and pod")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-timeout", type=int, default=240, help="seconds each native half may take")
    a = ap.parse_args()
    build_native()
    import torch  # (its HIP context comes up before the library's first viewer: the host round trip stages planes with it)

    torch.zeros(1, device="cuda")
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    edges = np.quantile(g["pos"][:, 0].astype(np.float64), [0.0, 0.25, 0.5, 0.75, 1.0])
    out = dict(tool="bench_merge", config=a.config, n=n, reps=a.reps, pods={})
    for pod, sh, cov in (("f32", ShKind.Single, Cov3dKind.Single), ("norm8_half", ShKind.Norm8, Cov3dKind.Half)):
        rows = {}
        with MultiModelViewer(sh=sh, cov3d=cov) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
            ev = MaskEvaluator(v)
            sizes = []
            for k, key in enumerate(PIECES):  # four slabs along x (a Gaussian exactly on an edge lands in both neighbours)
                lo, hi = edges[k], edges[k + 1]
                box = MaskShape(MaskShapeKind.Box, pos=np.float32([(lo + hi) / 2, 0, 0]), scale=np.float32([(hi - lo) / 2, 1e6, 1e6]))
                ev.evaluate(MaskOp.parse("0"), "m", [box])
                sizes.append(v.models["m"].extract(key, _lib.GSX_BOUNDS_MASKED))
            v.remove_model("m")
            note(pod, "pieces", sizes)
            for name, moved in SETTINGS.items():
                for k, key in enumerate(PIECES):
                    v.update_model_transform(key, *(MOVED if k < moved else IDENTITY))
                v.merge("warm", PIECES)  # (the workspace, the code objects)
                v.remove_model("warm")
                ms = []
                for _ in range(a.reps):
                    v.poll()
                    t0 = time.perf_counter()
                    total, _ = v.merge("d", PIECES)
                    v.poll()
                    ms.append((time.perf_counter() - t0) * 1e3)
                    v.remove_model("d")
                assert total == sum(sizes)
                rows[name] = dict(total=total, call_ms=round(statistics.median(ms), 4), call_ms_all=[round(x, 4) for x in ms])
                rows[name].update(host_round_trip(v, moved))
                note(pod, name, rows[name])
            for k, key in enumerate(PIECES):
                v.update_model_transform(key, *(MOVED if k < 3 else IDENTITY))
            v.merge("merged", PIECES)
            rows["frame_ms"] = dict(layered_pieces=frame_ms(v, list(PIECES), (w, h)), merged=frame_ms(v, ["merged"], (w, h)))
        kernels = json.loads(run_native([KERNELS, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
        extract = json.loads(run_native([EXTRACT, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
        out["pods"][pod] = dict(pieces=sizes, kernels=kernels, bench_extract_all=extract["all"], **rows)
    out["bench_hbm_copy"] = [" ".join(ln.split()) for ln in run_native([HBM, str(n)], a.kernel_timeout).splitlines() if "copy" in ln]
    ratios = {f"{pod}/{name}": round(out["pods"][pod][name]["host_ms"] / out["pods"][pod][name]["call_ms"], 1) for pod in out["pods"] for name in SETTINGS}
    rates = {pod: round(out["pods"][pod]["kernels"]["identity_TBps"] / out["pods"][pod]["bench_extract_all"]["scatter_TBps"], 3) for pod in out["pods"]}
    same = {pod: round(out["pods"][pod]["kernels"]["identity_TBps"] / out["pods"][pod]["kernels"]["extract_whole_TBps"], 3) for pod in out["pods"]}
    out["bars"] = {"call_vs_host": dict(ratio=ratios, smallest=min(ratios.values()), met=bool(min(ratios.values()) > 1.0)),
                   "identity_vs_bench_extract": dict(ratio=rates, same_binary_ratio=same, met=bool(min(rates.values()) >= 0.9))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
