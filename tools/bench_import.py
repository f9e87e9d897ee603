#!/usr/bin/env python3
"""What gsx_model_import_ply costs on cfg4's model (10 M Gaussians, SH 3) as a canonical PLY file (2.48 GB), one process tree, one GPU.

The file is written once by the host writer into a temporary directory; every measurement below runs in a child process of its own
that reads it back into pageable memory (so that a route's peak host memory is its own), each wrapped in `timeout`:
  device    (a) `stream_ms`: gsx_model_upload_ply_rows of every row into an existing model, default staging: the chunk loop alone;
            `copy_ms`: the bare chunked host-to-device copy of the same bytes from the same pageable buffer through two device
            buffers of the same staging size (torch, one copy a chunk, one synchronise at the end), alternating with (a), `--reps` each.
            The bar: median stream_ms <= median copy_ms x (1 + 1 / chunks) + 3 x the standard deviation of copy_ms (the range of
            copy_ms is printed too).  `import_ms`: the whole gsx_model_import_ply call (header, model creation, rows);
            `create_ms` = import_ms - stream_ms, beside `add_model_ms` (gsx_model_create, which also zeroes the planes): allocation
            is reported, it is not part of the ratio
  host      (b) the route the parent commit offers: Gaussians.read_ply in one call, add_model, update_range, with its parts
  both report `peak_host_mb`: the growth of the process's resident peak over the route (the file itself is resident before it)
  kernels   (c) tools/bench_import_kernels (tools/bench_import.hip): k_import_rows alone, each read side, beside k_convert
Prints ONE JSON line.

    python tools/bench_import.py [--config cfg4] [--reps 5] [--kernel-reps 10] [--skip-host]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import resource
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wgpu_3dgs_viewer_app_amd import _lib, ply, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, MultiModelViewer, ShKind  # noqa: E402

KERNELS = os.path.join(ROOT, "tools", "bench_import_kernels")
DEFAULT_STAGING = 32 << 20
PODS = {"f32": (ShKind.Single, Cov3dKind.Single), "norm8_half": (ShKind.Norm8, Cov3dKind.Half)}


def build_native() -> None:
    """the native half, on first use (a profiling tool must not fail the product's build)"""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    src = os.path.join(ROOT, "tools", "bench_import.hip")
    deps = [src] + [os.path.join(csrc, f) for f in ("kernels_import.hip", "import_math.h", "pod_store.h", "pod_quant.h", "gsx_internal.h")]
    if os.path.exists(KERNELS) and all(os.path.getmtime(KERNELS) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                           "-I" + os.path.join(ROOT, "include"), "-o", KERNELS])


def note(*what) -> None:
    print("[bench_import]", *what, file=sys.stderr, flush=True)


def run_child(cmd, timeout_s: int) -> dict:
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s), *cmd], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd[:3])} exited with {r.returncode}: {r.stderr.strip()[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def peak_mb() -> float:
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def child_device(path: str, pod: str, reps: int) -> dict:
    import torch

    torch.zeros(1, device="cuda")
    data = np.fromfile(path, np.uint8)  # pageable
    header = ply.Gaussians.read_ply_header(data)
    raw, n = header.raw, header.count()
    body = data[raw.header_bytes: raw.header_bytes + n * raw.vertex_bytes]
    stage_rows = max(min(DEFAULT_STAGING // raw.vertex_bytes, n), 1)
    chunk = stage_rows * raw.vertex_bytes
    chunks = (body.size + chunk - 1) // chunk
    sh, cov = PODS[pod]
    out = dict(n=n, bytes=int(body.size), chunks=int(chunks), staging_bytes=DEFAULT_STAGING)
    src = torch.from_numpy(body)
    stage = [torch.empty(chunk, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def bare_copy():
        t0 = time.perf_counter()
        for c in range(chunks):
            piece = src[c * chunk: (c + 1) * chunk]
            stage[c & 1][: piece.numel()].copy_(piece)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        t0 = time.perf_counter()
        v.add_model("m", n)
        v.poll()
        out["add_model_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        buf = v.models["m"].gaussian_buffers.gaussians_buffer

        def stream():
            t0 = time.perf_counter()
            buf.update_range_ply(0, body, header)
            return (time.perf_counter() - t0) * 1e3

        bare_copy(), stream()  # (the staging buffers, the code object, the source's pages)
        base = peak_mb()
        copy_ms, stream_ms = [], []
        for _ in range(reps):  # alternating: what drifts on the machine drifts for both
            copy_ms.append(bare_copy())
            stream_ms.append(stream())
        import_ms = []
        for r in range(reps):
            t0 = time.perf_counter()
            got = v.import_ply(f"i{r}", data)
            import_ms.append((time.perf_counter() - t0) * 1e3)
            assert got == n
            v.remove_model(f"i{r}")
        out["peak_host_mb"] = round(peak_mb() - base, 1)
    med = statistics.median
    out.update(copy_ms=round(med(copy_ms), 3), copy_ms_all=[round(x, 3) for x in copy_ms], copy_ms_stdev=round(statistics.stdev(copy_ms), 3) if reps > 1 else 0.0,
               copy_ms_range=round(max(copy_ms) - min(copy_ms), 3), stream_ms=round(med(stream_ms), 3), stream_ms_all=[round(x, 3) for x in stream_ms],
               import_ms=round(med(import_ms), 3), import_ms_all=[round(x, 3) for x in import_ms], create_ms=round(med(import_ms) - med(stream_ms), 3))
    bar = out["copy_ms"] * (1.0 + 1.0 / chunks) + 3.0 * out["copy_ms_stdev"]
    out.update(bar_ms=round(bar, 3), ratio=round(out["stream_ms"] / out["copy_ms"], 4), met=bool(out["stream_ms"] <= bar))
    return out


def child_host(path: str, pod: str) -> dict:
    data = np.fromfile(path, np.uint8)
    sh, cov = PODS[pod]
    with MultiModelViewer(sh=sh, cov3d=cov) as v:
        base = peak_mb()
        t0 = time.perf_counter()
        g = ply.Gaussians.read_ply(data).gaussians
        t1 = time.perf_counter()
        v.add_model("m", g.shape[0])
        t2 = time.perf_counter()
        v.models["m"].gaussian_buffers.gaussians_buffer.update_range(0, g)
        t3 = time.perf_counter()
        return dict(host_ms=round((t3 - t0) * 1e3, 1), read_ply_ms=round((t1 - t0) * 1e3, 1), add_model_ms=round((t2 - t1) * 1e3, 1),
                    update_range_ms=round((t3 - t2) * 1e3, 1), peak_host_mb=round(peak_mb() - base, 1), n=int(g.shape[0]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per row")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds each child may take")
    ap.add_argument("--skip-host", action="store_true", help="leave the host route out")
    ap.add_argument("--child", choices=["device", "host"], help=argparse.SUPPRESS)
    ap.add_argument("--file", help=argparse.SUPPRESS)
    ap.add_argument("--pod", default="norm8_half", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_device(a.file, a.pod, a.reps) if a.child == "device" else child_host(a.file, a.pod)))
        return
    build_native()
    n, sh_deg, _, _, seed = scene.CONFIGS[a.config]
    out = dict(tool="bench_import", config=a.config, n=n, reps=a.reps, pods={})
    with tempfile.TemporaryDirectory(prefix="bench_import_") as tmp:
        path = os.path.join(tmp, "model.ply")
        ply.Gaussians(scene.synthetic_gaussians(n, seed, sh_deg)).write_ply_array().tofile(path)
        out["file_bytes"] = os.path.getsize(path)
        note("file", out["file_bytes"], "bytes")
        me = [sys.executable, os.path.abspath(__file__), "--file", path, "--reps", str(a.reps)]
        for pod, (sh, cov) in PODS.items():
            row = dict(device=run_child(me + ["--child", "device", "--pod", pod], a.timeout))
            note(pod, "device", row["device"])
            if not a.skip_host:
                row["host"] = run_child(me + ["--child", "host", "--pod", pod], a.timeout)
                note(pod, "host", row["host"])
            r = subprocess.run(["timeout", "-k", "10", str(a.timeout), KERNELS, str(n), str(int(sh)), str(int(cov)), str(a.kernel_reps)], capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"{KERNELS} exited with {r.returncode}: {r.stderr.strip()}")
            row["kernels"] = json.loads(r.stdout.strip().splitlines()[-1])
            note(pod, "kernels", row["kernels"])
            out["pods"][pod] = row
    out["bars"] = {"stream_vs_copy": {pod: dict(ratio=r["device"]["ratio"], bar_ms=r["device"]["bar_ms"], stream_ms=r["device"]["stream_ms"], met=r["device"]["met"])
                                      for pod, r in out["pods"].items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
