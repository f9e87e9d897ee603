#!/usr/bin/env python3
"""What gsx_model_convert and gsx_model_set_pod_kind cost on cfg4's model (10 M Gaussians), one process tree, one GPU.

Two legs, Single/Single -> Norm8/Half and back.  Per leg the model is uploaded in the source kind, then:
  convert_ms       the whole gsx_model_convert call (filter 0), host to host, followed by a device synchronise; median of --reps,
                   the new model removed outside the timed window
  set_pod_kind_ms  the whole gsx_model_set_pod_kind call, host to host, followed by a device synchronise; median of --reps, the
                   model set back to the source kind outside the timed window
  create_ms        gsx_model_create of the destination kind alone (with its zero fill), then gsx_model_remove: what the calls and the host
                   route pay for the new planes; median of --reps
  host_ms          the host route of today: gsx_model_download_pod, gsx_model_create in the destination kind,
                   gsx_model_upload_pod_device (the planes staged on the device with torch); one run, with its parts
  frame_ms         a frame of the converted model beside a frame of the same Gaussians uploaded in the destination kind, the host
                   waiting for every frame as tools/bench_rows.py does; median of 10.  (From Single/Single the two models hold the same
                   bits; from Norm8/Half the converted model holds the decoded quantised values.)  No bar
  kernels          tools/bench_convert_kernels (tools/bench_convert.hip: the kernel files compiled as source, HIP events around the
                   launches): k_convert_kind for all 56 ordered pairs of kinds, keeping everything and keeping a random 3 in 100,
                   beside k_merge_bake for the source and the destination kind in the same process (run before and after the pairs),
                   and the two-kernel device route launch_unpack_pod + launch_pack_pod for the two legs
Every GPU child is wrapped in `timeout`.  Prints ONE JSON line; `bars.call_vs_host` holds host_ms / call_ms per leg and call (the bar:
the device call is faster in every row), `bars.kernel_pairs` the pairs whose bytes/s missed the lower of the two bake rates less
the baseline's spread, by kept set.

    python tools/bench_convert.py [--config cfg4] [--reps 3] [--kernel-reps 10]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from wgpu_3dgs_viewer_app_amd import _lib, camera, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, GaussianDisplayMode, GaussianShDegree, MultiModelViewer, MultiModelViewerModel, ShKind  # noqa: E402

KERNELS = os.path.join(ROOT, "tools", "bench_convert_kernels")
F32, N8H = (ShKind.Single, Cov3dKind.Single), (ShKind.Norm8, Cov3dKind.Half)
LEGS = {"f32_to_norm8_half": (F32, N8H), "norm8_half_to_f32": (N8H, F32)}


def build_native() -> None:
    """the native half, on first use (a profiling tool must not fail the product's build)"""
    csrc = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")
    src = os.path.join(ROOT, "tools", "bench_convert.hip")
    deps = [src] + [os.path.join(csrc, f) for f in ("kernels_extract.hip", "kernels_merge.hip", "kernels_convert.hip", "kernels_project.hip", "extract_math.h",
                                                    "merge_math.h", "pod_quant.h", "pod_planes.h", "pod_store.h", "gsx_internal.h")]
    if os.path.exists(KERNELS) and all(os.path.getmtime(KERNELS) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", src, "-I" + csrc,
                           "-I" + os.path.join(ROOT, "include"), "-o", KERNELS])


def note(*what) -> None:
    print("[bench_convert]", *what, file=sys.stderr, flush=True)


def run_native(cmd, timeout_s: int) -> str:
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s), *cmd], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{cmd[0]} exited with {r.returncode}: {r.stderr.strip()}")
    return r.stdout


def host_route(v, key, dst):
    """download_pod -> gsx_model_create in the destination kind -> gsx_model_upload_pod_device; milliseconds, host to host, and its parts"""
    import torch

    t0 = time.perf_counter()
    pos, color, sh, cov = v.models[key].gaussian_buffers.gaussians_buffer.download_pod()
    t1 = time.perf_counter()
    _lib.check(v._L.gsx_model_create(v._h, b"host", pos.shape[0], int(dst[0]), int(dst[1])))
    v.models["host"] = MultiModelViewerModel(v, "host")
    t2 = time.perf_counter()
    dev = [torch.from_numpy(a).cuda() for a in (pos, color.view("int32"), sh, cov)]
    torch.cuda.synchronize()
    v.models["host"].gaussian_buffers.gaussians_buffer.update_range_pod_device(0, pos.shape[0], *(t.data_ptr() for t in dev))
    v.poll()
    t3 = time.perf_counter()
    v.remove_model("host")
    return dict(host_ms=round((t3 - t0) * 1e3, 1), host_download_ms=round((t1 - t0) * 1e3, 1), host_create_ms=round((t2 - t1) * 1e3, 1),
                host_upload_ms=round((t3 - t2) * 1e3, 1))


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


def timed(v, reps, call, undo):
    ms = []
    for _ in range(reps):
        v.poll()
        t0 = time.perf_counter()
        call()
        v.poll()
        ms.append((time.perf_counter() - t0) * 1e3)
        undo()
    return dict(ms=round(statistics.median(ms), 4), ms_all=[round(x, 4) for x in ms])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per leg")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--kernel-timeout", type=int, default=300, help="seconds the native half may take")
    a = ap.parse_args()
    build_native()
    import torch  # (its HIP context comes up before the library's first viewer: the host route stages planes with it)

    torch.zeros(1, device="cuda")
    n, sh_deg, w, h, seed = scene.CONFIGS[a.config]
    g = scene.synthetic_gaussians(n, seed, sh_deg)
    out = dict(tool="bench_convert", config=a.config, n=n, reps=a.reps, legs={})
    for leg, (src, dst) in LEGS.items():
        with MultiModelViewer(sh=src[0], cov3d=src[1]) as v:  # raises without a GPU: there is nothing to measure then
            v.add_model("m", n)
            m = v.models["m"]
            m.gaussian_buffers.gaussians_buffer.update_range(0, g)
            m.convert("warm", *dst)  # (the workspace, the code objects)
            v.remove_model("warm")
            row = dict(convert=timed(v, a.reps, lambda: m.convert("d", *dst), lambda: v.remove_model("d")))
            row["set_pod_kind"] = timed(v, a.reps, lambda: m.set_pod_kind(*dst), lambda: m.set_pod_kind(*src))
            # what both calls (and the host route) pay for the destination's planes: gsx_model_create alone, the same way
            row["create"] = timed(v, a.reps, lambda: _lib.check(v._L.gsx_model_create(v._h, b"alloc", n, int(dst[0]), int(dst[1]))),
                                  lambda: _lib.check(v._L.gsx_model_remove(v._h, b"alloc")))
            row.update(host_route(v, "m", dst))
            note(leg, row)
            assert m.convert("c", *dst) == n and m.pod_kind == src
            _lib.check(v._L.gsx_model_create(v._h, b"loaded", n, int(dst[0]), int(dst[1])))
            v.models["loaded"] = MultiModelViewerModel(v, "loaded")
            v.models["loaded"].gaussian_buffers.gaussians_buffer.update_range(0, g)
            row["frame_ms"] = dict(converted=frame_ms(v, ["c"], (w, h)), loaded_in_destination_kind=frame_ms(v, ["loaded"], (w, h)))
            kind = (C.c_int32(), C.c_int32())
            _lib.check(v._L.gsx_model_pod_kind(v._h, b"c", C.byref(kind[0]), C.byref(kind[1])))
            assert (kind[0].value, kind[1].value) == (int(dst[0]), int(dst[1]))
            note(leg, row["frame_ms"])
        out["legs"][leg] = row
    out["kernels"] = json.loads(run_native([KERNELS, str(n), str(a.kernel_reps)], a.kernel_timeout).strip().splitlines()[-1])
    ratios = {f"{leg}/{call}": round(out["legs"][leg]["host_ms"] / out["legs"][leg][call]["ms"], 1) for leg in LEGS for call in ("convert", "set_pod_kind")}
    missed = {name: [pair for pair, r in p["pairs"].items() if not r["met"]] for name, p in out["kernels"]["patterns"].items()}
    out["bars"] = {"call_vs_host": dict(ratio=ratios, smallest=min(ratios.values()), met=bool(min(ratios.values()) > 1.0)),
                   "kernel_pairs": dict(missed=missed, met=not any(missed.values()))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
