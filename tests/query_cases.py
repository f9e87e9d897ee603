"""Scenes, queries and the float64 side shared by tests/test_query_cpu.py and tests/test_gpu_query_paths.py (spec §7 "Query")."""
import numpy as np

import oracle
from oracle import spec_f64
from tests import common
from wgpu_3dgs_viewer_app_amd import camera, query

W, H = 176, 128
POSE = 12
HIT_COORDS = [(88.0, 64.0), (40.25, 100.75), (0.5, 0.5), (175.5, 127.5)]
# test_gpu_query_paths.test_hit_results_saturate_at_65536: more hits than the result buffer holds
CAP_N, CAP_SEED, CAP_SCALE, CAP_W, CAP_H, CAP_POSE, CAP_COORDS = 80000, 77, 400.0, 64, 48, 3, (32.0, 24.0)


def texture30(w=W, h=H, seed=2):
    """The random 30 % query texture of test_gpu_edit.test_selection_queries_and_ops."""
    return (np.random.default_rng(seed).random((h, w)) < 0.3).astype(np.uint8) * 200


def selection_queries(op=query.QuerySelectionOp.Set):
    """name -> (pod, texture): the four queries of test_selection_queries_and_ops; the rectangle's corners are inverted in y."""
    return {"rect": (query.QueryPod.rect((20.5, 90.0), (120.0, 10.25), op), None),
            "brush": (query.QueryPod.brush((30.0, 30.0), (150.0, 100.0), 14.5, op), None),
            "disc": (query.QueryPod.brush((60.0, 60.0), (60.0, 60.0), 25.0, op), None),
            "texture": (query.QueryPod.texture(op), texture30())}


def with_op(pod, op):
    return query.QueryPod(pod.kind, op, pod.p0, pod.p1, pod.radius)


def unpack_bits(words, n):
    i = np.arange(n)
    return ((np.asarray(words, np.uint32)[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def project_both(g, cam, w, h, mt=None, sh_kind=0, cov_kind=0, mask=None, size=1.0, display_mode=0, selection=None, sel_edit=None):
    """(frame, f32 C-oracle projection, float64 projection) of one model, both from the pod as the GPU holds it (round-tripped planes).
    mask: words.  The float64 side skips SH (no query reads the colour); selection (bool[n]) + sel_edit (dict) as spec_f64.project."""
    mt = mt or camera.ModelTransform()
    pos, color, sh, cov = oracle.convert_pod(g, sh_kind, cov_kind)
    f = common.oracle_frame(cam, w, h, mt, size=size, display_mode=display_mode)
    pr = oracle.project(f, pos, color, sh, cov, mask)
    p64 = spec_f64.project(cam.view(), cam.projection(w / h), w, h, pos, color, None, cov, mt.pos, mt.quat(), mt.scale, size=size,
                           display_mode=display_mode, sh_deg=0, mask=mask, selection=selection, sel_edit=sel_edit)
    return f, pr, p64


def measure(f, pr, p64, coords_list):
    """Largest differences between the f32 C oracle and the float64 spec: (|mean2d| px over the Gaussians visible in both;
    |q| / k^2 over those with q <= 2 k^2 at any of coords_list; |alpha| over the hits both sides return there).  alpha is the
    C oracle's own (oracle.query_hits); q, which it does not return, is restated with its fmaf chain (a float32 product is exact
    in float64, so float32(float64 product + addend) is the fused result up to a double rounding)."""
    vis = (pr["key"] != 0xFFFFFFFF) & p64["visible"]
    d_mean = float(np.abs(pr["mean2d"][vis].astype(np.float64) - p64["mean2d"][vis]).max())
    k2 = float(f.k2)
    d_q = d_a = 0.0

    def fmaf(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)

    for c in coords_list:
        c32 = np.asarray(c, np.float32)
        dx, dy = c32[0] - pr["mean2d"][:, 0], c32[1] - pr["mean2d"][:, 1]
        co = pr["conic_opacity"]
        q32 = fmaf(co[:, 0] * dx, dx, fmaf(co[:, 2] * dy, dy, ((np.float32(2.0) * co[:, 1]) * dx) * dy))
        ex, ey = float(c32[0]) - p64["mean2d"][:, 0], float(c32[1]) - p64["mean2d"][:, 1]
        cn = p64["conic"]
        q64 = cn[:, 0] * ex * ex + cn[:, 2] * ey * ey + 2.0 * cn[:, 1] * ex * ey
        cand = vis & (q64 <= 2.0 * k2)
        if cand.any():
            d_q = max(d_q, float(np.abs(q32[cand].astype(np.float64) - q64[cand]).max()) / k2)
        hits = oracle.query_hits(f, pr, c, capacity=pr["key"].shape[0])
        idx, _, a64, _ = spec_f64.query_hits(p64, c, display_mode=int(f.display_mode))
        _, ia, ib = np.intersect1d(hits["index"], idx, return_indices=True)
        if ia.size:
            d_a = max(d_a, float(np.abs(hits["alpha"][ia].astype(np.float64) - a64[ib]).max()))
    return d_mean, d_q, d_a


def tolerance_scenes():
    """Every (scene, transform, pod, display mode, size, viewport, pose, hit coordinates) the query tests project: what QUERY_TOL,
    QUERY_TOL_Q and QUERY_TOL_ALPHA of oracle/spec_f64.py are measured over."""
    ident, odd = camera.ModelTransform(), common.odd_transform()
    out = []
    for n_a, n_b in ((40000, 40000), (40007, 18013)):          # the CPU tests' scenes; the GPU tests' models "a" and "b"
        for shk, cvk in ((0, 0), (2, 1)):
            out.append(dict(n=n_a, seed=31, scale=8.0, mt=ident, sh=shk, cov=cvk, mode=0, size=1.0, w=W, h=H, pose=POSE, coords=HIT_COORDS))
            out.append(dict(n=n_b, seed=32, scale=8.0, mt=odd, sh=shk, cov=cvk, mode=0, size=1.0, w=W, h=H, pose=POSE, coords=HIT_COORDS))
    for mode in (0, 1, 2):                                      # the hit queries' display modes at size 1.5
        out.append(dict(n=40007, seed=31, scale=8.0, mt=ident, sh=0, cov=0, mode=mode, size=1.5, w=W, h=H, pose=POSE, coords=HIT_COORDS))
        out.append(dict(n=18013, seed=32, scale=8.0, mt=odd, sh=0, cov=0, mode=mode, size=1.5, w=W, h=H, pose=POSE, coords=HIT_COORDS))
    out.append(dict(n=CAP_N, seed=CAP_SEED, scale=CAP_SCALE, mt=ident, sh=0, cov=0, mode=0, size=1.0, w=CAP_W, h=CAP_H, pose=CAP_POSE,
                    coords=[CAP_COORDS]))
    out.append(dict(n=6000, seed=35, scale=6.0, mt=ident, sh=0, cov=0, mode=0, size=1.0, w=W, h=H, pose=150,   # test_hit_query_and_positions
                    coords=[(88.0, 64.0), (40.25, 100.75)]))
    return out


def measure_scene(s):
    g = common.small_scene(s["n"], s["seed"], scale_mul=s["scale"])
    f, pr, p64 = project_both(g, camera.orbit_pose(s["pose"]), s["w"], s["h"], s["mt"], s["sh"], s["cov"], size=s["size"],
                              display_mode=s["mode"])
    return measure(f, pr, p64, s["coords"])
