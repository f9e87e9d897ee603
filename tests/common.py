"""Shared helpers for the parity tests: seeded scenes sized so the oracle finishes in seconds."""
import numpy as np

import oracle
from oracle.spec_f64 import quat_to_mat
from wgpu_3dgs_viewer_app_amd import camera, scene


def small_scene(n, seed, sh_degree=3, scale_mul=6.0):
    """Synthetic scene with enlarged splats so a small frame sees real overdraw."""
    g = scene.synthetic_gaussians(n, seed, sh_degree)
    g["scale"] *= np.float32(scale_mul)
    return g


def default_transform():
    return camera.ModelTransform()


def odd_transform():
    return camera.ModelTransform(pos=np.array([0.3, -0.2, 0.5], np.float32), rot=np.array([20, -35, 50], np.float32),
                                 scale=np.array([1.2, 0.9, 1.1], np.float32))


def cfg5_scene():
    """BASELINE configs[4] as the benchmark's cfg5 leg builds it: four models `a b c d` of n = CONFIGS["cfg5"][0] // 4 Gaussians (seeds
    seed + i), a TRS each, the `0 - 1` mask (box minus ellipsoid) for `a`, the stored rectangle selection (made at orbit pose 0) and
    the HSV edit of what it selected.  Returns a dict: n, sh, w, h, seeds, tr, mask_op, mask_shapes, rect, edit."""
    from wgpu_3dgs_viewer_app_amd import query
    from wgpu_3dgs_viewer_app_amd.mask import MaskOp, MaskShape, MaskShapeKind

    n_total, sh, w, h, seed = scene.CONFIGS["cfg5"]
    tr = {"a": camera.ModelTransform(pos=np.array([0.0, 0.0, 2.5], np.float32)),
          "b": camera.ModelTransform(pos=np.array([2.0, 0.2, -1.0], np.float32), rot=np.array([0, 35, 0], np.float32)),
          "c": camera.ModelTransform(pos=np.array([-2.5, -0.1, -0.5], np.float32), scale=np.array([0.9, 0.9, 0.9], np.float32)),
          "d": odd_transform()}
    shapes = [MaskShape(MaskShapeKind.Box, pos=np.array([0.0, 0.0, 2.5], np.float32), scale=np.array([3.0, 3.0, 3.0], np.float32)),
              MaskShape(MaskShapeKind.Ellipsoid, pos=np.array([0.0, 0.0, 2.5], np.float32), scale=np.array([1.5, 1.5, 1.5], np.float32))]
    return dict(n=n_total // 4, sh=sh, w=w, h=h, seeds={k: seed + i for i, k in enumerate(tr)}, tr=tr, mask_op=MaskOp.parse("0 - 1"),
                mask_shapes=shapes, rect=query.QueryPod.rect((1200.0, 600.0), (2600.0, 1500.0), query.QuerySelectionOp.Set),
                edit=query.GaussianEditPod(query.GaussianEditFlag.ENABLED, (0.5, 1.0, 1.2), 0.1, 0.2, 1.0, 0.9))


def surface_depth(cam, w, h, surfaces):
    """A Depth32Float buffer as the gizmos write it: per pixel centre, the NDC depth (clip.z / clip.w, float64, stored as f32) of
    the nearest surface the camera's ray hits; 1.0 (cleared) where none is hit.  surfaces: dict(kind "plane", point, normal) |
    dict(kind "box" | "ellipsoid", pos, quat, scale (half extents / radii))."""
    V = np.asarray(cam.view(), np.float64).reshape(4, 4).T
    P = np.asarray(cam.projection(w / h), np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:h, 0:w]
    nx, ny = (xs + 0.5) / w * 2.0 - 1.0, 1.0 - (ys + 0.5) / h * 2.0
    dv = np.stack([nx / P[0, 0], ny / P[1, 1], -np.ones_like(nx)], -1)      # view-space ray, view depth d = t
    R, t = V[:3, :3], V[:3, 3]
    origin = -R.T @ t
    dw = dv @ R                                                              # R^T dv per pixel
    best = np.full((h, w), np.inf)
    for s in surfaces:
        if s["kind"] == "plane":
            n = np.asarray(s["normal"], np.float64)
            den = dw @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                tt = ((np.asarray(s["point"], np.float64) - origin) @ n) / den
        else:
            Rs = quat_to_mat(s["quat"])
            sc = np.asarray(s["scale"], np.float64)
            o = ((origin - np.asarray(s["pos"], np.float64)) @ Rs) / sc                    # local frame: the unit shape
            d = (dw @ Rs) / sc
            if s["kind"] == "ellipsoid":
                a, b, c = (d * d).sum(-1), 2.0 * (d @ o), o @ o - 1.0
                disc = b * b - 4 * a * c
                with np.errstate(invalid="ignore"):
                    tt = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    t1, t2 = (-1.0 - o) / d, (1.0 - o) / d
                tn, tf = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
                tt = np.where(tn <= tf, tn, np.inf)
        tt = np.where(tt > 0, tt, np.inf)
        best = np.minimum(best, tt)
    with np.errstate(invalid="ignore"):
        pv = dv * best[..., None]                                            # the hit in view space
        pc = np.concatenate([pv, np.ones((h, w, 1))], -1) @ P.T
        z = pc[..., 2] / pc[..., 3]
    return np.where(np.isfinite(best) & (z < 1.0), z, 1.0).astype(np.float32)


def oracle_frame(cam, w, h, mt=None, size=1.0, display_mode=0, sh_deg=3, no_sh0=0, params=None):
    mt = mt or camera.ModelTransform()
    return oracle.frame_setup(cam.view(), cam.projection(w / h), w, h, mt.pos, mt.quat(), mt.scale, size, display_mode,
                              sh_deg, no_sh0, params)


def oracle_model_frame(g, cam, w, h, mt=None, fb=None, mask=None, **kw):
    """Oracle pipeline for one model; returns (frame, projection dict, sorted idx, n_vis, fb)."""
    f = oracle_frame(cam, w, h, mt, **kw)
    pos, color, sh, cov = oracle.convert(g)
    pr = oracle.project(f, pos, color, sh, cov, mask)
    idx, nvis = oracle.depth_sort(pr["key"])
    if fb is None:
        fb = oracle.new_framebuffer(f)
    oracle.rasterize(f, pr, idx, nvis, fb)
    return f, pr, idx, nvis, fb


class ThreadHub:
    """Shared state of ``ThreadComm``: `world` ranks of ONE process (threads), each with its own viewer + stream."""

    def __init__(self, world, timeout=120.0):
        import threading

        self.world = world
        self.barrier = threading.Barrier(world, timeout=timeout)
        self.slots = [None] * world


class ThreadComm:
    """Stand-in for ``parallel.TorchComm`` that lets `world` ranks run the real exchange protocol on one device:
    the collectives are device-to-device copies between the ranks' buffers, delivered exactly in the order
    ``all_to_all_single`` / ``all_gather_into_tensor`` deliver them (by source rank).  TEST ONLY."""

    def __init__(self, hub, rank):
        self.hub, self.rank = hub, rank
        self.bytes_sent = 0

    @staticmethod
    def _sync(t):
        import torch

        if t.is_cuda:
            torch.cuda.current_stream().synchronize()

    def all_to_all_slots(self, recv, send):
        """Fixed-size slots [world, 1 + T, 12]: slot p of `send` goes to rank p.  ``bytes_sent`` counts the PAYLOAD the
        headers announce (word 1 of a slot's first record = records sent), not the slot size."""
        import numpy as np

        h = self.hub
        self._sync(send)
        h.slots[self.rank] = send
        sent = send[:, 0, 1].cpu().numpy().view(np.uint32)
        self.bytes_sent += int(sum(int(c) for g, c in enumerate(sent) if g != self.rank)) * send.shape[2] * 4
        h.barrier.wait()
        for src in range(h.world):
            s = h.slots[src]
            assert s.shape == send.shape, f"rank {src} sized its slots {tuple(s.shape)}, rank {self.rank} {tuple(send.shape)}"
            recv[src].copy_(s[self.rank])
        self._sync(recv)
        h.barrier.wait()

    def all_gather(self, out, inp):
        h = self.hub
        self._sync(inp)
        h.slots[self.rank] = inp
        h.barrier.wait()
        n = inp.numel()
        for src in range(h.world):
            out[src * n:(src + 1) * n].copy_(h.slots[src])
        self._sync(out)
        h.barrier.wait()


def run_ranks(world, fn):
    """Run fn(rank, comm) on `world` threads; re-raises the first failure (and releases the others)."""
    import threading

    hub = ThreadHub(world)
    errors, results = [], [None] * world

    def body(r):
        try:
            results[r] = fn(r, ThreadComm(hub, r))
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            hub.barrier.abort()

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    real = [e for e in errors if not isinstance(e, threading.BrokenBarrierError)]
    if real or errors:
        raise (real or errors)[0]
    return results
