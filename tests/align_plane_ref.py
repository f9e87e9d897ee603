"""The numpy restatement of spec §27's point-to-plane step (gsx_model_align_plane_step), for tests/test_align_plane_cpu.py and
tests/test_gpu_align_plane.py.  The float32 steps are the kernel's (d = q - c and g = q - t per axis, d2); every term is taken in
float64 exactly as the kernel takes it, so a term has the same bits on both sides; each sum is math.fsum's, the correctly rounded sum
of the terms: only the order of the additions separates the device from this file.  With every sum comes the sum of the terms'
magnitudes, from which the tests derive their bound.  The solve is numpy's eigh and a pseudo-inverse at a given rank.  The fixtures
of the issue: a noisy corner of three planes, a planar lattice, a sphere and a cylinder with analytic float32 normals."""
from __future__ import annotations

import math

import numpy as np

from tests import nearest_ref as R
from tests import normals_ref as NR

F = np.float32
INF = F(np.inf)
TRI = np.triu_indices(6)
RANK = 1e-9  # kAlignPlaneRank
IDENTITY = np.eye(3, 4, dtype=F)


def used_rows(variation, max_variation=0.0) -> np.ndarray:
    """bool[m]: the target has a fitted normal (a finite variation) within the limit"""
    v = np.asarray(variation, F)
    ok = v < INF
    if F(max_variation) > 0:
        ok &= v <= F(max_variation)
    return ok


def sums(q, t, n, variation, max_variation=0.0) -> dict:
    """q, t, n: float32[m, 3] over the FOUND pairs in index order (q mapped), variation float32[m].  Returns n_pairs, n_unfitted,
    sum_q, centre (float64 of the float32 centre), A21, b, sum_e2, sum_d2, rms_before, rms_plane_before, and `mag`: the sums of the
    terms' magnitudes under the same names (A21, b, sum_q, sum_e2, sum_d2)"""
    q, t, n = (np.ascontiguousarray(a, F).reshape(-1, 3) for a in (q, t, n))
    use = used_rows(variation, max_variation)
    n_unfitted = int((~use).sum())
    q, t, n = q[use], t[use], n[use]
    m = q.shape[0]
    fs = lambda terms: np.array([math.fsum(col) for col in np.atleast_2d(terms.T)])  # noqa: E731
    q64 = q.astype(np.float64)
    sum_q = fs(q64) if m else np.zeros(3)
    c = (sum_q / m).astype(F) if m else np.zeros(3, F)
    d = (q - c).astype(F).astype(np.float64)
    g = (q - t).astype(F).astype(np.float64)
    nn = n.astype(np.float64)
    a = np.stack([d[:, 1] * nn[:, 2] - d[:, 2] * nn[:, 1], d[:, 2] * nn[:, 0] - d[:, 0] * nn[:, 2], d[:, 0] * nn[:, 1] - d[:, 1] * nn[:, 0]], axis=1)
    e = (g[:, 0] * nn[:, 0] + g[:, 1] * nn[:, 1]) + g[:, 2] * nn[:, 2]
    J = np.concatenate([a, nn], axis=1)
    tA = J[:, TRI[0]] * J[:, TRI[1]]
    tb = J * e[:, None]
    te2 = e * e
    gf = (q - t).astype(F)
    d2 = ((gf[:, 0] * gf[:, 0] + gf[:, 1] * gf[:, 1]).astype(F) + gf[:, 2] * gf[:, 2]).astype(F).astype(np.float64)
    z = lambda k: np.zeros(k)  # noqa: E731
    out = dict(n_pairs=m, n_unfitted=n_unfitted, sum_q=sum_q, centre=c.astype(np.float64), A21=fs(tA) if m else z(21), b=fs(tb) if m else z(6),
               sum_e2=math.fsum(te2), sum_d2=math.fsum(d2))
    out["rms_before"] = math.sqrt(out["sum_d2"] / m) if m else 0.0
    out["rms_plane_before"] = math.sqrt(out["sum_e2"] / m) if m else 0.0
    out["mag"] = dict(sum_q=np.abs(q64).sum(axis=0) if m else z(3), A21=np.abs(tA).sum(axis=0) if m else z(21), b=np.abs(tb).sum(axis=0) if m else z(6),
                      sum_e2=float(te2.sum()), sum_d2=float(d2.sum()))
    return out


def bound(m, mag):
    """|got - fsum| <= (m + 4) 2^-53 sum|term|: m - 1 additions of a sum in any order, each with a relative error of at most 2^-53
    of a partial sum that no more than sum|term| bounds, to first order (m - 1) 2^-53 sum|term|; the second-order part, fsum's own
    final rounding and the slack of "first order" fit in the 5 extra units for every m below 2^26."""
    return (m + 4) * 2.0 ** -53 * np.asarray(mag, np.float64)


def full(A21) -> np.ndarray:
    A = np.zeros((6, 6))
    A[TRI] = np.asarray(A21, np.float64)
    return A + np.triu(A, 1).T


def solve(A21, b, centre, rank=None) -> dict:
    """numpy's answer: eigh, the rank by the library's rule unless given, x = -pinv_rank(A) b, the delta about the centre"""
    A = full(A21)
    w, V = np.linalg.eigh(A)
    w, V = w[::-1], V[:, ::-1]
    if rank is None:
        rank = int((w > RANK * w[0]).sum()) if w[0] > 0 else 0
    x = np.zeros(6)
    for i in range(rank):
        x -= V[:, i] * (V[:, i] @ np.asarray(b, np.float64)) / w[i]
    om, tau = x[:3], x[3:]
    ang = float(np.linalg.norm(om))
    quat = np.array([0.0, 0.0, 0.0, 1.0]) if ang == 0 else np.concatenate([om / ang * math.sin(ang / 2), [math.cos(ang / 2)]])
    Rm = R.quat_rows(quat)
    c = np.asarray(centre, np.float64)
    return dict(eigenvalues=w, rank=rank, x=x, quat=quat, R=Rm, pos=c + tau - Rm @ c, scale=1.0)


def matrix34(delta) -> np.ndarray:
    return np.concatenate([delta["R"], np.asarray(delta["pos"], np.float64)[:, None]], axis=1)


def compose34(a, b) -> np.ndarray:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]], axis=1)


def nearest(q, targets):
    """(index, float32 d2) of every mapped query's nearest target: nearest_ref's definition"""
    q, targets = np.ascontiguousarray(q, F), np.ascontiguousarray(targets, F)
    return R.brute(q, np.ones(len(q), bool), targets, np.ones(len(targets), bool))


def plane_step_numpy(src, xform, targets, normals, variation):
    """one whole step in numpy: (xform_next float32[3, 4], sums, delta)"""
    q = R.map_points(xform, src)
    index, _ = nearest(q, targets)
    s = sums(q, targets[index], normals[index], variation[index])
    d = solve(s["A21"], s["b"], s["centre"])
    return compose34(matrix34(d), xform).astype(F), s, d


def point_step_numpy(src, xform, targets):
    """one point-to-point step (spec §23) in numpy: xform_next float32[3, 4]"""
    q = R.map_points(xform, src)
    index, _ = nearest(q, targets)
    return R.compose(R.align_solve(R.align_sums(q, targets[index])), xform)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def rigid(deg, axis, shift) -> np.ndarray:
    """float64[3, 4]: the rotation by `deg` degrees about `axis` through the box's centre (0.5, 0.5, 0.5), then `shift`"""
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = math.radians(deg) / 2
    Rm = R.quat_rows(np.concatenate([ax * math.sin(h), [math.cos(h)]]))
    c = np.full(3, 0.5)
    return np.concatenate([Rm, (c - Rm @ c + np.asarray(shift, np.float64))[:, None]], axis=1)


def corner_points(n, seed, noise=0.002) -> np.ndarray:
    """n points on the three faces x = 0, y = 0, z = 0 of the unit box, with noise across the face"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    face = rng.integers(0, 3, n)
    p[np.arange(n), face] = rng.normal(0.0, noise, n)
    return p.astype(F)


def corner(seed, n_dst=3000, n_src=1500):
    """(targets, source, truth): a noisy corner, an independent sample of it moved by 2 degrees and 1 % of the box; `truth` (float64
    3x4) maps the source back onto the targets' surface"""
    targets = corner_points(n_dst, 100 + seed)
    fresh = corner_points(n_src, 200 + seed).astype(np.float64)
    move = rigid(2.0, (1.0, 2.0, 3.0), (0.006, -0.005, 0.006))
    src = (fresh @ move[:, :3].T + move[:, 3]).astype(F)
    Rm = move[:, :3]
    return targets, src, np.concatenate([Rm.T, (-Rm.T @ move[:, 3])[:, None]], axis=1)


def fitted_normals(pos, k=8):
    """(normal float32[n, 3], variation float32[n]) by normals_ref: what gsx_model_normals returns up to its documented tolerance"""
    index, d2 = NR.lists(pos, np.ones(len(pos), bool), k)
    f = NR.fit(pos, index, d2)
    return f["normal"], f["variation"]


def lattice(side=40, spacing=0.025):
    """(targets, normals, variation): side x side points at z = 0, normals (0, 0, 1)"""
    u = np.arange(side, dtype=np.float64) * spacing
    g = np.stack(np.meshgrid(u, u, indexing="ij"), axis=-1).reshape(-1, 2)
    pos = np.concatenate([g, np.zeros((len(g), 1))], axis=1).astype(F)
    return pos, np.tile(F([0, 0, 1]), (len(pos), 1)), np.zeros(len(pos), F)


def sphere(n=2000, seed=5, lift=0.01):
    """(targets, normals, variation, source): n / 2 random directions and their antipodes on a sphere of radius 0.4 about (0.5, 0.5,
    0.5), the analytic normals, and every target lifted along its own normal as the source: each source's nearest target is its own
    (a neighbour is farther by the chord), the sources' mean is the sphere's centre, so d is parallel to n and the pairs determine
    the three translations alone"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n // 2, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v = np.concatenate([v, -v])
    return (0.5 + 0.4 * v).astype(F), v.astype(F), np.zeros(len(v), F), (0.5 + (0.4 + lift) * v).astype(F)


def cylinder(n=2000, seed=6, lift=0.01):
    """(targets, normals, variation, source): n / 2 random (angle, height) and the points opposite them on a cylinder of radius 0.3
    about the axis x = y = 0.5, the analytic normals, every target lifted along its normal as the source: the slide along the axis
    and the turn about it are left undetermined, rank 4"""
    rng = np.random.default_rng(seed)
    a, z = rng.random(n // 2) * 2 * math.pi, rng.random(n // 2)
    a, z = np.concatenate([a, a + math.pi]), np.concatenate([z, z])
    nrm = np.stack([np.cos(a), np.sin(a), np.zeros(len(a))], axis=1)
    base = np.array([0.5, 0.5, 0.0]) + z[:, None] * np.array([0, 0, 1.0])
    return (base + 0.3 * nrm).astype(F), nrm.astype(F), np.zeros(len(a), F), (base + (0.3 + lift) * nrm).astype(F)


def lattice_source(pos, count=800, seed=3, shift=(0.007, 0.004, 0.05)):
    """`count` of the lattice's points (a seeded choice, ascending) shifted by less than half the spacing in the plane and lifted"""
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(len(pos), count, replace=False))
    return (pos[pick] + F(shift)).astype(F)
