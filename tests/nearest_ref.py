"""gsx_model_nearest, gsx_model_select_nearest and gsx_model_align_step (spec/RENDER_SPEC.md §23) restated in numpy, for
tests/test_nearest_cpu.py and tests/test_gpu_nearest.py.  `brute` is the definition: the queries mapped row by row in float32 with
every operation rounded, the float32 d2 of every (query, target) pair (tests/neighbors_ref.py: `_d2`), the smallest d2 within reach
and, among equal d2, the smallest target index.  The statistics and the align sums are float64; the align solve is numpy's SVD
(Kabsch / Umeyama), which shares nothing with csrc/align_math.h's Jacobi iteration.  Nothing here includes a csrc header: the two are
compared, not derived from one another."""
from __future__ import annotations

import numpy as np

from tests.neighbors_ref import _d2

F = np.float32
NONE = 0xFFFFFFFF               # GSX_NEAREST_NONE
MODEL_TRANSFORMS = 1            # GSX_NEAREST_MODEL_TRANSFORMS
SELECT_RANGE, SELECT_TRANSFER = 0, 1
ALIGN_SCALE = 1
INF = F(np.inf)
FLT_MAX = np.finfo(F).max


def map_points(xform, pos) -> np.ndarray:
    """float32[n, 3]: q_r = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3, every operation rounded to float32"""
    m = np.ascontiguousarray(xform, F).reshape(3, 4)
    p = np.ascontiguousarray(pos, F)
    with np.errstate(over="ignore", invalid="ignore"):
        out = [(((m[r, 0] * p[:, 0]).astype(F) + (m[r, 1] * p[:, 1]).astype(F)).astype(F) + (m[r, 2] * p[:, 2]).astype(F)).astype(F) + m[r, 3]
               for r in range(3)]
    return np.stack(out, axis=1).astype(F)


def query_participates(xform, pos, passes=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(q, participates, non-finite): a query participates if it passes, its stored and its mapped position are finite"""
    q = map_points(xform, pos)
    passes = np.ones(q.shape[0], bool) if passes is None else np.asarray(passes, bool)
    finite = np.isfinite(np.asarray(pos, F)).all(axis=1) & np.isfinite(q).all(axis=1)
    return q, passes & finite, passes & ~finite


def cap2(max_distance) -> np.float32:
    """the cap on d2: fl(max * max), or the largest float32 without a max_distance (a d2 that overflowed is out of reach)"""
    m = F(max_distance)
    return F(m * m) if m > 0 else FLT_MAX


def brute(q, q_part, targets, t_part, max_distance=0.0, chunk=512) -> tuple[np.ndarray, np.ndarray]:
    """(uint32 index[n], float32 d2[n]) over the mapped queries q: the definition"""
    q = np.ascontiguousarray(q, F)
    n = q.shape[0]
    index, best = np.full(n, NONE, np.uint32), np.full(n, INF, F)
    tidx = np.nonzero(np.asarray(t_part, bool))[0]
    qidx = np.nonzero(np.asarray(q_part, bool))[0]
    if tidx.size == 0 or qidx.size == 0:
        return index, best
    t = np.ascontiguousarray(targets, F)[tidx]
    cap = cap2(max_distance)
    for a in range(0, qidx.size, chunk):
        rows = qidx[a:a + chunk]
        with np.errstate(over="ignore", invalid="ignore"):
            d = _d2(q[rows], t)
        col = d.argmin(axis=1)  # (the first of equal values: tidx ascends, so the smallest target index)
        dmin = d[np.arange(rows.size), col]
        found = dmin <= cap
        index[rows[found]] = tidx[col[found]].astype(np.uint32)
        best[rows[found]] = dmin[found]
    return index, best


def stats(index, d2) -> dict:
    """over the found queries: n_found, exact d_min and d_max, the float64 mean distance and rms; all 0 without any"""
    found = np.asarray(index) != NONE
    m = int(found.sum())
    if m == 0:
        return dict(n_found=0, d_min=F(0), d_max=F(0), mean=0.0, rms=0.0)
    v = np.asarray(d2, F)[found]
    d = np.sqrt(v).astype(F)
    return dict(n_found=m, d_min=d.min(), d_max=d.max(), mean=float(d.astype(np.float64).sum() / m),
                rms=float(np.sqrt(v.astype(np.float64).sum() / m)))


def hit(index, d2, q_part, mode, lo=0.0, hi=0.0, dst_selected=None) -> np.ndarray:
    """bool[n]: RANGE participates and lo <= sqrtf(d2) <= hi; TRANSFER found and the target is selected (dst_selected: bool per target, or
    None: the target model has no selection)"""
    index = np.asarray(index)
    if mode == SELECT_RANGE:
        d = np.sqrt(np.asarray(d2, F)).astype(F)
        return np.asarray(q_part, bool) & (d >= F(lo)) & (d <= F(hi))
    out = np.zeros(index.shape[0], bool)
    if dst_selected is not None:
        found = index != NONE
        out[found] = np.asarray(dst_selected, bool)[index[found]]
    return out


def model_matrix(src_t, dst_t) -> np.ndarray:
    """float32[3, 4] = inv(M_dst) M_src in float64, rounded once; a transform is (pos[3], quat xyzw[4], scale[3]), M = T R S"""
    def m44(t):
        pos, quat, scale = (np.asarray(np.asarray(a, F), np.float64) for a in t)
        x, y, z, w = quat / np.sqrt((quat * quat).sum())
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        M = np.eye(4)
        M[:3, :3] = R * scale[None, :]
        M[:3, 3] = pos
        return M
    return (np.linalg.inv(m44(dst_t)) @ m44(src_t))[:3].astype(F)


def quat_rows(q) -> np.ndarray:
    x, y, z, w = np.asarray(q, np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rows_quat(R) -> np.ndarray:
    """the unit quaternion (x, y, z, w), w >= 0, of a rotation matrix (float64; Shepperd's branch on the largest of w, x, y, z)"""
    R = np.asarray(R, np.float64)
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], -R[0, 0] + R[1, 1] - R[2, 2], -R[0, 0] - R[1, 1] + R[2, 2]]
    k = int(np.argmax(t))
    if k == 0:
        w = np.sqrt(1 + t[0]) / 2
        q = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    elif k == 1:
        x = np.sqrt(1 + t[1]) / 2
        q = [x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x), (R[2, 1] - R[1, 2]) / (4 * x)]
    elif k == 2:
        y = np.sqrt(1 + t[2]) / 2
        q = [(R[0, 1] + R[1, 0]) / (4 * y), y, (R[1, 2] + R[2, 1]) / (4 * y), (R[0, 2] - R[2, 0]) / (4 * y)]
    else:
        z = np.sqrt(1 + t[3]) / 2
        q = [(R[0, 2] + R[2, 0]) / (4 * z), (R[1, 2] + R[2, 1]) / (4 * z), z, (R[1, 0] - R[0, 1]) / (4 * z)]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def align_sums(q, t) -> dict:
    """the sums of spec §23 over the pairs (q[i], t[i]), float32 arrays: n, the float64 sums, and about the means rounded to float32
    the products of the float32 differences, taken and summed in float64"""
    q, t = np.ascontiguousarray(q, F), np.ascontiguousarray(t, F)
    n = q.shape[0]
    sq, st = q.astype(np.float64).sum(axis=0), t.astype(np.float64).sum(axis=0)
    if n == 0:
        return dict(n=0, sum_q=sq, sum_t=st, H=np.zeros((3, 3)), spread_q=0.0, spread_t=0.0)
    qm, tm = (sq / n).astype(F), (st / n).astype(F)
    dq, dt = (q - qm).astype(F).astype(np.float64), (t - tm).astype(F).astype(np.float64)
    return dict(n=n, sum_q=sq, sum_t=st, H=dq.T @ dt, spread_q=float((dq * dq).sum()), spread_t=float((dt * dt).sum()))


def horn_matrix(H) -> np.ndarray:
    """Horn's symmetric 4x4 N(H) over (w, x, y, z): the test derives its tolerance from this matrix's norm and eigenvalue gap"""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = np.asarray(H, np.float64)
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])


def align_solve(sums, with_scale=False) -> dict:
    """Kabsch / Umeyama by numpy's float64 SVD: t ~ s R q + p.  R = V diag(1, 1, det) U^T of H = U S V^T (H's rows: q's axes)"""
    n, H = sums["n"], np.asarray(sums["H"], np.float64)
    U, S, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    s = float((S * np.diag(D)).sum() / sums["spread_q"]) if with_scale else 1.0
    qm, tm = sums["sum_q"] / n, sums["sum_t"] / n
    return dict(quat=rows_quat(R), R=R, scale=s, pos=tm - s * (R @ qm))


def compose(delta, xform) -> np.ndarray:
    """float32[3, 4] of delta o xform, composed in float64 and rounded once"""
    A = np.asarray(xform, F).reshape(3, 4).astype(np.float64)
    sR = delta["scale"] * quat_rows(delta["quat"])
    return np.concatenate([sR @ A[:, :3], (sR @ A[:, 3] + np.asarray(delta["pos"], np.float64))[:, None]], axis=1).astype(F)

