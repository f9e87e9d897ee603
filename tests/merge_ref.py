"""gsx_model_merge (spec/RENDER_SPEC.md §13) restated in numpy float64, for tests/test_merge_cpu.py and tests/test_gpu_merge.py: the
kept set and the order (tests/extract_ref.py per source), the bake of a model transform into positions, covariances and SH
coefficients, and the requantisation into the pod kind through oracle.spec_f64.quantise_pod.  The SH matrices are fitted by least
squares to oracle.spec_f64.sh_color at random directions; nothing here looks at csrc/merge_math.h: the two are compared."""
from __future__ import annotations

import numpy as np

from oracle import spec_f64
from tests import extract_ref as X

MAX_SOURCES = 64  # GSX_MERGE_MAX_SOURCES
BANDS = ((0, 3), (3, 5), (8, 7))  # (first SH coefficient, size) of degrees 1, 2, 3
U = 2.0 ** -24  # float32 unit roundoff


def is_identity(pos, quat, scale) -> bool:
    """pos 0, scale 1, quat (0, 0, 0, +-1), as float32 values"""
    p, q, s = (np.asarray(a, np.float32) for a in (pos, quat, scale))
    return bool(np.all(p == 0) and np.all(s == 1) and np.all(q[:3] == 0) and abs(float(q[3])) == 1.0)


def quat_rows_f32(quat) -> np.ndarray:
    """R_m as the library's host code makes it (spec §3): from the quaternion as given, in float32 — returned as float64"""
    f = np.float32
    x, y, z, w = (f(v) for v in quat)
    x2, y2, z2 = f(x + x), f(y + y), f(z + z)
    xx, xy, xz, yy, yz, zz = f(x * x2), f(x * y2), f(x * z2), f(y * y2), f(y * z2), f(z * z2)
    wx, wy, wz = f(w * x2), f(w * y2), f(w * z2)
    one = f(1)
    r = [[f(one - f(yy + zz)), f(xy - wz), f(xz + wy)], [f(xy + wz), f(one - f(xx + zz)), f(yz - wx)], [f(xz - wy), f(yz + wx), f(one - f(xx + yy))]]
    return np.array(r, np.float32).astype(np.float64)


def sh_basis(dirs) -> np.ndarray:
    """Y[k, i]: the k-th basis function of degrees 1..3 at direction i, read off spec_f64.sh_color with one-hot coefficients"""
    dirs = np.asarray(dirs, np.float64)
    out = np.empty((15, dirs.shape[0]))
    for k in range(15):
        sh = np.zeros((dirs.shape[0], 15, 3))
        sh[:, k, 0] = 1.0
        out[k] = spec_f64.sh_color(dirs, sh, 3)[:, 0]
    return out


def sh_matrices(quat, n_dirs: int = 400, seed: int = 1):
    """[M_1 (3x3), M_2 (5x5), M_3 (7x7)] in float64 with  sum_k (M c)_k Y_k(R d) = sum_k c_k Y_k(d)  for all unit d, R the rotation of
    the NORMALISED quaternion: the least-squares solution of  Z^T M = Y^T  over random directions (Z = Y at the rotated ones)."""
    q = np.asarray(quat, np.float64)
    R = spec_f64.quat_to_mat(q / np.linalg.norm(q))
    d = np.random.default_rng(seed).normal(size=(n_dirs, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y, Z = sh_basis(d), sh_basis(d @ R.T)
    return [np.linalg.lstsq(Z[c0:c0 + m].T, Y[c0:c0 + m].T, rcond=None)[0] for c0, m in BANDS]


def flat_matrices(mats) -> np.ndarray:
    """the 83 numbers in the library's order: the three matrices row-major, one behind the other"""
    return np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in mats])


def _sym(cov):
    c = np.asarray(cov, np.float64)
    S = np.empty((c.shape[0], 3, 3))
    S[:, 0, 0], S[:, 0, 1], S[:, 0, 2] = c[:, 0], c[:, 1], c[:, 2]
    S[:, 1, 0], S[:, 1, 1], S[:, 1, 2] = c[:, 1], c[:, 3], c[:, 4]
    S[:, 2, 0], S[:, 2, 1], S[:, 2, 2] = c[:, 2], c[:, 4], c[:, 5]
    return S


def _six(S):
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def bake(pos, sh, cov, m_pos, m_quat, m_scale):
    """One source's planes (the exact dequantisation of what it stores) under its model transform, in float64:
    p' = R (s * p) + t, S' = M S M^T with M = R diag(s) — R the float32 R_m (quat_rows_f32) — and per band c' = M_l c.
    Returns (pos, sh [n, 45], cov [n, 6]) and, as a second tuple, the sums of |a_i b_i| over each result's own products (the
    magnitudes the forward-error bounds of a float32 evaluation are stated in)."""
    R, s, t = quat_rows_f32(m_quat), np.asarray(m_scale, np.float32).astype(np.float64), np.asarray(m_pos, np.float32).astype(np.float64)
    p = np.asarray(pos, np.float64)
    sp = p * s
    out_p = sp @ R.T + t
    mag_p = np.abs(sp) @ np.abs(R).T + np.abs(t)
    M = R * s[None, :]
    S = _sym(cov)
    out_c = _six(M @ S @ M.T)
    mag_c = _six(np.abs(M) @ np.abs(S) @ np.abs(M).T)
    c = np.asarray(sh, np.float64).reshape(p.shape[0], -1, 3)
    out_s, mag_s = np.zeros_like(c), np.zeros_like(c)
    if c.shape[1]:
        for (c0, m), Ml in zip(BANDS, sh_matrices(m_quat)):
            out_s[:, c0:c0 + m] = np.einsum("jk,nkc->njc", Ml, c[:, c0:c0 + m])
            mag_s[:, c0:c0 + m] = np.einsum("jk,nkc->njc", np.abs(Ml), np.abs(c[:, c0:c0 + m]))
    return (out_p, out_s.reshape(p.shape[0], -1), out_c), (mag_p, mag_s.reshape(p.shape[0], -1), mag_c)


def merge(sources, filter_bits: int = 0, flags: int = 0, sh_kind: int = 0, cov_kind: int = 0):
    """sources: dicts with pos [n, 3], color [n], sh [n, 45] (or [n, 0]), cov [n, 6] — float32, as gsx_model_download_pod returns them —
    and optionally mt = (pos, quat, scale), mask, selection (bool[n]), edit_flags (uint32[n]).
    Returns a dict: counts; kept (per source, ascending indices); pos, color, sh, cov — float32, what the merged model of kinds
    (sh_kind, cov_kind) holds, dequantised (identity sources as they are, baked ones rounded to float32 / requantised by
    spec_f64.quantise_pod); exact = (pos, sh, cov) float64 before any rounding; mag = the matching |a_i b_i| sums (zero rows for
    identity sources); baked = bool per merged Gaussian."""
    parts = {k: [] for k in ("pos", "color", "sh", "cov", "xp", "xs", "xc", "mp", "ms", "mc", "baked")}
    counts, kept_all = [], []
    for src in sources:
        n = src["pos"].shape[0]
        kept = X.kept(n, filter_bits, flags, src.get("mask"), src.get("selection"), src.get("edit_flags"))
        counts.append(kept.size)
        kept_all.append(kept)
        pos, color, sh, cov = (np.asarray(src[k])[kept] for k in ("pos", "color", "sh", "cov"))
        mt = src.get("mt")
        if mt is None or is_identity(*mt):
            exact, mag = (pos.astype(np.float64), sh.astype(np.float64), cov.astype(np.float64)), (np.zeros(pos.shape), np.zeros(sh.shape), np.zeros(cov.shape))
            out = (pos, sh, cov)
        else:
            exact, mag = bake(pos, sh, cov, *mt)
            with np.errstate(over="ignore"):
                q_sh, q_cov = spec_f64.quantise_pod(exact[1].astype(np.float32), exact[2].astype(np.float32), sh_kind if sh.shape[1] else 0, cov_kind)
            out = (exact[0].astype(np.float32), q_sh, q_cov)
        for k, a in zip(("pos", "sh", "cov", "xp", "xs", "xc", "mp", "ms", "mc"), out + exact + mag):
            parts[k].append(a)
        parts["color"].append(color)
        parts["baked"].append(np.full(kept.size, not (mt is None or is_identity(*mt))))
    cat = {k: np.concatenate(v) for k, v in parts.items()}
    return dict(counts=counts, kept=kept_all, pos=cat["pos"], color=cat["color"], sh=cat["sh"], cov=cat["cov"], exact=(cat["xp"], cat["xs"], cat["xc"]),
                mag=(cat["mp"], cat["ms"], cat["mc"]), baked=cat["baked"])


def half_ulp(x) -> np.ndarray:
    """one binary16 unit in the last place at |x| (subnormals: 2^-24)"""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)
