"""The numpy restatement of spec §28's model plane (gsx_model_fit_plane, gsx_model_select_plane, gsx_plane_level), for
tests/test_plane_cpu.py and tests/test_gpu_plane.py.  The hash and the probe in Python integers; the candidates and the residual in
float32 operation by operation (the triple's cross product in float64: differences of exact products, as the header takes them); the
counts by brute force; the moments in float64 from the same float32 values, every sum math.fsum's, the correctly rounded sum, with
the sum of the terms' magnitudes beside it; the solve numpy's eigh; the refine loop with its stop rule.  The fixtures are
align_plane_ref's: the noisy corner and the lattice."""
from __future__ import annotations

import math

import numpy as np

from tests import align_plane_ref as AP

F = np.float32
M64 = (1 << 64) - 1
TRIPLES, NORMALS, CALLER = 0, 1, 2
PROBES = 64
NONE = 0xFFFFFFFF
MIN_INLIERS = 3


# ---- the sampling ---------------------------------------------------------------------------------------------------------------------
def mix(seed: int, h: int, s: int, t: int) -> int:
    """output (h << 16 | s << 8 | t) of the splitmix64 stream seeded with `seed`"""
    k = (h << 16) | (s << 8) | t
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def probe(seed: int, h: int, s: int, ok: np.ndarray) -> int:
    """the first of mix(seed, h, s, t) mod n, t = 0 .. 63, with ok[index]; NONE if there is none"""
    n = len(ok)
    if n == 0:
        return NONE
    for t in range(PROBES):
        i = mix(seed, h, s, t) % n
        if ok[i]:
            return i
    return NONE


def participants(pos, keep=None) -> np.ndarray:
    """bool[n]: passes the filter (`keep`, default all) and has three finite coordinates"""
    pos = np.asarray(pos, F).reshape(-1, 3)
    fin = np.isfinite(pos).all(axis=1)
    return fin if keep is None else (fin & np.asarray(keep, bool))


# ---- the residual and the inlier rule ---------------------------------------------------------------------------------------------------
def dot32(n, p) -> np.ndarray:
    """(nx px + ny py) + nz pz in float32, every operation rounded; n: [3] or [m, 3], p: [m, 3]"""
    n, p = np.asarray(n, F), np.asarray(p, F)
    with np.errstate(all="ignore"):
        a = (n[..., 0] * p[..., 0]).astype(F)
        b = (n[..., 1] * p[..., 1]).astype(F)
        c = (n[..., 2] * p[..., 2]).astype(F)
        return ((a + b).astype(F) + c).astype(F)


def residual(plane, pos) -> np.ndarray:
    plane = np.asarray(plane, F)
    with np.errstate(all="ignore"):
        return (dot32(plane[:3], np.asarray(pos, F).reshape(-1, 3)) - plane[3]).astype(F)


def facing(plane, normals, variation, min_cos) -> np.ndarray:
    """bool[n]: fitted and |c| >= min_cos, c the float32 cosine of the kept normal against the plane's"""
    c = dot32(np.asarray(plane, F)[:3], np.asarray(normals, F).reshape(-1, 3))
    return np.isfinite(np.asarray(variation, F)) & (np.abs(c) >= F(min_cos))


def inliers(plane, pos, part, tolerance, min_cos=0.0, normals=None, variation=None) -> np.ndarray:
    with np.errstate(all="ignore"):
        ok = part & (np.abs(residual(plane, pos)) <= F(tolerance))
    if F(min_cos) > 0:
        ok &= facing(plane, normals, variation, min_cos)
    return ok


def in_range(plane, pos, part, lo, hi, min_cos=0.0, normals=None, variation=None) -> np.ndarray:
    r = residual(plane, pos)
    with np.errstate(all="ignore"):
        ok = part & (r >= F(lo)) & (r <= F(hi))
    if F(min_cos) > 0:
        ok &= facing(plane, normals, variation, min_cos)
    return ok


# ---- the candidates ---------------------------------------------------------------------------------------------------------------------
def from_normal(a, k) -> np.ndarray:
    k = np.asarray(k, F)
    return np.array([k[0], k[1], k[2], dot32(k, np.asarray(a, F).reshape(1, 3))[0]], F)


def from_triple(a, b, c):
    """the plane through three float32 points, or None where the cross product's length is zero or not finite"""
    a, b, c = (np.asarray(x, F) for x in (a, b, c))
    with np.errstate(all="ignore"):
        u, v = (b - a).astype(F).astype(np.float64), (c - a).astype(F).astype(np.float64)
        x = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        ln = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) if np.isfinite(x).all() else math.inf
    if not (ln > 0.0 and ln < math.inf):
        return None
    n = (x / ln).astype(F)
    return np.array([n[0], n[1], n[2], dot32(n, a.reshape(1, 3))[0]], F)


def caller_ok(plane) -> bool:
    plane = np.asarray(plane, F)
    return bool(np.isfinite(plane).all() and (plane[:3] != 0).any())


def candidates(pos, part, sample, H, seed, normals=None, variation=None, given=None):
    """(planes float32[H, 4] as reported: zeros where invalid, valid bool[H], slots int[H, 3]: the sampled indices, NONE where unused)"""
    pos = np.asarray(pos, F).reshape(-1, 3)
    planes, valid, slots = np.zeros((H, 4), F), np.zeros(H, bool), np.full((H, 3), NONE, np.int64)
    for h in range(H):
        pl = None
        if sample == CALLER:
            pl = np.asarray(given[h], F) if caller_ok(given[h]) else None
        elif sample == NORMALS:
            i = probe(seed, h, 0, part & np.isfinite(np.asarray(variation, F)))
            slots[h, 0] = i
            if i != NONE:
                pl = from_normal(pos[i], normals[i])
        else:
            s = [probe(seed, h, k, part) for k in range(3)]
            slots[h] = s
            if NONE not in s and len(set(s)) == 3:
                pl = from_triple(pos[s[0]], pos[s[1]], pos[s[2]])
        if pl is not None:
            planes[h], valid[h] = pl, True
    return planes, valid, slots


def counts(planes, valid, pos, part, tolerance, min_cos=0.0, normals=None, variation=None) -> np.ndarray:
    """uint32[H]: the brute-force float32 inlier count of every valid candidate, 0 for an invalid one"""
    out = np.zeros(len(planes), np.uint32)
    for h in range(len(planes)):
        if valid[h]:
            out[h] = int(inliers(planes[h], pos, part, tolerance, min_cos, normals, variation).sum())
    return out


def winner(cnt, valid) -> int:
    """the valid candidate with the largest count, ties to the smaller index; NONE without a valid one"""
    best = NONE
    for h in range(len(cnt)):
        if valid[h] and (best == NONE or cnt[h] > cnt[best]):
            best = h
    return best


# ---- the moments and the solve ------------------------------------------------------------------------------------------------------------
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def moments(plane, pos, inl) -> dict:
    """over the inliers: count, sum_p, sum_r2 (r the float32 residual, squared in float64), centre (float32), scatter (xx xy xz yy yz zz
    of d = p - centre in float32, products in float64); every sum exactly rounded; `mag`: the sums of the terms' magnitudes"""
    p = np.asarray(pos, F).reshape(-1, 3)[inl]
    m = len(p)
    fs = lambda cols: np.array([math.fsum(c) for c in cols])  # noqa: E731
    p64 = p.astype(np.float64)
    r = residual(plane, p).astype(np.float64)
    sum_p = fs(p64.T) if m else np.zeros(3)
    c = (sum_p / m).astype(F) if m else np.zeros(3, F)
    d = (p - c).astype(F).astype(np.float64)
    terms = np.stack([d[:, a] * d[:, b] for a, b in TRI], axis=0) if m else np.zeros((6, 0))
    return dict(count=m, sum_p=sum_p, sum_r2=math.fsum(r * r), centre=c, scatter=fs(terms) if m else np.zeros(6),
                mag=dict(sum_p=np.abs(p64).sum(axis=0) if m else np.zeros(3), sum_r2=float((r * r).sum()), scatter=np.abs(terms).sum(axis=1)))


def bound(m, mag):
    """align_plane_ref.bound: |got - fsum| <= (m + 4) 2^-53 sum|term| for m terms added in any order"""
    return AP.bound(m, mag)


def flip(n, c, toward=None) -> bool:
    """section 26's sign rule at the point c: TOWARD by the float64 dot product of the float32 normal with toward - c, a zero falling
    back to CANONICAL: the first non-zero component positive"""
    n = np.asarray(n, F)
    if toward is not None:
        dot = 0.0
        for a in range(3):
            dot = dot + float(n[a]) * (float(F(toward[a])) - float(F(c[a])))
        if dot != 0.0:
            return dot < 0.0
    for a in range(3):
        if n[a] != 0:
            return bool(n[a] < 0)
    return False


def solve(mom, toward=None):
    """numpy's answer to the moments: dict(plane float32[4], centre, eigenvalues descending) or None (fewer than 3 points, no spread)"""
    if mom["count"] < MIN_INLIERS:
        return None
    s = mom["scatter"]
    A = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    w, V = np.linalg.eigh(A)
    w = np.maximum(w[::-1], 0.0)
    if not (w.sum() > 0 and np.isfinite(w.sum())):
        return None
    v = V[:, 0]
    n = (v / np.linalg.norm(v)).astype(F)
    if flip(n, mom["centre"], toward):
        n = -n
    n = (n + F(0)).astype(F)
    c = mom["centre"].astype(np.float64)
    n64 = n.astype(np.float64)
    off = F((n64[0] * c[0] + n64[1] * c[1]) + n64[2] * c[2])
    return dict(plane=np.array([n[0], n[1], n[2], off], F), centre=mom["centre"], eigenvalues=w)


def fit(pos, part, sample, H, seed, tolerance, min_cos=0.0, refine_iters=0, toward=None, normals=None, variation=None, given=None) -> dict:
    """the whole call: candidates, counts, winner, refine with the stop rule"""
    pos = np.asarray(pos, F).reshape(-1, 3)
    planes, valid, slots = candidates(pos, part, sample, H, seed, normals, variation, given)
    cnt = counts(planes, valid, pos, part, tolerance, min_cos, normals, variation)
    w = winner(cnt, valid)
    out = dict(candidates=planes, valid=valid, slots=slots, counts=cnt, winner=w, n_valid=int(valid.sum()), count=int(part.sum()), degenerate=True,
               plane=np.zeros(4, F), candidate=np.zeros(4, F), candidate_inliers=0 if w == NONE else int(cnt[w]), n_inliers=0, refine_done=0,
               centroid=np.zeros(3, F), eigenvalues=np.zeros(3), rms=0.0, history=[])
    if w == NONE or cnt[w] < MIN_INLIERS:
        return out
    out.update(degenerate=False, plane=planes[w].copy(), candidate=planes[w].copy(), n_inliers=int(cnt[w]))
    plane = planes[w]
    for it in range(refine_iters):
        inl = inliers(plane, pos, part, tolerance, min_cos, normals, variation)
        mom = moments(plane, pos, inl)
        f = solve(mom, toward)
        if f is None:
            break
        again = inliers(f["plane"], pos, part, tolerance, min_cos, normals, variation)
        out["history"].append(int(again.sum()))
        if int(again.sum()) < out["n_inliers"]:
            break
        nxt = moments(f["plane"], pos, again)
        out.update(plane=f["plane"], n_inliers=int(again.sum()), refine_done=it + 1, centroid=f["centre"], eigenvalues=f["eigenvalues"],
                   rms=math.sqrt(nxt["sum_r2"] / nxt["count"]), moments=mom, sum_r2=nxt["sum_r2"], mag_r2=nxt["mag"]["sum_r2"])
        plane = f["plane"]
    return out


# ---- gsx_plane_level --------------------------------------------------------------------------------------------------------------------------
def quat_rows(q) -> np.ndarray:
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def level(plane, up):
    """(quat float64[4], pos float64[3]) by the header's definition, written independently: Rodrigues' shortest arc"""
    plane, up = np.asarray(plane, F).astype(np.float64), np.asarray(up, F).astype(np.float64)
    a, b = plane[:3] / np.linalg.norm(plane[:3]), up / np.linalg.norm(up)
    w = 1.0 + a @ b
    if w > 2.0 ** -40:
        q = np.concatenate([np.cross(a, b), [w]])
    else:
        e = np.zeros(3)
        e[int(np.argmin(np.abs(a)))] = 1.0
        q = np.concatenate([np.cross(e, a), [0.0]])
    return q / np.linalg.norm(q), -(plane[3] / np.linalg.norm(plane[:3])) * b


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
def corner(seed):
    """(pos float32[3000, 3], normals, variation): align_plane_ref's noisy corner and its fitted normals"""
    pos = AP.corner_points(3000, seed)
    nrm, var = AP.fitted_normals(pos)
    return pos, nrm, var


def peel(pos, sample, H=256, seed=7, tolerance=0.006, refine_iters=2, normals=None, variation=None):
    """three successive fits, each over the participants no earlier plane took: [(fit, inlier mask)]"""
    part = participants(pos)
    out = []
    for _ in range(3):
        f = fit(pos, part, sample, H, seed, tolerance, refine_iters=refine_iters, normals=normals, variation=variation)
        inl = inliers(f["plane"], pos, part, tolerance)
        out.append((f, inl))
        part = part & ~inl
    return out


def tilted_lattice(deg=20.0, axis=(1.0, 2.0, 0.5), shift=(0.1, -0.2, 0.3)):
    """align_plane_ref.lattice() rotated and shifted: (pos float32[1600, 3], the true unit normal float64[3])"""
    pos, _, _ = AP.lattice()
    T = AP.rigid(deg, axis, shift)
    return (pos.astype(np.float64) @ T[:, :3].T + T[:, 3]).astype(F), T[:, :3] @ np.array([0.0, 0.0, 1.0])
