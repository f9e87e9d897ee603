"""gsx_model_neighbors (spec/RENDER_SPEC.md §18) restated in numpy float32, for tests/test_neighbors_cpu.py and
tests/test_gpu_neighbors.py.  `brute` is the definition: every pair, d2 = (dx*dx + dy*dy) + dz*dz with every operation rounded to
float32, neighbours where d2 <= r2.  `grid` is a sorted-cell version for larger n whose cells are its own (floor of x / (2 r) in
float64: wider than any rounding of the distance could reach); it is checked against `brute`.  `cells` / `buckets` restate
csrc/neighbors_math.h's nb_grid, nb_cell and nb_bucket for the comparison with tests/neighbors_driver.cpp.  Nothing here includes
the header: the two are compared, not derived from one another."""
from __future__ import annotations

import numpy as np

F = np.float32
MAX_COUNT = 4095   # GSX_NEIGHBOR_MAX_COUNT
MAX_CELL = 32767   # kNbMaxCell
MAX_BITS = 24
SET, ADD, REMOVE = 0, 1, 2  # gsx_selection_op


def participates(pos, passes=None) -> np.ndarray:
    """bool[n]: passes the filter and has three finite coordinates"""
    pos = np.asarray(pos, F)
    ok = np.isfinite(pos).all(axis=1)
    return ok if passes is None else ok & np.asarray(passes, bool)


def _d2(a, b):
    """float32 d2 of every pair (a: (m, 3), b: (k, 3)) -> (m, k)"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (a[:, None, :] - b[None, :, :]).astype(F)
        sq = (d * d).astype(F)
        return ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)


def brute(pos, part, r, cap=MAX_COUNT, chunk=512) -> np.ndarray:
    """uint32[n]: min(neighbours, cap) for participants, 0 otherwise; n^2 in chunks"""
    pos = np.ascontiguousarray(pos, F)
    part = np.asarray(part, bool)
    n = pos.shape[0]
    r2 = F(r) * F(r)
    idx = np.nonzero(part)[0]
    p = pos[idx]
    out = np.zeros(n, np.uint32)
    for a in range(0, idx.size, chunk):
        near = _d2(p[a:a + chunk], p) <= r2
        out[idx[a:a + chunk]] = near.sum(axis=1) - 1  # (a participant is at d2 = 0 <= r2 of itself)
    return np.minimum(out, np.uint32(cap))


def grid(pos, part, r, cap=MAX_COUNT) -> np.ndarray:
    """the same counts from sorted cells of edge 2 r (float64 floor; far coordinates are clamped into +-2^20 cells, which only joins
    cells): every pair with d2 <= r2 has |dx| <= r (1 + 2^-20) in each axis, so its cells differ by at most 1"""
    pos = np.ascontiguousarray(pos, F)
    part = np.asarray(part, bool)
    n = pos.shape[0]
    r2 = F(r) * F(r)
    out = np.zeros(n, np.uint32)
    idx = np.nonzero(part)[0]
    if idx.size == 0:
        return out
    p = pos[idx]
    c = np.clip(np.floor(p.astype(np.float64) / (2.0 * float(r))), -(2 ** 20), 2 ** 20).astype(np.int64) + 2 ** 20
    key = (c[:, 0] << 44) | (c[:, 1] << 22) | c[:, 2]
    order = np.argsort(key, kind="stable")
    skey, sp = key[order], p[order]
    ukey, start = np.unique(skey, return_index=True)
    end = np.append(start[1:], skey.size)
    counts = np.zeros(idx.size, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                other = ukey + ((dx << 44) + (dy << 22) + dz)
                at = np.searchsorted(ukey, other)
                ok = (at < ukey.size) & (ukey[np.minimum(at, ukey.size - 1)] == other)
                for a, b in zip(np.nonzero(ok)[0], at[ok]):
                    near = _d2(sp[start[a]:end[a]], sp[start[b]:end[b]]) <= r2
                    counts[start[a]:end[a]] += near.sum(axis=1)
    out[idx[order]] = counts - 1
    return np.minimum(out, np.uint32(cap))


def hist(counts, part, cap=MAX_COUNT) -> np.ndarray:
    """uint64[cap + 1]: participants per saturated count"""
    return np.bincount(np.asarray(counts)[np.asarray(part, bool)], minlength=cap + 1).astype(np.uint64)


def hits(counts, part, lo, hi) -> np.ndarray:
    c = np.asarray(counts)
    return np.asarray(part, bool) & (c >= lo) & (c <= hi)


# ---- the engineered sets of the tests -------------------------------------------------------------------------------------------------
def lattice(r=0.25, side=9):
    """side^3 points at spacing exactly r, centred: coordinates are multiples of r on both sides of zero"""
    k = np.arange(side) - side // 2
    return (np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3).astype(F) * F(r)).astype(F)


def special_scene(n=5000, seed=3):
    """a random scene with far, huge, coincident and non-finite positions planted in it; returns (pos, radius)"""
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((n, 3)).astype(F)
    pos[10], pos[11] = [1e6, 0, 0], [1e6, 0, 0]                 # two coincident far points: neighbours of each other
    pos[12], pos[13] = [-1e6, 2, 3], [0, -1e6, 0]
    pos[14], pos[15], pos[16] = [3e38, 0, 0], [-3e38, -3e38, 3e38], [3e38, 3e38, 3e38]
    pos[17], pos[18], pos[19] = [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]
    pos[20:30] = pos[30]                                        # eleven coincident points
    return pos, F(0.12)


# ---- csrc/neighbors_math.h restated -------------------------------------------------------------------------------------------------
def radius_ok(r) -> bool:
    r = F(r)
    with np.errstate(over="ignore", under="ignore"):
        r2 = F(r * r)
    return bool(np.isfinite(r) and r > 0 and r2 > 0 and np.isfinite(r2))


def grid_of(r):
    """(r2, h, inv_h) as nb_grid: h = sqrt(the float32 above r2) * (1 + 2^-5) in float64, rounded to float32"""
    r2 = F(r) * F(r)
    above = float(np.nextafter(r2, F(np.inf))) if r2 < np.finfo(F).max else float(r2) * (1.0 + 2.0 ** -24)
    h = F(np.sqrt(above) * (1.0 + 1.0 / 32.0))
    return r2, h, F(1.0) / h


def cells(x, origin, inv_h) -> np.ndarray:
    """nb_cell of every coordinate (x >= origin, both finite)"""
    with np.errstate(over="ignore"):
        u = ((np.asarray(x, F) - F(origin)).astype(F) * F(inv_h)).astype(F)
    return np.where(u >= F(MAX_CELL), MAX_CELL, np.minimum(u, F(MAX_CELL)).astype(np.int64)).astype(np.uint32)


def buckets(cx, cy, cz, bits) -> np.ndarray:
    m = np.uint64(0xFFFFFFFF)
    k = (np.asarray(cx, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(cy, np.uint64) * np.uint64(0x85EBCA77)
         + np.asarray(cz, np.uint64) * np.uint64(0xC2B2AE3D)) & m
    k ^= k >> np.uint64(15)
    k = (k * np.uint64(0x2C1B3C6D)) & m
    k ^= k >> np.uint64(12)
    k = (k * np.uint64(0x297A2D39)) & m
    k ^= k >> np.uint64(15)
    return (k & np.uint64((1 << bits) - 1)).astype(np.uint32)


def auto_bits(n: int) -> int:
    bits = 8
    while bits < MAX_BITS and (1 << bits) < n:
        bits += 1
    return bits
