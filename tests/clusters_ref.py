"""gsx_model_clusters and gsx_model_select_clusters (spec/RENDER_SPEC.md §19) restated in numpy, for tests/test_clusters_cpu.py and
tests/test_gpu_clusters.py.  The edges are the definition's: every pair of participants, d2 = (dx*dx + dy*dy) + dz*dz with every
operation rounded to float32 (tests/neighbors_ref.py: _d2), an edge where d2 <= r2.  A sequential union-find joins them; the label of
a cluster is computed afterwards as the minimum index over its members, not taken from the order of the unions.  Nothing here
includes csrc/clusters_math.h: the two are compared, not derived from one another."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import neighbors_ref as N

F = np.float32
NONE = 0xFFFFFFFF                     # GSX_CLUSTER_NONE
BY_SIZE, LARGEST, SEEDED = 0, 1, 2    # gsx_cluster_select_desc.mode
SET, ADD, REMOVE = N.SET, N.ADD, N.REMOVE


def edges(pos, part, r, chunk=512):
    """(i, j) index arrays, i < j: the pairs of participants with d2 <= r2; n^2 in chunks"""
    pos = np.ascontiguousarray(pos, F)
    idx = np.nonzero(np.asarray(part, bool))[0]
    p = pos[idx]
    r2 = F(r) * F(r)
    out_i, out_j = [], []
    for a in range(0, idx.size, chunk):
        ii, jj = np.nonzero(N._d2(p[a:a + chunk], p) <= r2)
        ii = ii + a
        keep = ii < jj
        out_i.append(idx[ii[keep]])
        out_j.append(idx[jj[keep]])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_i), np.concatenate(out_j)


def grid_edges(pos, part, r):
    """the same pairs from sorted cells of edge 2 r, for larger n (tests/neighbors_ref.py: grid has the argument: a pair with d2 <= r2
    lies in cells that differ by at most 1 per axis); checked against `edges`"""
    pos = np.ascontiguousarray(pos, F)
    idx = np.nonzero(np.asarray(part, bool))[0]
    empty = np.zeros(0, np.int64)
    if idx.size == 0:
        return empty, empty
    r2 = F(r) * F(r)
    p = pos[idx]
    c = np.clip(np.floor(p.astype(np.float64) / (2.0 * float(r))), -(2 ** 20), 2 ** 20).astype(np.int64) + 2 ** 20
    key = (c[:, 0] << 44) | (c[:, 1] << 22) | c[:, 2]
    order = np.argsort(key, kind="stable")
    skey, sp, sidx = key[order], p[order], idx[order]
    ukey, start = np.unique(skey, return_index=True)
    end = np.append(start[1:], skey.size)
    out_i, out_j = [empty], [empty]
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                other = ukey + ((dx << 44) + (dy << 22) + dz)
                at = np.searchsorted(ukey, other)
                ok = (at < ukey.size) & (ukey[np.minimum(at, ukey.size - 1)] == other)
                for a, b in zip(np.nonzero(ok)[0], at[ok]):
                    ii, jj = np.nonzero(N._d2(sp[start[a]:end[a]], sp[start[b]:end[b]]) <= r2)
                    gi, gj = sidx[start[a] + ii], sidx[start[b] + jj]
                    keep = gi < gj
                    out_i.append(gi[keep])
                    out_j.append(gj[keep])
    return np.concatenate(out_i), np.concatenate(out_j)


def components(n, part, ei, ej):
    """(labels uint32[n], sizes uint32[n]) of the graph: the label is the smallest index of the component, NONE / 0 outside `part`"""
    part = np.asarray(part, bool)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(ei).tolist(), np.asarray(ej).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[rb] = ra  # (whichever: the label does not come from here)
    root = np.array([find(i) for i in range(n)], np.int64)
    smallest = np.full(n, n, np.int64)
    members = np.nonzero(part)[0]
    np.minimum.at(smallest, root[members], members)
    count = np.bincount(root[members], minlength=n)
    labels = np.full(n, NONE, np.uint32)
    sizes = np.zeros(n, np.uint32)
    labels[members] = smallest[root[members]]
    sizes[members] = count[root[members]]
    return labels, sizes


@dataclasses.dataclass
class Clusters:
    labels: np.ndarray
    sizes: np.ndarray
    count: int
    n_clusters: int
    largest_size: int
    largest_label: int


def of_labels(labels, sizes) -> Clusters:
    """the stats of a labelling: the largest cluster's label is the smallest on a tie, NONE without participants"""
    part = labels != NONE
    roots = np.nonzero(part & (labels == np.arange(labels.size)))[0]
    if roots.size == 0:
        return Clusters(labels, sizes, 0, 0, 0, NONE)
    largest = int(sizes[roots].max())
    return Clusters(labels, sizes, int(part.sum()), int(roots.size), largest, int(roots[sizes[roots] == largest].min()))


def clusters(pos, part, r) -> Clusters:
    part = np.asarray(part, bool)
    return of_labels(*components(np.asarray(pos).shape[0], part, *edges(pos, part, r)))


def hits(c: Clusters, mode, size_lo=0, size_hi=0, seeds=None) -> np.ndarray:
    """bool[n]: the hit set of gsx_model_select_clusters; seeds: the selection before the call (None: the model has none)"""
    part = c.labels != NONE
    if mode == BY_SIZE:
        return part & (c.sizes >= size_lo) & (c.sizes <= size_hi)
    if mode == LARGEST:
        return part & (c.labels == c.largest_label)
    if seeds is None:
        return np.zeros(part.size, bool)
    seeded = np.unique(c.labels[part & np.asarray(seeds, bool)])
    return part & np.isin(c.labels, seeded)


def apply_op(old, hit, op):
    return hit if op == SET else (old | hit if op == ADD else old & ~hit)


# ---- the engineered sets of the tests -------------------------------------------------------------------------------------------------
def chain(n=4096, seed=11, split=False):
    """n points at x = 0.5 k in shuffled index order (returns pos and k of every index): at r = 0.5 consecutive points are at
    d2 == r2 exactly, so one cluster; `split` moves every point past the middle by +0.25, so the gap there is 0.75: two clusters"""
    k = np.random.default_rng(seed).permutation(n)
    x = k.astype(F) * F(0.5)
    if split:
        x = np.where(k >= n // 2, x + F(0.25), x).astype(F)
    pos = np.zeros((n, 3), F)
    pos[:, 0] = x
    return pos, k


def bridge(seed=5):
    """two 27-point blobs at spacing 0.25 whose nearest points are 0.5 apart, and one point half way between them (index returned):
    at r = 0.25 one cluster of 55 with it, two of 27 without; index order shuffled"""
    a = N.lattice(0.25, 3)
    b = (a + F([1.0, 0.0, 0.0])).astype(F)
    pos = np.concatenate([a, b, F([[0.5, 0.0, 0.0]])])
    order = np.random.default_rng(seed).permutation(pos.shape[0])
    return np.ascontiguousarray(pos[order]), int(np.nonzero(order == 54)[0][0])
