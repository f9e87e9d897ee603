"""gsx_model_knn and gsx_model_select_knn (spec/RENDER_SPEC.md §20) restated in numpy, for tests/test_knn_cpu.py and
tests/test_gpu_knn.py.  `brute` is the definition: the float32 d2 of every pair of participants (tests/neighbors_ref.py: `_d2`, every
operation rounded), the diagonal set to +inf (self is excluded by index), each row sorted, its first k values, padded with +inf.
The scores are float32 in the stated order (numpy's float32 sqrt, add and divide are correctly rounded), the statistics float64.
Nothing here includes csrc/knn_math.h: the two are compared, not derived from one another."""
from __future__ import annotations

import numpy as np

from tests.neighbors_ref import _d2

F = np.float32
MAX_K = 16                      # GSX_KNN_MAX_K
SCORE_KTH, SCORE_MEAN = 0, 1    # GSX_KNN_SCORE_*
SELECT_RANGE, SELECT_OUTLIERS = 0, 1
INF = F(np.inf)


def brute(pos, part, k, chunk=512) -> np.ndarray:
    """float32[n, k]: row i = the k smallest d2(i, j) over the participants j != i, ascending, +inf where there are fewer; a row of
    +inf for a Gaussian that does not participate"""
    pos = np.ascontiguousarray(pos, F)
    part = np.asarray(part, bool)
    n = pos.shape[0]
    idx = np.nonzero(part)[0]
    p = pos[idx]
    out = np.full((n, k), INF, F)
    for a in range(0, idx.size, chunk):
        d = _d2(p[a:a + chunk], p)
        rows = np.arange(d.shape[0])
        d[rows, a + rows] = INF  # self, by index
        d.sort(axis=1)
        have = min(k, d.shape[1])
        out[idx[a:a + chunk], :have] = d[:, :have]
    return out


def score(rows, kind) -> np.ndarray:
    """float32[n]: sqrt of the k-th value, or ((sqrt r0 + sqrt r1) + ...) / k with every operation rounded to float32"""
    rows = np.asarray(rows, F)
    k = rows.shape[1]
    root = np.sqrt(rows).astype(F)
    if kind == SCORE_KTH:
        return root[:, k - 1].copy()
    s = root[:, 0].copy()
    for q in range(1, k):
        s = (s + root[:, q]).astype(F)
    return (s / F(k)).astype(F)


def stats(scores) -> dict:
    """over the finite scores (a Gaussian that does not participate has +inf): n_scored, exact min and max, the float64 mean and the
    two-pass sample deviation; all 0 without any"""
    s = np.asarray(scores, F)
    s = s[np.isfinite(s)]
    m = int(s.size)
    if m == 0:
        return dict(n_scored=0, score_min=F(0), score_max=F(0), mean=0.0, std=0.0)
    d = s.astype(np.float64)
    mean = float(d.sum() / m)
    std = float(np.sqrt(((d - mean) ** 2).sum() / (m - 1))) if m > 1 else 0.0
    return dict(n_scored=m, score_min=s.min(), score_max=s.max(), mean=mean, std=std)


def threshold(mean, std, std_ratio) -> np.float32:
    """(float)(mean + (double)std_ratio * std)"""
    return F(np.float64(mean) + np.float64(F(std_ratio)) * np.float64(std))


def hit(scores, part, mode, lo=0.0, hi=0.0, std_ratio=0.0, st=None) -> np.ndarray:
    """bool[n]: RANGE participates and lo <= score <= hi; OUTLIERS participates, a finite score exists and score > threshold (from
    `st`, or the statistics of the scores)"""
    s = np.asarray(scores, F)
    part = np.asarray(part, bool)
    if mode == SELECT_RANGE:
        return part & (s >= F(lo)) & (s <= F(hi))
    st = stats(np.where(part, s, INF)) if st is None else st
    if st["n_scored"] == 0:
        return np.zeros(s.shape[0], bool)
    return part & (s > threshold(st["mean"], st["std"], std_ratio))


def kth_distance_median(pos, part, k=1) -> float:
    """the median distance to the k-th nearest other participant: the scale the tests' hints are multiples of"""
    r = brute(pos, part, k)[np.asarray(part, bool), k - 1]
    return float(np.sqrt(np.median(r[np.isfinite(r)])))
