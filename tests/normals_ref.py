"""gsx_model_normals and gsx_model_select_normals (spec/RENDER_SPEC.md §26) restated in numpy, for tests/test_normals_cpu.py and
tests/test_gpu_normals.py.  `lists` is the definition of the neighbour list: the float32 d2 of every pair of participants
(tests/neighbors_ref.py: `_d2`, the one tests/knn_ref.py uses), the diagonal removed (self is excluded by index), each row ordered by
(d2, index), its first k entries; an entry whose d2 is +inf, or that does not exist, has the index NONE.  `fit` is the definition of
the plane: the float32 offsets in list order with the Gaussian's own offset 0 first, their mean and scatter summed in float64 in
that order, numpy.linalg.eigh for the eigenvalues and vectors (NOT the library's fixed-sweep Jacobi: the two are compared, not
derived from one another), the eigenvalues clamped at 0, the normal rounded to float32 and signed.  Nothing here includes
csrc/normals_math.h."""
from __future__ import annotations

import numpy as np

from tests.neighbors_ref import _d2

F = np.float32
MIN_K, MAX_K = 3, 16                    # GSX_NORMALS_MIN_K, GSX_NORMALS_MAX_K
ORIENT_CANONICAL, ORIENT_TOWARD = 0, 1  # GSX_NORMALS_ORIENT_*
SELECT_VARIATION, SELECT_FACING = 0, 1  # GSX_NORMALS_SELECT_*
ABS = 1                                 # GSX_NORMALS_ABS
NONE = 0xFFFFFFFF                       # GSX_NORMALS_NONE
INF = F(np.inf)
CERTAIN = 1e-6                          # a normal is compared where (l1 - l2) / l0 is at least this
NORMAL_ATOL = 2.0 ** -23                # per component, against eigh (tests/test_normals_cpu.py: where the bound comes from)
REF_VARIATION_ERROR = 2.0 ** -50        # eigh's own absolute error in l2 / trace: a few 2^-53 (tests/test_normals_cpu.py)
TINY_VARIATION = 2.0 ** -26             # below it that error exceeds a float32 ulp of the value: 1 ulp + REF_VARIATION_ERROR there
UNSIGNED_MAX = 4                        # rows of a fixture whose sign the reference cannot decide (`signed` false), at the most


def lists(pos, part, k, chunk=512):
    """(uint32[n, k], float32[n, k]): row i = the k smallest (d2(i, j), j) over the participants j != i; NONE / +inf where there are
    fewer, NONE where the d2 is +inf, and in the whole row of a Gaussian that does not participate"""
    pos = np.ascontiguousarray(pos, F)
    part = np.asarray(part, bool)
    n = pos.shape[0]
    idx = np.nonzero(part)[0]
    p = pos[idx]
    index = np.full((n, k), NONE, np.uint32)
    d2 = np.full((n, k), INF, F)
    for a in range(0, idx.size, chunk):
        d = _d2(p[a:a + chunk], p)
        rows = np.arange(d.shape[0])
        d[rows, a + rows] = INF
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)[None, :]
        key[rows, a + rows] = np.uint64(0xFFFFFFFFFFFFFFFF)  # self, by index
        key.sort(axis=1)
        have = min(k, max(idx.size - 1, 0))
        best = key[:, :have]
        dd = (best >> np.uint64(32)).astype(np.uint32).view(F)
        jj = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        d2[idx[a:a + chunk], :have] = dd
        index[idx[a:a + chunk], :have] = np.where(np.isfinite(dd), jj, np.uint32(NONE))
    return index, d2


def fitted_rows(d2) -> np.ndarray:
    """bool[n]: all k entries finite and the k-th above 0"""
    d2 = np.asarray(d2, F)
    return np.isfinite(d2[:, -1]) & (d2[:, -1] > 0)


def canonical_flip(n32) -> np.ndarray:
    """bool[m]: the first non-zero component of the float32 normal is negative"""
    x, y, z = n32[:, 0], n32[:, 1], n32[:, 2]
    return (x < 0) | ((x == 0) & ((y < 0) | ((y == 0) & (z < 0))))


def fit(pos, index, d2, orient=ORIENT_CANONICAL, toward=None) -> dict:
    """normal float32[n, 3] ((0, 0, 0) unfitted), variation float32[n] (+inf unfitted), fitted bool[n], and `gap` float64[n]:
    (l1 - l2) / l0, how certain the normal's direction is (0 unfitted), and `signed` bool[n]: the component (or, with TOWARD, the dot
    product) that decides the sign is further from 0 than NORMAL_ATOL can move it"""
    pos = np.ascontiguousarray(pos, F)
    n, k = index.shape
    normal = np.zeros((n, 3), F)
    variation = np.full(n, INF, F)
    gap = np.zeros(n)
    signed = np.zeros(n, bool)
    ok = fitted_rows(d2)
    rows = np.nonzero(ok)[0]
    if rows.size:
        with np.errstate(over="ignore"):
            off = (pos[index[rows].astype(np.int64)] - pos[rows][:, None, :]).astype(F)  # float32 differences, list order
        q = np.concatenate([np.zeros((rows.size, 1, 3)), off.astype(np.float64)], axis=1)  # q_0 = 0
        s = np.zeros((rows.size, 3))
        for m in range(k + 1):
            s = s + q[:, m]
        mu = s / float(k + 1)
        c = np.zeros((rows.size, 3, 3))
        for m in range(k + 1):
            e = q[:, m] - mu
            c = c + e[:, :, None] * e[:, None, :]
        w, v = np.linalg.eigh(c)  # ascending
        w = np.maximum(w, 0.0)
        l0, l1, l2 = w[:, 2], w[:, 1], w[:, 0]
        trace = (l0 + l1) + l2
        good = (trace > 0) & np.isfinite(trace)
        vec = v[:, :, 0]
        vec = vec / np.sqrt((vec[:, 0] ** 2 + vec[:, 1] ** 2) + vec[:, 2] ** 2)[:, None]
        n32 = vec.astype(F)
        flip = canonical_flip(n32)
        # the sign is certain where what decides it is further from 0 than the normals' tolerance can move it
        decides = np.abs(n32[np.arange(rows.size), np.argmax(n32 != 0, axis=1)]).astype(np.float64)
        sure = decides > NORMAL_ATOL
        if orient == ORIENT_TOWARD:
            t = np.asarray(toward, F).astype(np.float64)[None, :] - pos[rows].astype(np.float64)
            nd = n32.astype(np.float64)
            dot = (nd[:, 0] * t[:, 0] + nd[:, 1] * t[:, 1]) + nd[:, 2] * t[:, 2]
            flip = np.where(dot != 0, dot < 0, flip)
            sure = np.where(dot != 0, np.abs(dot) > NORMAL_ATOL * np.abs(t).sum(axis=1), sure)
        signed[rows[good]] = sure[good]
        n32 = np.where(flip[:, None], -n32, n32) + F(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = (l2 / trace).astype(F)
            g = np.where(l0 > 0, (l1 - l2) / l0, 0.0)
        normal[rows[good]] = n32[good]
        variation[rows[good]] = var[good]
        gap[rows[good]] = g[good]
    return dict(normal=normal, variation=variation, fitted=np.isfinite(variation), gap=gap, signed=signed)


def stats(variation) -> dict:
    """over the fitted (finite variation): n_fitted, exact min and max, the float64 mean; all 0 without any"""
    s = np.asarray(variation, F)
    s = s[np.isfinite(s)]
    m = int(s.size)
    if m == 0:
        return dict(n_fitted=0, variation_min=F(0), variation_max=F(0), mean=0.0)
    return dict(n_fitted=m, variation_min=s.min(), variation_max=s.max(), mean=float(s.astype(np.float64).sum() / m))


def direction(d) -> np.ndarray:
    """dir normalised in float64, rounded to float32"""
    d = np.asarray(d, F).astype(np.float64)
    return (d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])).astype(F)


def cosine(normal, d) -> np.ndarray:
    """c = (nx dx + ny dy) + nz dz, every operation rounded to float32"""
    nrm, d = np.asarray(normal, F), direction(d)
    return ((nrm[:, 0] * d[0]).astype(F) + (nrm[:, 1] * d[1]).astype(F)).astype(F) + (nrm[:, 2] * d[2]).astype(F)


def hit(normal, variation, mode, lo, hi, d=None, flags=0) -> np.ndarray:
    """bool[n]: fitted and lo <= the measure <= hi"""
    variation = np.asarray(variation, F)
    c = variation
    if mode == SELECT_FACING:
        c = cosine(normal, d).astype(F)
        if flags & ABS:
            c = np.abs(c)
    return np.isfinite(variation) & (c >= F(lo)) & (c <= F(hi))


# ---- the fixture families of the tests ------------------------------------------------------------------------------------------------
def uniform_cube(n, seed=0):
    return np.random.default_rng(seed).random((n, 3)).astype(F)


def noisy_sheet(n, seed=1, noise=0.002):
    """a unit square sheet, tilted, with a little noise across it"""
    rng = np.random.default_rng(seed)
    uv = rng.random((n, 2))
    w = rng.normal(0.0, noise, n)
    a, b, c = np.array([1.0, 0.2, 0.1]), np.array([-0.1, 1.0, 0.3]), np.array([0.05, -0.32, 1.0])
    return (uv[:, :1] * a + uv[:, 1:] * b + w[:, None] * c).astype(F)


def far_cloud(n, seed=2):
    """a 1 cm cloud at offset 1000: the float32 coordinates carry 6e-5 of absolute rounding"""
    return (np.random.default_rng(seed).random((n, 3)) * 0.01 + 1000.0).astype(F)


FAMILIES = (("cube", uniform_cube), ("sheet", noisy_sheet), ("far", far_cloud))
