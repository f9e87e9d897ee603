"""The yardstick of gsx_model_export (spec §14), restated in numpy: the float32 upload conversion of a (rot, scale) pair (spec §2,
k_convert), the covariance error of an exported pair, the float64 path it is measured against (numpy.linalg.eigh of the stored
covariance, the same canonical form, rounded to float32), the canonical-form checks, and the covariance fixtures."""
from __future__ import annotations

import numpy as np

F = np.float32
#: the bound of §14: the code under test's worst error over a fixture is at most this many times the float64 path's
FACTOR = 4.0
GAUSSIAN_WORDS, PLY_WORDS = 56, 62


def upload_cov(rot, scale):
    """Spec §2's float32 upload conversion, operation for operation as k_convert: rot (n, 4) x, y, z, w; scale (n, 3) -> (n, 6)."""
    rot, scale = np.asarray(rot, F), np.asarray(scale, F)
    x, y, z, w = (rot[:, k] for k in range(4))
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz = x * x2, x * y2, x * z2
    yy, yz, zz = y * y2, y * z2, z * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    one = F(1.0)
    R = [one - (yy + zz), xy - wz, xz + wy, xy + wz, one - (xx + zz), yz - wx, xz - wy, yz + wx, one - (xx + yy)]
    M = [R[r * 3 + c] * scale[:, c] for r in range(3) for c in range(3)]

    def dot(a, b):
        return (M[3 * a] * M[3 * b] + M[3 * a + 1] * M[3 * b + 1]) + M[3 * a + 2] * M[3 * b + 2]

    with np.errstate(all="ignore"):
        return np.stack([dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)], axis=1).astype(F)


def cov_err(cov, rot, scale):
    """Per Gaussian: max |S' - S| / max |S| with S' the upload conversion of (rot, scale); 0 where S is all zero and so is S'."""
    cov = np.asarray(cov, F).astype(np.float64)
    got = upload_cov(rot, scale).astype(np.float64)
    num = np.abs(got - cov).max(axis=1)
    den = np.abs(cov).max(axis=1)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), num)


def quat_from_matrix(R):
    """(n, 3, 3) proper rotations -> (n, 4) x, y, z, w in float64: the branch on the largest of (R00, R11, R22, trace), normalised,
    w >= 0 (w == 0: the first non-zero of x, y, z positive)."""
    m = lambda r, c: R[:, r, c]  # noqa: E731
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    with np.errstate(all="ignore"):  # (every branch is evaluated for every matrix; the one that applies is well defined)
        st = np.sqrt(tr + 1.0) * 2.0
        s0 = np.sqrt(1.0 + m(0, 0) - m(1, 1) - m(2, 2)) * 2.0
        s1 = np.sqrt(1.0 + m(1, 1) - m(0, 0) - m(2, 2)) * 2.0
        s2 = np.sqrt(1.0 + m(2, 2) - m(0, 0) - m(1, 1)) * 2.0
        branches = [np.stack([(m(2, 1) - m(1, 2)) / st, (m(0, 2) - m(2, 0)) / st, (m(1, 0) - m(0, 1)) / st, 0.25 * st], axis=1),
                    np.stack([0.25 * s0, (m(0, 1) + m(1, 0)) / s0, (m(0, 2) + m(2, 0)) / s0, (m(2, 1) - m(1, 2)) / s0], axis=1),
                    np.stack([(m(0, 1) + m(1, 0)) / s1, 0.25 * s1, (m(1, 2) + m(2, 1)) / s1, (m(0, 2) - m(2, 0)) / s1], axis=1),
                    np.stack([(m(0, 2) + m(2, 0)) / s2, (m(1, 2) + m(2, 1)) / s2, 0.25 * s2, (m(1, 0) - m(0, 1)) / s2], axis=1)]
    use_t = (tr >= m(0, 0)) & (tr >= m(1, 1)) & (tr >= m(2, 2))
    use_0 = ~use_t & (m(0, 0) >= m(1, 1)) & (m(0, 0) >= m(2, 2))
    use_1 = ~use_t & ~use_0 & (m(1, 1) >= m(2, 2))
    which = np.where(use_t, 0, np.where(use_0, 1, np.where(use_1, 2, 3)))
    q = np.choose(which[:, None], branches)
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    # the sign: the first non-zero of w, x, y, z is positive
    order = q[:, [3, 0, 1, 2]]
    first = np.take_along_axis(order, np.argmax(order != 0, axis=1)[:, None], axis=1)[:, 0]
    return np.where(first[:, None] < 0, -q, q)


def through_log(scale):
    """linear scales as a PLY row carries them: the float32 logarithm, read back"""
    with np.errstate(all="ignore"):
        return np.exp(np.log(np.asarray(scale, F).astype(np.float64)).astype(F).astype(np.float64)).astype(F)


def solve_f64(cov):
    """The float64 path: eigh of the stored covariance, eigenvalues descending, determinant fixed, the canonical quaternion;
    scale = sqrt(max(lambda, 0)); both rounded to float32.  cov: (n, 6) finite float32."""
    c = np.asarray(cov, F).astype(np.float64)
    S = np.empty((c.shape[0], 3, 3))
    S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2] = (c[:, k] for k in range(6))
    S[:, 1, 0], S[:, 2, 0], S[:, 2, 1] = S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]
    lam, V = np.linalg.eigh(S)
    lam, V = lam[:, ::-1], V[:, :, ::-1].copy()
    V[:, :, 2] *= np.where(np.linalg.det(V) < 0, -1.0, 1.0)[:, None]
    return quat_from_matrix(V).astype(F), np.sqrt(np.maximum(lam, 0.0)).astype(F)


def check_canonical(rot, scale):
    """|rot| = 1 within 4 * 2^-24, w >= 0 (w == 0: first non-zero component positive), scales sorted, finite and >= 0."""
    rot, scale = np.asarray(rot, F), np.asarray(scale, F)
    norm = np.sqrt((rot.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(norm - 1.0).max() <= 4 * 2.0 ** -24, np.abs(norm - 1.0).max()
    assert (rot[:, 3] >= 0).all()
    for q in rot[rot[:, 3] == 0]:
        assert next(c for c in q[:3] if c != 0) > 0
    assert np.isfinite(scale).all() and (scale >= 0).all()
    assert (scale[:, 0] >= scale[:, 1]).all() and (scale[:, 1] >= scale[:, 2]).all()


# ---- fixtures: covariances as an upload makes them ----
def random_rot(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.sqrt((q * q).sum(axis=1))[:, None]).astype(F)


def fixture(name, n, seed):
    """(n, 6) float32 covariances: 'bench' (the bench generator's scales), 'loguniform' (e^-9 .. e^1), 'spheres' (three equal
    scales), 'flats' (one scale e^-30)."""
    rng = np.random.default_rng(seed)
    rot = random_rot(rng, n)
    if name == "bench":
        from wgpu_3dgs_viewer_app_amd import scene

        g = scene.synthetic_gaussians(n, seed, 3)
        rot, scale = g["rot"], g["scale"]
    elif name == "loguniform":
        scale = np.exp(rng.uniform(-9.0, 1.0, size=(n, 3))).astype(F)
    elif name == "spheres":
        scale = np.repeat(np.exp(rng.uniform(-9.0, 1.0, size=(n, 1))), 3, axis=1).astype(F)
    elif name == "flats":
        scale = np.exp(rng.uniform(-9.0, 1.0, size=(n, 3))).astype(F)
        scale[np.arange(n), rng.integers(0, 3, n)] = F(np.exp(-30.0))
    else:
        raise ValueError(name)
    return upload_cov(rot, scale)


FIXTURES = ("bench", "loguniform", "spheres", "flats")
