"""gsx_model_apply_transform (spec/RENDER_SPEC.md §21) restated in numpy, for tests/test_transform_cpu.py and
tests/test_gpu_transform.py: the mode of a transform, its validity, and the position formula in float32, operation by operation
(numpy rounds every array operation to the array's type and fuses nothing).  Nothing here looks at csrc/transform_math.h: the two
are compared, not derived from one another."""
from __future__ import annotations

import numpy as np

IDENTITY, TRANSLATE, NO_ROTATION, FULL = 0, 1, 2, 3
F = np.float32


def _f3(a):
    return np.asarray(a, F).reshape(3)


def rotation_is_identity(quat) -> bool:
    """quat (0, 0, 0, +-1) as float32 values (-0 is 0)"""
    q = np.asarray(quat, F).reshape(4)
    return bool(np.all(q[:3] == 0) and abs(float(q[3])) == 1.0)


def mode(pos, quat, scale) -> int:
    p, s = _f3(pos), _f3(scale)
    rot, one = rotation_is_identity(quat), bool(np.all(s == 1))
    if rot and one and np.all(p == 0):
        return IDENTITY
    if not rot:
        return FULL
    return TRANSLATE if one else NO_ROTATION


def is_valid(pos, quat, scale, pivot) -> bool:
    q = np.asarray(quat, F).reshape(4)
    if not all(np.isfinite(a).all() for a in (_f3(pos), q, _f3(scale), _f3(pivot))):
        return False
    return float((q.astype(np.float64) ** 2).sum()) > 0.0


def quat_rows(quat) -> np.ndarray:
    """the float32 matrix of the quaternion AS GIVEN (spec §3; glam's Mat3::from_quat written out), row-major [3, 3]"""
    x, y, z, w = (F(v) for v in np.asarray(quat, F).reshape(4))
    with np.errstate(over="ignore", invalid="ignore"):
        x2, y2, z2 = F(x + x), F(y + y), F(z + z)
        xx, xy, xz, yy, yz, zz = F(x * x2), F(x * y2), F(x * z2), F(y * y2), F(y * z2), F(z * z2)
        wx, wy, wz = F(w * x2), F(w * y2), F(w * z2)
        one = F(1)
        return np.array([[F(one - F(yy + zz)), F(xy - wz), F(xz + wy)], [F(xy + wz), F(one - F(xx + zz)), F(yz - wx)],
                         [F(xz - wy), F(yz + wx), F(one - F(xx + yy))]], F)


def position(p, pos, quat, scale, pivot=(0.0, 0.0, 0.0)) -> np.ndarray:
    """p' of float32 points p [n, 3]: q = p - c, a = s * q, row r (((R_r0 a0 + R_r1 a1) + R_r2 a2) + t_r) + c_r, every operation
    rounded to float32; with a pivot that is exactly zero (as float32 values) the subtraction and the last addition are not performed"""
    p = np.ascontiguousarray(p, F)
    assert p.ndim == 2 and p.shape[1] == 3
    R, s, t, c = quat_rows(quat), _f3(scale), _f3(pos), _f3(pivot)
    use_pivot = not bool(np.all(c == 0))
    with np.errstate(over="ignore", invalid="ignore"):
        q = p - c[None, :] if use_pivot else p
        a = q * s[None, :]
        out = np.empty_like(p)
        for r in range(3):
            o = ((R[r, 0] * a[:, 0] + R[r, 1] * a[:, 1]) + R[r, 2] * a[:, 2]) + t[r]
            out[:, r] = o + c[r] if use_pivot else o
    assert out.dtype == F
    return out
