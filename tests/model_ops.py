"""What the GPU tests of the model operations (gsx_model_extract, gsx_model_merge, gsx_model_export and the filter they share with
gsx_model_bounds) all need: loading a model, its length, its resident planes, a few frames of it, and the eight pod kinds."""
import ctypes as C

import numpy as np

from wgpu_3dgs_viewer_app_amd import _lib, camera
from wgpu_3dgs_viewer_app_amd.viewer import Cov3dKind, GaussianDisplayMode, GaussianShDegree, ShKind

W, H = 96, 64
KINDS = [(sh, cov) for sh in ShKind for cov in Cov3dKind]
KIND_IDS = [f"{sh.name}-{cov.name}" for sh, cov in KINDS]


def load(v, g, key="src", mt=None):
    v.add_model(key, g.shape[0])
    v.models[key].gaussian_buffers.gaussians_buffer.update_range(0, g)
    if mt is not None:
        v.update_model_transform(key, *mt)


def model_len(v, key):
    """(status, length) of gsx_model_len"""
    n = C.c_uint64()
    return v._L.gsx_model_len(v._h, key.encode(), C.byref(n)), int(n.value)


def pod(v, key="src", sh_zeros=False):
    """the resident planes, dequantised: pos, color, sh, cov3d; the sh of a viewer without SH planes is an empty (n, 0) array, or with
    `sh_zeros` the (n, 45) zeros such a model stands for"""
    if v.sh != ShKind.Remove:
        return v.models[key].gaussian_buffers.gaussians_buffer.download_pod()
    n = model_len(v, key)[1]
    pos, color, cov = np.empty((n, 3), np.float32), np.empty(n, np.uint32), np.empty((n, 6), np.float32)
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    _lib.check(v._L.gsx_model_download_pod(v._h, key.encode(), f32p(pos), color.ctypes.data_as(C.POINTER(C.c_uint32)), None, f32p(cov)))
    return pos, color, np.zeros((n, 45), np.float32) if sh_zeros else np.empty((n, 0), np.float32), cov


def frames(v, keys, poses=(5, 6, 7), size=(W, H), sh_deg=3):
    """one frame per pose (a camera path: the later ones are speculated), each downloaded"""
    out = []
    for pose in poses:
        v.update_camera(camera.orbit_pose(pose), size)
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(sh_deg), False)
        v.render_frame(list(keys))
        out.append(v.download_framebuffer())
    return out
