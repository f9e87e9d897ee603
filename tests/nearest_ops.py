"""What the GPU tests of the nearest search across models (tests/test_gpu_nearest.py) need beside tests/model_ops.py: a scene with
given positions, a model that carries every plane a filter reads, and the Gaussians a filter lets pass."""
import numpy as np

from tests import common
from tests import extract_ref as X
from tests.model_ops import load
from wgpu_3dgs_viewer_app_amd import query
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as EF


def with_pos(pos):
    """small_scene's Gaussians at the given positions"""
    g = common.small_scene(pos.shape[0], 5, 0)
    g["pos"] = pos
    return g


def filter_model(v, n, seed, key):
    """a model with a mask, a selection (garbage in both tails) and stored edits (some ENABLED + HIDDEN), NaN and infinite positions;
    returns the host arrays: the Gaussians, the mask, the selection, the stored edit flags"""
    g = common.small_scene(n, seed, 0)
    g["pos"][5, 0], g["pos"][n // 2, 0], g["pos"][n - 1, 0], g["pos"][7, 1] = np.nan, np.inf, -np.inf, np.nan
    rng = np.random.default_rng(seed)
    mask, sel = rng.random(n) < 0.6, rng.random(n) < 0.4
    mask[[0, n - 1]], sel[[0, n // 2]] = True, True
    edits = query.default_edits(n)
    edits["flag"][0::3] = int(EF.ENABLED | EF.HIDDEN)
    edits["flag"][1::3] = int(EF.ENABLED)
    edits["flag"][5::7] |= int(EF.HIDDEN)  # (HIDDEN without ENABLED hides nothing)
    load(v, g, key)
    bufs = v.models[key].gaussian_buffers
    bufs.mask_buffer.upload(X.words(mask, True))
    bufs.selection_buffer.upload(X.words(sel, True))
    bufs.gaussians_edit_buffer.upload(edits)
    return g, mask, sel, bufs.gaussians_edit_buffer.download()["flag"]


def passes(n, flt, mask=None, sel=None, flags=None):
    """bool[n]: the Gaussians that pass the GSX_BOUNDS_* filter `flt` (tests/extract_ref.py)"""
    out = np.zeros(n, bool)
    out[X.kept(n, flt, 0, mask, sel, flags)] = True
    return out
