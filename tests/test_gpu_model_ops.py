"""GPU: one filter, four readers.  gsx_model_bounds, gsx_model_extract, gsx_model_merge and gsx_model_export build their filter in one
place (csrc/gsx_state.h: model_filter) and the last three share one kept-set pass: for every filter value the four must count the
same Gaussians, the ones tests/extract_ref.py keeps.  Sizes: the word and workgroup tails of the bounds chunk and the extract group."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import extract_ref as X
from tests.model_ops import load
from wgpu_3dgs_viewer_app_amd import _lib, query
from wgpu_3dgs_viewer_app_amd.query import GaussianEditFlag as F
from wgpu_3dgs_viewer_app_amd.viewer import MultiModelViewer, ShKind

pytestmark = pytest.mark.gpu
SIZES = [1, 31, 32, 33, 1023, 1024, 1025, 2049]


def _export_count(v, key, flt, invert):
    """gsx_model_export with out = NULL: the count alone"""
    desc = _lib.ExportDesc(flt, _lib.GSX_EXTRACT_INVERT if invert else 0, _lib.GSX_EXPORT_GAUSSIANS, 0, 0)
    count = C.c_uint64(0xDEAD)
    _lib.check(v._L.gsx_model_export(v._h, key.encode(), C.byref(desc), None, 0, C.byref(count)))
    return int(count.value)


def _counts(v, key, flt, invert):
    """what extract, merge (of that one source) and export count; the models the first two make are removed again"""
    got = {"extract": v.models[key].extract("x", flt, invert=invert)}
    total, per_source = v.merge("m", [key], flt, invert=invert)
    assert per_source == [total]
    got["merge"] = total
    for made in ("x", "m"):
        if made in v.models:
            v.remove_model(made)
    got["export"] = _export_count(v, key, flt, invert)
    return got


@pytest.mark.parametrize("n", SIZES)
def test_one_filter_four_readers(n):
    rng = np.random.default_rng(1000 + n)
    g = common.small_scene(n, 23, 0)
    mask, sel = rng.random(n) < 0.6, rng.random(n) < 0.5
    edits = query.default_edits(n)
    edits["flag"] = rng.choice(np.uint32([0, int(F.ENABLED), int(F.HIDDEN), int(F.ENABLED | F.HIDDEN)]), n)
    with MultiModelViewer(sh=ShKind.Remove) as v:
        for key in ("src", "nosel"):  # the second: the same model without a selection
            load(v, g, key)
            bufs = v.models[key].gaussian_buffers
            bufs.mask_buffer.upload(X.words(mask, True))  # (garbage above n)
            bufs.gaussians_edit_buffer.upload(edits)
        v.models["src"].gaussian_buffers.selection_buffer.upload(X.words(sel, True))
        stored = v.models["src"].gaussian_buffers.gaussians_edit_buffer.download()["flag"]
        cases = [("src", flt, sel) for flt in range(8)] + [("nosel", flt, None) for flt in (X.SELECTED, X.MASKED | X.SKIP_HIDDEN | X.SELECTED)]
        for key, flt, selection in cases:
            want = X.kept(n, flt, 0, mask, selection, stored).size
            if selection is None:
                assert want == 0  # SELECTED without a selection: none
            elif n >= 32 and flt:
                assert 0 < want < n, (flt, "a degenerate scene would pass trivially")
            b = v.models[key].bounds(masked=bool(flt & X.MASKED), skip_hidden=bool(flt & X.SKIP_HIDDEN), selected=bool(flt & X.SELECTED))
            assert b.count + b.n_nonfinite == want, (key, flt)
            assert _counts(v, key, flt, False) == dict(extract=want, merge=want, export=want), (key, flt)
            assert _counts(v, key, flt, True) == dict(extract=n - want, merge=n - want, export=n - want), (key, flt, "invert")
