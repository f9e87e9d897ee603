"""gsx_model_extract's kept set (spec/RENDER_SPEC.md §12) restated in numpy, for tests/test_extract_cpu.py and tests/test_gpu_extract.py:
which Gaussians of a model a filter keeps, from the model's mask, selection and stored edit flags, and the bit-plane helpers the
tests share.  Nothing here looks at csrc/extract_math.h: the two are compared, not derived from one another."""
from __future__ import annotations

import numpy as np

MASKED, SKIP_HIDDEN, SELECTED = 1, 2, 4  # GSX_BOUNDS_*
INVERT, DROP_EDITS = 1, 2  # GSX_EXTRACT_*
EDIT_ENABLED, EDIT_HIDDEN = 1, 2  # GSX_EDIT_*
GROUP = 1024  # Gaussians per workgroup of the keep and scatter kernels (csrc/extract_math.h: kExtractGroup)
SCAN_PASS = 256  # partials per pass of the scan kernel (kExtractScanPass)


def bits(words, n: int) -> np.ndarray:
    """bool[n] from ceil(n / 32) little-endian bit-plane words; whatever the last word holds at or above n is dropped"""
    w = np.ascontiguousarray(words, dtype="<u4")
    assert w.size == (n + 31) // 32
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def words(flags, garbage_tail: bool = False) -> np.ndarray:
    """ceil(n / 32) words from bool[n]; garbage_tail sets every bit of the last word at or above n"""
    b = np.asarray(flags, bool)
    n = b.size
    padded = np.zeros(((n + 31) // 32) * 32, np.uint8)
    padded[:n] = b
    if garbage_tail:
        padded[n:] = 1
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def hidden(edit_flags) -> np.ndarray:
    """a stored edit hides its Gaussian when its flag has ENABLED and HIDDEN (HIDDEN alone hides nothing)"""
    f = np.asarray(edit_flags, np.uint32)
    return ((f & EDIT_ENABLED) != 0) & ((f & EDIT_HIDDEN) != 0)


def kept(n: int, filter_bits: int, flags: int = 0, mask=None, selection=None, edit_flags=None) -> np.ndarray:
    """Indices of the Gaussians gsx_model_extract keeps, ascending (= their order in the new model).  mask / selection: bool[n] or
    None (no mask: all pass; no selection: none pass); edit_flags: uint32[n] stored flags or None (no edit records: none hidden)."""
    ok = np.ones(n, bool)
    if filter_bits & MASKED and mask is not None:
        ok &= np.asarray(mask, bool)
    if filter_bits & SKIP_HIDDEN and edit_flags is not None:
        ok &= ~hidden(edit_flags)
    if filter_bits & SELECTED:
        ok &= np.asarray(selection, bool) if selection is not None else np.zeros(n, bool)
    if flags & INVERT:
        ok = ~ok
    return np.nonzero(ok)[0]
