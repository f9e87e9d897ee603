"""The model properties (gsx_model_property_values, gsx_model_histogram, gsx_model_select_range; spec/RENDER_SPEC.md §17) restated
in numpy float32, for tests/test_property_cpu.py (against csrc/property_math.h played by tests/property_driver.cpp) and
tests/test_gpu_property.py (against the device): the value of properties 0..9 from the position and the colour word, the bins of a
range, the histogram of downloaded values, the hit set of a select and the selection op on bit planes.  The scales (properties
10..12) are not restated: their yardstick is gsx_model_export."""
from __future__ import annotations

import numpy as np

F = np.float32
(POS_X, POS_Y, POS_Z, RED, GREEN, BLUE, OPACITY, HUE, SATURATION, VALUE, SCALE_MAX, SCALE_MID, SCALE_MIN, COUNT) = range(14)
WORLD, AUTO_RANGE = 1, 4
MAX_BINS = 4096
SET, ADD, REMOVE = 0, 1, 2
BIN_COUNTS = (1, 2, 255, 256, 4096)
FLT_MAX = F(3.402823466e+38)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(F)


def finite(v):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(v, F)) <= FLT_MAX


# ---- values ----
def world_positions(pos, R, s, t):
    """p' = R (s * p) + t, each row ((R0 a0 + R1 a1) + R2 a2) + t in float32"""
    pos, R, s, t = np.asarray(pos, F), np.asarray(R, F), np.asarray(s, F), np.asarray(t, F)
    with np.errstate(all="ignore"):
        a = pos * s[None, :]
        return np.stack([((R[3 * k] * a[:, 0] + R[3 * k + 1] * a[:, 1]) + R[3 * k + 2] * a[:, 2]) + t[k] for k in range(3)], axis=1).astype(F)


def rgb_to_hsv(r, g, b):
    """edit_math.h's em_rgb_to_hsv, element-wise in float32"""
    r, g, b = (np.asarray(c, F) for c in (r, g, b))
    with np.errstate(all="ignore"):
        mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
        d = (mx - mn).astype(F)
        s = np.where(mx > 0, d / np.where(mx > 0, mx, F(1)), F(0)).astype(F)
        safe = np.where(d > 0, d, F(1))
        hr = ((g - b) / safe).astype(F)
        hr = np.where(hr < 0, hr + F(6), hr).astype(F)
        hg = ((b - r) / safe + F(2)).astype(F)
        hb = ((r - g) / safe + F(4)).astype(F)
        h = np.where(~(d > 0), F(0), np.where(mx == r, hr, np.where(mx == g, hg, hb))).astype(F)
        h = (h / F(6)).astype(F)
    return h, s, mx.astype(F)


def values_pc(prop, pos, color, transform=None):
    """Properties 0..9 of Gaussians with stored positions `pos` (n, 3) and colour words `color` (n,); transform: (R, s, t) of a
    GSX_PROP_WORLD position under a transform that is not the identity"""
    pos, color = np.asarray(pos, F), np.asarray(color, np.uint32)
    if prop <= POS_Z:
        return (pos if transform is None else world_positions(pos, *transform))[:, prop].copy()
    byte = lambda k: (((color >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(F) / F(255)).astype(F)  # noqa: E731
    if prop <= OPACITY:
        return byte(prop - RED)
    h, s, v = rgb_to_hsv(byte(0), byte(1), byte(2))
    return {HUE: h, SATURATION: s, VALUE: v}[prop]


# ---- min / max in the order -inf < ... < -0 < +0 < ... < +inf ----
def key(v):
    u = bits(v).astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def min_max(v):
    """(min, max) of a non-empty array of finite float32 by key: exact, -0 below +0"""
    v = np.asarray(v, F)
    k = key(v)
    return v[np.argmin(k)], v[np.argmax(k)]


# ---- bins ----
class Range:
    def __init__(self, lo, hi, bins):
        self.lo, self.hi, self.bins = F(lo), F(hi), max(int(bins), 1)
        fb = F(self.bins)
        with np.errstate(all="ignore"):
            rng = F(self.hi - self.lo)
            self.live = bool(rng > 0 and finite(rng) and F(rng / fb) > 0 and finite(F(fb / rng)))
            self.width = F(rng / fb) if self.live else F(0)
            self.scale = F(fb / rng) if self.live else F(0)

    def edge(self, b):
        b = np.asarray(b, np.int64)
        with np.errstate(all="ignore"):
            mid = np.minimum(self.hi, (self.lo + (b.astype(F) * self.width).astype(F)).astype(F)).astype(F)
        return np.where(b == 0, self.lo, np.where(b >= self.bins, self.hi, mid)).astype(F)

    def bin(self, v):
        """the bin of values lo <= v <= hi"""
        v = np.asarray(v, F)
        if not self.live:
            return np.zeros(v.shape, np.int64)
        with np.errstate(all="ignore"):
            t = ((v - self.lo).astype(F) * self.scale).astype(F)
        b = np.where(t >= F(self.bins - 1), self.bins - 1, np.where(t > 0, np.minimum(t, F(self.bins)).astype(np.int64), 0)).astype(np.int64)
        while True:
            m = (b > 0) & (v < self.edge(b))
            if not m.any():
                break
            b[m] -= 1
        while True:
            m = (b + 1 < self.bins) & (v > self.edge(b + 1))
            if not m.any():
                break
            b[m] += 1
        return b


NONFINITE, BELOW, ABOVE = -1, -2, -3


def classify(r, v):
    v = np.asarray(v, F)
    out = np.full(v.shape, NONFINITE, np.int64)
    fin = finite(v)
    with np.errstate(all="ignore"):
        below, above = fin & (v < r.lo), fin & (v > r.hi)
    inside = fin & ~below & ~above
    out[below], out[above] = BELOW, ABOVE
    out[inside] = r.bin(v[inside])
    return out


def histogram(values, passes, bins, lo=None, hi=None):
    """gsx_model_histogram of downloaded `values` over the Gaussians `passes` (bool): lo is None = GSX_HIST_AUTO_RANGE.  Returns a
    dict with the gsx_histogram_t fields and `bins`."""
    values, passes = np.asarray(values, F), np.asarray(passes, bool)
    fin = finite(values)
    counted = values[passes & fin]
    out = dict(count=int(counted.size), below=0, above=0, n_nonfinite=int((passes & ~fin).sum()), lo=F(0) if lo is None else F(lo),
               hi=F(0) if hi is None else F(hi), min=F(0), max=F(0), bins=np.zeros(bins, np.uint64))
    if counted.size == 0:
        return out
    out["min"], out["max"] = min_max(counted)
    if lo is None:
        out["lo"], out["hi"] = out["min"], out["max"]
    cls = classify(Range(out["lo"], out["hi"], bins), counted)
    out["below"], out["above"] = int((cls == BELOW).sum()), int((cls == ABOVE).sum())
    out["bins"] = np.bincount(cls[cls >= 0], minlength=bins).astype(np.uint64)
    return out


def hits(values, passes, lo, hi, bins=0, bin_lo=0, bin_hi=0):
    """the hit set of gsx_model_select_range, as a bool array"""
    cls = classify(Range(lo, hi, bins), values)
    hit = np.asarray(passes, bool) & (cls >= 0)
    if bins:
        hit &= (cls >= bin_lo) & (cls <= bin_hi)
    return hit


def apply_op(op, old, hit):
    """the selection afterwards (bool arrays): Set, Add, Remove"""
    old, hit = np.asarray(old, bool), np.asarray(hit, bool)
    return hit.copy() if op == SET else ((old | hit) if op == ADD else (old & ~hit))


def words(flags, garbage_tail=False):
    """bool[n] -> ceil(n / 32) u32 words, bit i % 32 of word i // 32; garbage_tail: the bits at and above n set"""
    flags = np.asarray(flags, bool)
    n = flags.size
    padded = np.zeros(((n + 31) // 32) * 32, bool)
    padded[:n] = flags
    if garbage_tail:
        padded[n:] = True
    return (padded.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def unwords(w, n):
    w = np.asarray(w, np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)[:n]


def next_up(v, k=1):
    """the float32 k ulps above v (below for k < 0), by key"""
    kk = (key(np.array([v], F)).astype(np.int64) + k).astype(np.uint32)
    return from_bits(np.where(kk & np.uint32(0x80000000), kk & np.uint32(0x7FFFFFFF), ~kk).astype(np.uint32))[0]
