"""gsx_model_bounds restated in numpy (spec/RENDER_SPEC.md §11), for tests/test_bounds_cpu.py and tests/test_gpu_bounds.py:
the exact fields over a set of kept positions, the one-level 2048-bin trimmed box of csrc/bounds_math.h in float32, and the
bounds the trimmed box has to meet whatever the method."""
from __future__ import annotations

import numpy as np

f32 = np.float32
BINS = 2048
MASKED, SKIP_HIDDEN, SELECTED = 1, 2, 4


def bits(words: np.ndarray, n: int) -> np.ndarray:
    """bit i of a ceil(n / 32)-word bitset, as bool[n]"""
    return ((np.asarray(words, np.uint32)[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


def trim_k(count: int, trim_permille: int) -> int:
    return count * trim_permille // 1000


class Axis:
    """bounds_axis: 2048 equal bins over [lo, hi] in float32; not live when the range is zero, not a finite float32, or so small that
    a bin's width is 0 or the scale is not finite"""

    def __init__(self, lo, hi):
        self.lo, self.hi = f32(lo), f32(hi)
        with np.errstate(over="ignore", invalid="ignore"):
            rng = f32(self.hi - self.lo)
            self.live = bool(rng > 0 and np.isfinite(rng) and f32(rng / f32(BINS)) > 0 and np.isfinite(f32(f32(BINS) / rng)))
        self.width = f32(rng / f32(BINS)) if self.live else f32(0)
        self.scale = f32(f32(BINS) / rng) if self.live else f32(0)

    def edges(self) -> np.ndarray:
        """bounds_edge for b = 0 .. 2048"""
        e = np.minimum(self.hi, (self.lo + np.arange(BINS + 1, dtype=f32) * self.width).astype(f32))
        e[0], e[BINS] = self.lo, self.hi
        return e

    def bins(self, v: np.ndarray) -> np.ndarray:
        """bounds_bin: the estimate, moved until edge(b) <= v <= edge(b + 1)"""
        v = np.asarray(v, f32)
        e = self.edges()
        t = ((v - self.lo).astype(f32) * self.scale).astype(f32)
        b = np.where(t >= f32(BINS - 1), BINS - 1, np.where(t > 0, np.minimum(t, f32(BINS - 1)).astype(np.int64), 0))
        while True:
            down = (b > 0) & (v < e[b])
            if not down.any():
                break
            b = b - down
        while True:
            up = (b + 1 < BINS) & (v > e[np.minimum(b + 1, BINS)])
            if not up.any():
                break
            b = b + up
        return b


def scan(hist: np.ndarray, k: int, reverse: bool):
    """bounds_scan: position in scan order of the first bin whose cumulative count exceeds k, and the count in front of it"""
    h = np.asarray(hist, np.int64)[::-1] if reverse else np.asarray(hist, np.int64)
    cum = np.cumsum(h)
    over = np.nonzero(cum > k)[0]
    if over.size == 0:
        return len(h), int(cum[-1])
    return int(over[0]), int(cum[over[0]] - h[over[0]])


def trimmed_axis(values: np.ndarray, k: int):
    """the one-level method on one axis: (trim_min, trim_max) as float32"""
    values = np.asarray(values, f32)
    ax = Axis(values.min(), values.max())
    if not ax.live:
        return ax.lo, ax.hi
    hist = np.bincount(ax.bins(values), minlength=BINS)
    e = ax.edges()
    pos_lo, _ = scan(hist, k, False)
    pos_hi, _ = scan(hist, k, True)
    return (e[pos_lo] if pos_lo < BINS else ax.lo), (e[BINS - pos_hi] if pos_hi < BINS else ax.hi)


def trim_limits(values: np.ndarray, k: int):
    """What ANY trimmed box has to meet on one axis, from the sorted counted values s, w = (max - min) / 2048 and
    e = 4 * 2^-23 * max(|min|, |max|):  s[k] - w - e <= trim_min <= s[k] + e  and  s[n-1-k] - e <= trim_max <= s[n-1-k] + w + e.
    Returns ((min of trim_min, max of trim_min), (min of trim_max, max of trim_max)) in float64."""
    s = np.sort(np.asarray(values, np.float64))
    n = s.size
    w = (s[-1] - s[0]) / BINS
    e = 4.0 * 2.0 ** -23 * max(abs(s[0]), abs(s[-1]))
    return (s[k] - w - e, s[k] + e), (s[n - 1 - k] - e, s[n - 1 - k] + w + e)


def reference(pos: np.ndarray, keep: np.ndarray) -> dict:
    """The exact fields over pos[keep] (pos: float32 [n, 3] as uploaded): count, n_nonfinite, min, max, center in float32 as the
    header defines them, mean64 in float64, and the counted positions themselves."""
    p = np.asarray(pos, f32)[np.asarray(keep, bool)]
    fin = np.isfinite(p).all(axis=1)
    c = p[fin]
    out = {"count": int(c.shape[0]), "n_nonfinite": int((~fin).sum()), "counted": c}
    if c.shape[0] == 0:
        for name in ("min", "max", "center"):
            out[name] = np.zeros(3, f32)
        out["mean64"] = np.zeros(3)
        return out
    out["min"], out["max"] = c.min(axis=0), c.max(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        out["center"] = (f32(0.5) * (out["min"] + out["max"]).astype(f32)).astype(f32)
    out["mean64"] = c.astype(np.float64).mean(axis=0)
    return out
