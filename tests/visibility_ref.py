"""The reference of gsx_model_visibility (spec/RENDER_SPEC.md §24) in plain numpy: the walk alone.  Its input is what calls from
before section 24 return — a projection (``mean2d``, ``conic_opacity``) and complete per-tile lists (``tile_offsets``, ``tile_list``), the
device's own (``gsx_model_download_projection``, ``gsx_model_download_tile_lists`` after a ``progressive = 0`` frame) or the oracle's
(``oracle.project``, ``oracle.tile_lists``) — so a comparison isolates the new kernel.

Per pixel, front to back (spec §6): ``q`` in float32 with the spec's operation order, ``fmaf`` emulated through float64 (the product of
two float32 is exact there), so the support decisions ``0 <= q <= k2`` are the device's exactly; ``exp``, alpha, ``w = T * alpha`` and
``T *= 1 - alpha`` in float64.  The pixel closes at ``T < t_epsilon``.  The device computes T in float32, so that decision can differ
where T lies within ``tol = (L_max + 2) * 2^-21`` of ``t_epsilon`` (L_max: the longest tile list; §24 derives the bound): a decision is
CERTAIN when T is further away than that.  After an uncertain decision the reference keeps walking the pixel as if it were open (the
device either does the same or has closed it) and every later pair of that pixel is an UNCERTAIN pair, until T < t_epsilon - tol
closes it for certain.  So per Gaussian the reference returns a range:

  ``peak_lo`` / ``weight_lo`` / ``pixels_lo``   over the certain pairs alone,
  ``peak_hi`` / ``weight_hi`` / ``pixels_hi``   with the uncertain pairs as well,

equal for every Gaussian without an uncertain pair (``uncertain[g]`` False).  ``T`` and ``rgb`` are the frame under the reference's
own decisions (closed at T < t_epsilon)."""
import dataclasses

import numpy as np

F = np.float32
TILE = 16


def tol(l_max: int) -> float:
    """spec §24: one ulp of the hardware exp2 and of its argument per alpha, two roundings per T step, over at most L_max steps"""
    return (l_max + 2) * 2.0 ** -21


def weight_tol(l_max: int, pixels) -> np.ndarray:
    """... per pixel, plus half a unit of the 2^-24 fixed point"""
    return np.asarray(pixels, np.float64) * (tol(l_max) + 2.0 ** -25)


def fmaf(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


@dataclasses.dataclass
class Ref:
    peak_lo: np.ndarray
    peak_hi: np.ndarray
    weight_lo: np.ndarray
    weight_hi: np.ndarray
    pixels_lo: np.ndarray
    pixels_hi: np.ndarray
    uncertain: np.ndarray   # bool per Gaussian: it has an uncertain pair
    T: np.ndarray           # (h, w) float64
    rgb: np.ndarray | None  # (h, w, 3) float64, when colours were given
    l_max: int
    n_pairs: int            # the reference's own blended pairs
    margin: float           # the smallest |T - t_epsilon| / tol over the CERTAIN decisions (> 1)


def walk(mean2d, conic_opacity, tile_offsets, tile_list, w, h, k2, alpha_max=1.0, alpha_min=0.0, t_eps=1e-4, display_mode=0, rgb=None) -> Ref:
    mean2d = np.asarray(mean2d, F)
    co = np.asarray(conic_opacity, F)
    n = mean2d.shape[0]
    off = np.asarray(tile_offsets, np.int64)
    lst = np.asarray(tile_list, np.int64)
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    assert off.shape[0] == tiles_x * tiles_y + 1
    l_max = int(np.diff(off).max()) if off.shape[0] > 1 else 0
    tl = tol(l_max)
    k2, t_eps, alpha_max, alpha_min = F(k2), float(F(t_eps)), float(F(alpha_max)), float(F(alpha_min))
    peak_lo, peak_hi = np.zeros(n), np.zeros(n)
    weight_lo, weight_hi = np.zeros(n), np.zeros(n)
    pix_lo, pix_hi = np.zeros(n, np.int64), np.zeros(n, np.int64)
    T_out = np.ones((h, w))
    rgb_out = np.zeros((h, w, 3)) if rgb is not None else None
    n_pairs, margin = 0, np.inf
    two_b = (F(2.0) * co[:, 1]).astype(F)
    for t in range(tiles_x * tiles_y):
        tx, ty = t % tiles_x, t // tiles_x
        ys, xs = np.mgrid[ty * TILE:min(ty * TILE + TILE, h), tx * TILE:min(tx * TILE + TILE, w)]
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        pxf, pyf = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
        T = np.ones(xs.shape[0])          # as if open
        T_own = np.ones(xs.shape[0])      # under the reference's own decisions
        C_own = np.zeros((xs.shape[0], 3))
        own_open = T_own >= t_eps
        open_ = np.ones(xs.shape[0], bool)   # not closed for certain
        zone = np.zeros(xs.shape[0], bool)   # an uncertain decision lies behind: the pairs from here on are uncertain
        for g in lst[off[t]:off[t + 1]]:
            if not open_.any():
                break
            dx, dy = pxf - mean2d[g, 0], pyf - mean2d[g, 1]
            inner = fmaf(np.broadcast_to(co[g, 2], dy.shape) * dy, dy, (two_b[g] * dx) * dy)
            q = fmaf(co[g, 0] * dx, dx, inner)
            hit = (q >= 0) & (q <= k2)
            if not hit.any():
                continue
            e = np.exp(-0.5 * q.astype(np.float64)) if display_mode == 0 else np.ones(q.shape[0])
            alpha = np.minimum(alpha_max, float(co[g, 3]) * e)
            blend = hit & ~(alpha < alpha_min)
            # the reference's own frame
            b_own = blend & own_open
            w_own = np.where(b_own, T_own * alpha, 0.0)
            if rgb is not None:
                C_own += w_own[:, None] * np.asarray(rgb[g], np.float64)[None]
            T_own = np.where(b_own, T_own * (1.0 - alpha), T_own)
            own_open &= T_own >= t_eps
            n_pairs += int(b_own.sum())
            # the range
            b = blend & open_
            wgt = np.where(b, T * alpha, 0.0)
            sure, maybe = b & ~zone, b & zone
            if sure.any():
                peak_lo[g] = max(peak_lo[g], wgt[sure].max())
                weight_lo[g] += wgt[sure].sum()
                pix_lo[g] += int(sure.sum())
            if b.any():
                peak_hi[g] = max(peak_hi[g], wgt[b].max())
                weight_hi[g] += wgt[b].sum()
                pix_hi[g] += int(b.sum())
            T = np.where(b, T * (1.0 - alpha), T)
            d = np.abs(T - t_eps)
            decided = b & (d > tl)
            if decided.any():
                margin = min(margin, float(d[decided].min() / tl))
            zone |= b & (d <= tl)
            open_ &= ~(b & (T < t_eps - tl))
        T_out[ys, xs] = T_own
        if rgb is not None:
            rgb_out[ys, xs] = C_own
    return Ref(peak_lo, peak_hi, weight_lo, weight_hi, pix_lo, pix_hi, pix_hi != pix_lo, T_out, rgb_out, l_max, n_pairs, margin)


def check(ref: Ref, peak, weight, pixels):
    """The assertions of §24's test 2 for one call's planes; returns the largest deviations seen (peak, weight / its bound)."""
    peak, weight, pixels = np.asarray(peak, np.float64), np.asarray(weight, np.float64), np.asarray(pixels, np.int64)
    tl = tol(ref.l_max)
    share = float(ref.uncertain.mean()) if ref.uncertain.size else 0.0
    assert share <= 0.02, f"{share:.3%} of the Gaussians have an uncertain pair (cap 2 %): the scene does not test what it should"
    assert np.all(pixels >= ref.pixels_lo) and np.all(pixels <= ref.pixels_hi), "pixels outside [certain, certain + uncertain]"
    dev_peak = np.maximum(ref.peak_lo - peak, peak - ref.peak_hi)
    assert dev_peak.max(initial=0.0) <= tl, f"peak off by {dev_peak.max():.3e} > {tl:.3e}"
    wt = weight_tol(ref.l_max, pixels)
    dev_w = np.maximum(ref.weight_lo - weight, weight - ref.weight_hi)
    assert np.all(dev_w <= wt), f"weight off by {(dev_w - wt).max():.3e} beyond the bound"
    seen = pixels > 0
    return float(dev_peak.max(initial=0.0)), float((dev_w[seen] / wt[seen]).max(initial=0.0))
