"""The reference of gsx_render_depth_map (spec/RENDER_SPEC.md §25) in plain numpy: the walk alone.  Its input is what calls from before
section 25 return — a projection (``mean2d``, ``conic_opacity``, the depth ``key``) and complete per-tile lists, the device's own
(``gsx_model_download_projection``, ``gsx_model_download_tile_lists`` after a ``progressive = 0`` frame) or the oracle's
(``oracle.project``, ``oracle.tile_lists``) — so a comparison isolates the new kernel.  One ``walk`` is one model; a model behind
continues from the ``Ref`` of the model in front (``state``), as the device continues from its planes.

Per pixel, front to back (spec §6): ``q`` in float32 with the spec's operation order, ``fmaf`` emulated through float64 (as
tests/visibility_ref.py does), so the support decisions are the device's exactly; ``exp``, alpha, ``w = T * alpha``, ``T *= 1 - alpha``,
``A += w`` and ``S += w * d`` in float64.  ``d`` is the float32 whose bits are the record's depth key.

Two decisions are made on T, which the device holds in float32: the pixel closes at ``T < t_epsilon``, and it crosses at the first
record after whose blend ``T < threshold``.  §24 bounds ``|T_dev - T|`` by ``s * 2^-21`` after ``s`` blends of the pixel; like the issue
the reference takes ``tol(s) = (s + 2) * 2^-21`` and calls a decision CERTAIN when T is further than that from its constant.

* A record with alpha = 0 exactly (opacity 0) decides nothing: the device's alpha is 0 exactly as well, and T stays bit for bit.
* Crossing: a blend with ``|T - threshold| <= tol`` is an uncertain crossing: the record is a CANDIDATE, and so is every later
  blended record up to and including the first with ``T < threshold - tol``.  A pixel with more than one candidate is ``uncertain``.
  ``surface`` / ``index`` / ``layer`` are the reference's own (float64) crossing.
* Closing: after an uncertain ``t_epsilon`` decision the device has either closed the pixel or not.  The reference snapshots
  ``(T, A, S)`` there (``*_lo`` for A and S, ``T_hi``) and keeps walking as if the pixel were open until it closes for certain
  (``*_hi``, ``T_lo``): ``w >= 0`` and ``d > 0``, so the device's values lie in between.  If the pixel has not crossed for certain by
  then, every later record is a candidate, "no crossing" (``maybe_none``) included, and the pixel is uncertain.

The bounds (§25): ``A`` telescopes, ``|A_dev - A| <= s * (2^-21 + 2^-22)``; for ``S`` the reference sums what the bound needs along
the pixel's own walk: the variation of d, the sum of d, the running S (``bound_A``, ``bound_S``)."""
import dataclasses

import numpy as np

from tests.visibility_ref import F, TILE, fmaf

NONE = 0xFFFFFFFF
U = 2.0 ** -21


def tol(s):
    """|T_dev - T| after s blends of the pixel (§24), with the issue's + 2"""
    return (np.asarray(s, np.float64) + 2.0) * U


@dataclasses.dataclass
class Ref:
    T: np.ndarray          # (h, w) float64: under the reference's own decisions
    A: np.ndarray
    S: np.ndarray
    T_lo: np.ndarray       # the ranges the device's values lie in before rounding (equal to T / A / S without an uncertain closing)
    T_hi: np.ndarray
    A_lo: np.ndarray
    A_hi: np.ndarray
    S_lo: np.ndarray
    S_hi: np.ndarray
    surface: np.ndarray    # (h, w) float32, inf without a crossing
    index: np.ndarray      # (h, w) uint32, NONE without
    layer: np.ndarray
    steps: np.ndarray      # (h, w) int64: s, the blends of the pixel (as if open)
    uncertain: np.ndarray  # (h, w) bool
    candidates: dict       # (y, x) -> list of (layer, index) for the uncertain pixels
    maybe_none: np.ndarray  # (h, w) bool: an uncertain closing lies in front of the crossing
    allow_none: np.ndarray  # (h, w) bool: "no crossing" is among the candidates (that, or an uncertain crossing and no certain one after it)
    bound_A: np.ndarray    # (h, w) float64
    bound_S: np.ndarray
    l_max: int
    # the walk's own bookkeeping, carried to the model behind
    _T_open: np.ndarray = None
    _A_open: np.ndarray = None
    _S_open: np.ndarray = None
    _open: np.ndarray = None
    _own_open: np.ndarray = None
    _zone: np.ndarray = None
    _crossed: np.ndarray = None      # crossed for certain
    _own_crossed: np.ndarray = None
    _pending: np.ndarray = None      # an uncertain crossing lies behind, no certain one yet
    _var_d: np.ndarray = None        # sum |d_k+1 - d_k| over the blends
    _last_d: np.ndarray = None
    _sum_d: np.ndarray = None
    _sum_S: np.ndarray = None


def _fresh(h, w):
    z = lambda v=0.0, t=np.float64: np.full((h, w), v, t)  # noqa: E731
    return Ref(T=z(1.0), A=z(), S=z(), T_lo=z(1.0), T_hi=z(1.0), A_lo=z(), A_hi=z(), S_lo=z(), S_hi=z(), surface=z(np.inf, F), index=z(NONE, np.uint32),
               layer=z(NONE, np.uint32), steps=z(0, np.int64), uncertain=z(False, bool), candidates={}, maybe_none=z(False, bool), allow_none=z(False, bool),
               bound_A=z(), bound_S=z(),
               l_max=0, _T_open=z(1.0), _A_open=z(), _S_open=z(), _open=z(True, bool), _own_open=z(True, bool), _zone=z(False, bool), _crossed=z(False, bool),
               _own_crossed=z(False, bool), _pending=z(False, bool), _var_d=z(), _last_d=z(np.nan), _sum_d=z(), _sum_S=z())


def walk(mean2d, conic_opacity, key, tile_offsets, tile_list, w, h, k2, alpha_max=1.0, alpha_min=0.0, t_eps=1e-4, display_mode=0, threshold=0.5,
         layer=0, state=None) -> Ref:
    mean2d = np.asarray(mean2d, F)
    co = np.asarray(conic_opacity, F)
    depth = np.ascontiguousarray(np.asarray(key, np.uint32)).view(F).astype(np.float64)
    off = np.asarray(tile_offsets, np.int64)
    lst = np.asarray(tile_list, np.int64)
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    assert off.shape[0] == tiles_x * tiles_y + 1
    r = _fresh(h, w) if state is None else dataclasses.replace(state, candidates={k: list(c) for k, c in state.candidates.items()})
    for name in [f.name for f in dataclasses.fields(Ref) if isinstance(getattr(r, f.name), np.ndarray)]:
        setattr(r, name, getattr(r, name).copy())
    r.l_max = max(r.l_max, int(np.diff(off).max()) if off.shape[0] > 1 else 0)
    k2, t_eps, alpha_max, alpha_min = F(k2), float(F(t_eps)), float(F(alpha_max)), float(F(alpha_min))
    thr = float(F(threshold))
    two_b = (F(2.0) * co[:, 1]).astype(F)
    for t in range(tiles_x * tiles_y):
        tx, ty = t % tiles_x, t // tiles_x
        ys, xs = np.mgrid[ty * TILE:min(ty * TILE + TILE, h), tx * TILE:min(tx * TILE + TILE, w)]
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        px = (ys, xs)
        pxf, pyf = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
        T, A, S = r._T_open[px], r._A_open[px], r._S_open[px]
        T_own, A_own, S_own = r.T[px], r.A[px], r.S[px]
        T_hi, A_lo, S_lo = r.T_hi[px], r.A_lo[px], r.S_lo[px]
        open_, own_open, zone = r._open[px], r._own_open[px], r._zone[px]
        crossed, own_crossed, pending, none_ok = r._crossed[px], r._own_crossed[px], r._pending[px], r.maybe_none[px]
        surface, index, lay, steps = r.surface[px], r.index[px], r.layer[px], r.steps[px]
        var_d, last_d, sum_d, sum_S = r._var_d[px], r._last_d[px], r._sum_d[px], r._sum_S[px]
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
            d = depth[g]
            # the reference's own walk
            b_own = blend & own_open
            w_own = np.where(b_own, T_own * alpha, 0.0)
            A_own = A_own + w_own
            S_own = S_own + w_own * d
            T_own = np.where(b_own, T_own * (1.0 - alpha), T_own)
            own_open &= T_own >= t_eps
            cross_own = b_own & ~own_crossed & (T_own < thr)
            surface = np.where(cross_own, F(d), surface)
            index = np.where(cross_own, np.uint32(g), index)
            lay = np.where(cross_own, np.uint32(layer), lay)
            own_crossed |= cross_own
            # as if open, with the decisions classified
            b = blend & open_
            wgt = np.where(b, T * alpha, 0.0)
            A = A + wgt
            S = S + wgt * d
            T = np.where(b, T * (1.0 - alpha), T)
            steps = steps + b
            var_d = var_d + np.where(b & ~np.isnan(last_d), np.abs(d - np.nan_to_num(last_d)), 0.0)
            last_d = np.where(b, d, last_d)
            sum_d = sum_d + np.where(b, d, 0.0)
            sum_S = sum_S + np.where(b, S, 0.0)
            tl = tol(steps)
            decides = b & (alpha > 0.0)
            # crossing
            look = decides & ~crossed
            sure_x = look & (T < thr - tl)
            unsure_x = look & ~sure_x & (T <= thr + tl)
            listed = (sure_x & (pending | zone)) | unsure_x | (look & zone & ~sure_x)
            for i in np.nonzero(listed)[0]:
                r.candidates.setdefault((int(ys[i]), int(xs[i])), []).append((int(layer), int(g)))
            pending |= unsure_x
            crossed |= sure_x
            # closing
            dist = np.abs(T - t_eps)
            new_zone = decides & ~zone & (dist <= tl)
            T_hi = np.where(new_zone, T, T_hi)
            A_lo = np.where(new_zone, A, A_lo)
            S_lo = np.where(new_zone, S, S_lo)
            zone |= new_zone
            none_ok |= new_zone & ~crossed
            open_ &= ~(decides & (T < t_eps - tl))
        unz = ~zone
        r._T_open[px], r._A_open[px], r._S_open[px] = T, A, S
        r.T[px], r.A[px], r.S[px] = T_own, A_own, S_own
        r.T_lo[px], r.T_hi[px] = T, np.where(unz, T, T_hi)
        r.A_lo[px], r.A_hi[px] = np.where(unz, A, A_lo), A
        r.S_lo[px], r.S_hi[px] = np.where(unz, S, S_lo), S
        r._open[px], r._own_open[px], r._zone[px] = open_, own_open, zone
        r._crossed[px], r._own_crossed[px], r._pending[px], r.maybe_none[px] = crossed, own_crossed, pending, none_ok
        r.surface[px], r.index[px], r.layer[px], r.steps[px] = surface, index, lay, steps
        r._var_d[px], r._last_d[px], r._sum_d[px], r._sum_S[px] = var_d, last_d, sum_d, sum_S
    # a pixel is uncertain when the device may have stored another crossing than the reference's own
    r.allow_none = r.maybe_none | (r._pending & ~r._crossed)
    r.uncertain = r.allow_none.copy()
    for (y, x), c in r.candidates.items():
        if len(set(c)) > 1 or c[0] != (int(r.layer[y, x]), int(r.index[y, x])):
            r.uncertain[y, x] = True
    s = r.steps.astype(np.float64)
    # §25: A telescopes to 1 - T: the error of T (s * 2^-21), three roundings a blend between w and T - T' (3 * 2^-24), one of the sum
    r.bound_A = s * (2.0 ** -21 + 2.0 ** -22)
    # §25: Abel's summation of (eps_k-1 - eps_k) * d_k over the blends, |eps_k| <= s * 2^-21: the variation of d plus the last d; the
    # three roundings times d; one rounding of the running S per fma (S_dev <= S * (1 + 2^-10) is far inside what the first terms allow)
    last = np.nan_to_num(r._last_d)
    r.bound_S = s * U * (r._var_d + last) + 3.0 * 2.0 ** -24 * r._sum_d + 2.0 ** -24 * (1.0 + 2.0 ** -10) * r._sum_S
    return r


def check(ref: Ref, surface, sum_, alpha, transmittance, index, layer, cap=0.02, floor=0.25):
    """§25's assertions for one call's planes against the reference of the same lists.  Returns the figures a test prints:
    (share of uncertain pixels, share of crossed pixels, largest |A_dev - A| / bound, largest |S_dev - S| / bound, largest |T_dev - T|
    / tol)."""
    surface, index, layer = np.asarray(surface, F), np.asarray(index, np.uint32), np.asarray(layer, np.uint32)
    A, S, T = np.asarray(alpha, np.float64), np.asarray(sum_, np.float64), np.asarray(transmittance, np.float64)
    unc = float(ref.uncertain.mean())
    crossed = float((ref.index != NONE).mean())
    assert unc <= cap, f"{unc:.2%} of the pixels have an uncertain crossing (cap {cap:.0%}): the scene does not test what it should"
    assert crossed >= floor, f"only {crossed:.2%} of the pixels cross (at least {floor:.0%})"
    sure = ~ref.uncertain
    assert np.array_equal(index[sure], ref.index[sure]), "the surface Gaussian at a certain pixel"
    assert np.array_equal(layer[sure], ref.layer[sure]), "the surface layer at a certain pixel"
    assert np.array_equal(surface[sure].view(np.uint32), ref.surface[sure].view(np.uint32)), "the surface depth at a certain pixel"
    for y, x in zip(*np.nonzero(ref.uncertain)):
        c = ref.candidates.get((int(y), int(x)), [])
        got = (int(layer[y, x]), int(index[y, x]))
        assert got in c or (ref.allow_none[y, x] and got == (NONE, NONE)), f"pixel ({x}, {y}): {got} is none of the candidates {c}"
    # index, layer and surface go together everywhere
    none = index == NONE
    assert np.array_equal(none, layer == NONE) and np.array_equal(none, np.isinf(surface)) and not np.isnan(surface).any()
    tl = tol(ref.steps)
    dev_T = np.maximum(ref.T_lo - T, T - ref.T_hi)
    dev_A = np.maximum(ref.A_lo - A, A - ref.A_hi)
    dev_S = np.maximum(ref.S_lo - S, S - ref.S_hi)
    assert np.all(dev_T <= tl), f"T off by {(dev_T - tl).max():.3e} beyond its bound"
    assert np.all(dev_A <= ref.bound_A), f"A off by {(dev_A - ref.bound_A).max():.3e} beyond its bound"
    assert np.all(dev_S <= ref.bound_S), f"S off by {(dev_S - ref.bound_S).max():.3e} beyond its bound"
    on = ref.steps > 0
    share = lambda dev, bound: float((dev[on] / bound[on]).max(initial=0.0))  # noqa: E731
    return unc, crossed, share(dev_A, ref.bound_A), share(dev_S, ref.bound_S), share(dev_T, tl)
