#!/usr/bin/env python3
"""Generates tests/golden/*.npz with the float64 spec oracle (oracle/spec_f64.py).

PARITY UNPINNED: the reference holds no golden vectors for this path and its implementation (the crate
wgpu-3dgs-viewer 0.2.0) is neither vendored nor buildable here, so these fixtures pin the WRITTEN SPEC
(spec/RENDER_SPEC.md), not the reference.  Inputs are stored next to the expected outputs so the
fixtures stay valid if the scene generator changes.  Run from the repo root:  python tests/golden/make_golden.py

Fixture keys (i = model index in load order):
  view, proj, size, n_models, paint_order        camera (column-major), viewport, far -> near model order
  g{i}, cov{i}, mt{i}                            gs::Gaussian records, float64-derived cov3d (as f32), model TRS (pos3 quat4 scale3)
  visible{i}, mean2d{i}, conic{i}, rgb{i}, depth{i}, opacity{i}    float64 projection
  frame                                          float32 [H, W, 4] premultiplied rgb + T
  kw_*                                           gaussian-transform arguments (size, sh_deg, display_mode, no_sh0)
  pod_kind = (sh_kind, cov_kind), sh_q{i}, cov_q{i}   compressed pod: the exact dequantisation of what is stored
  mask_expr, mask_shapes [k, 11] = kind pos3 quat4 scale3, mask_words{i}, mask_margin{i}
  selection_words{i}, sel_edit = flag color3 contrast exposure gamma alpha, highlight = r g b a
  params_<name>                                  gsx_spec_params that differ from the defaults (spec/RENDER_SPEC.md [BUILD-SPEC] constants)
  frame_ambiguity, ambiguity_tol                 (large fixtures) per pixel: how much of the value hangs on support decisions q <= k^2 closer
                                                 than ambiguity_tol to the cut — a discontinuity of the spec (oracle/spec_f64.render)
  depth, depth_tol                               (depth fixtures) the caller's Depth32Float buffer f32 [H, W] (NDC depth, row 0 at the top) and
                                                 the test `Less`; the frame is spec_f64.render's NDC-domain test, frame_ambiguity carries
                                                 the pairs within depth_tol of the surface (and ambiguity_tol of the cut, if given)
  prior_view, prior_proj                         (large fixtures) another camera: a frame rendered from it first leaves windows that are
                                                 wrong for this one, so the speculated frame needs its repair round
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import spec_f64  # noqa: E402
from tests.common import surface_depth  # noqa: E402
from wgpu_3dgs_viewer_app_amd import camera, scene  # noqa: E402
from wgpu_3dgs_viewer_app_amd.mask import MaskOp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def pod_f64(g):
    """Pod planes from gs::Gaussian records; cov3d in float64 from rot/scale, rounded to float32 like the upload."""
    cov = spec_f64.cov3d_from_gaussians(g["rot"].astype(np.float64), g["scale"].astype(np.float64)).astype(np.float32)
    color = (g["color"][:, 0].astype(np.uint32) | (g["color"][:, 1].astype(np.uint32) << 8)
             | (g["color"][:, 2].astype(np.uint32) << 16) | (g["color"][:, 3].astype(np.uint32) << 24))
    return g["pos"].copy(), color, g["sh"].reshape(-1, 45).copy(), cov


def make(name, models, cam, w, h, pod=None, mask=None, selection=None, sel_edit=None, highlight=None, params=None, prior_cam=None,
         ambiguity_tol=None, depth=None, **kw):
    """pod = (sh_kind, cov_kind); mask = (expression, [dict(kind, pos, quat, scale)]) applied to every model;
    selection = seed of a random selection bitset (every model); sel_edit = dict(flag, color, contrast, exposure, gamma, alpha);
    highlight = (r, g, b, a); depth = the caller's Depth32Float buffer (f32 [h, w]) with the test `Less`; kw: size, display_mode,
    sh_deg, no_sh0."""
    view, proj = cam.view(), cam.projection(w / h)
    out = dict(view=view, proj=proj, size=np.array([w, h]), n_models=np.array(len(models)))
    if pod:
        out["pod_kind"] = np.array(pod)
    if mask:
        out["mask_expr"] = np.array(mask[0])
        out["mask_shapes"] = np.array([[s["kind"], *s["pos"], *s["quat"], *s["scale"]] for s in mask[1]], np.float32)
    if sel_edit:
        out["sel_edit"] = np.array([sel_edit["flag"], *sel_edit["color"], sel_edit["contrast"], sel_edit["exposure"],
                                    sel_edit["gamma"], sel_edit["alpha"]], np.float32)
    if highlight:
        out["highlight"] = np.array(highlight, np.float32)
    if params:
        kw = dict(kw, params=params)
        for k, v in params.items():
            out[f"params_{k}"] = np.array(v, np.float32)
    if prior_cam is not None:
        out["prior_view"], out["prior_proj"] = prior_cam.view(), prior_cam.projection(w / h)
    spec_models = []
    for i, (g, mt) in enumerate(models):
        pos, color, sh, cov = pod_f64(g)
        out[f"g{i}"] = g
        out[f"cov{i}"] = cov
        out[f"mt{i}"] = np.concatenate([mt.pos, mt.quat(), mt.scale]).astype(np.float32)
        if pod:
            # the upload computes cov3d in float32 and quantises THAT; the float64-derived cov agrees to ~1e-7 relative, far
            # inside a binary16 rounding interval for all but a vanishing fraction of values — the fixture keeps what the
            # float64 statement says and the tests compare the quantised planes with a one-ulp16 tolerance on cov, exactly on sh
            sh, cov = spec_f64.quantise_pod(sh, cov, *pod)
            out[f"sh_q{i}"], out[f"cov_q{i}"] = sh, cov
        mdl = dict(pos=pos, color=color, sh=None if (pod and pod[0] == 3) else sh, cov3d=cov, m_pos=mt.pos, m_quat=mt.quat(), m_scale=mt.scale)
        if mask:
            kept, margin = spec_f64.mask_evaluate(pos, MaskOp.parse(mask[0]).tree, mask[1], mt.pos, mt.quat(), mt.scale)
            assert margin.min() > 1e-4, f"{name}: a Gaussian sits within {margin.min():.2e} of a mask shape boundary; pick another seed"
            assert 0 < kept.sum() < kept.size
            mdl["mask"] = spec_f64.mask_words(kept)
            out[f"mask_words{i}"] = mdl["mask"]
            out[f"mask_margin{i}"] = np.array(margin.min())
        if selection is not None:
            bits = np.random.default_rng(selection + i).random(pos.shape[0]) < 0.4
            mdl["selection"], mdl["sel_edit"], mdl["highlight"] = bits, sel_edit, highlight
            out[f"selection_words{i}"] = _sel_words(bits)
        spec_models.append(mdl)
        pr = spec_f64.project(view, proj, w, h, pos, color, mdl["sh"], cov, mt.pos, mt.quat(), mt.scale, mask=mdl.get("mask"),
                              selection=mdl.get("selection"), sel_edit=mdl.get("sel_edit"), highlight=mdl.get("highlight"), **kw)
        out[f"visible{i}"] = pr["visible"]
        out[f"mean2d{i}"] = pr["mean2d"]
        out[f"conic{i}"] = pr["conic"]
        out[f"rgb{i}"] = pr["rgb"]
        out[f"depth{i}"] = pr["depth"]
        out[f"opacity{i}"] = pr["opacity"]
    # paint order far -> near by centre distance (scene.rs:533-558)
    keys = camera.model_render_order(cam.pos, {i: mt.world_center() for i, (_, mt) in enumerate(models)})
    out["paint_order"] = np.array(keys)
    if depth is not None:
        depth = np.ascontiguousarray(depth, np.float32)
        assert depth.shape == (h, w)
        out["depth"], out["depth_tol"] = depth, np.array(spec_f64.DEPTH_TOL)
    if ambiguity_tol is not None or depth is not None:
        frame, amb = spec_f64.render(view, proj, w, h, [spec_models[k] for k in keys], ambiguity_tol=ambiguity_tol, depth=depth, **kw)
        out["frame_ambiguity"] = amb.astype(np.float32)
        if ambiguity_tol is not None:
            out["ambiguity_tol"] = np.array(ambiguity_tol)
        print(name, "pixels whose value hangs on a support decision within", ambiguity_tol, "of the cut or a depth decision within",
              spec_f64.DEPTH_TOL if depth is not None else None, "of the surface by more than 1e-4:", int((amb > 1e-4).sum()), "of",
              amb.size, "max allowance", float(amb.max()))
        assert (amb > 1e-4).mean() < 0.02, f"{name}: too much of the frame hangs on near-cut decisions; pick another scene"
    else:
        frame = spec_f64.render(view, proj, w, h, [spec_models[k] for k in keys], **kw)
    out["frame"] = frame.astype(np.float32)
    for k, v in kw.items():
        if k != "params":
            out[f"kw_{k}"] = np.array(v)
    if params and params.get("alpha_min", 0.0) > 0.0:
        # alpha_min > 0 makes a visibility decision depend on exp(): a float32 implementation may decide a contribution that sits
        # within its rounding of the threshold the other way (up to alpha_min x colour on that pixel).  The fixture is only kept
        # if no contribution that matters comes that close.
        margin = spec_f64.alpha_min_margin(view, proj, w, h, [spec_models[k] for k in keys], **kw)
        assert margin > 3e-5, f"{name}: a contribution lies within {margin:.1e} (relative) of alpha_min; pick another seed"
        out["alpha_min_margin"] = np.array(margin)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, {k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items() if k in ("frame", "g0")},
          "mean T", float(frame[..., 3].mean()), "visible", [int(out[f"visible{i}"].sum()) for i in range(len(models))])


def _sel_words(bits):
    """selection bitset: bit i of word i >> 5; tail bits clear."""
    n = bits.shape[0]
    w = np.zeros((n + 31) // 32, np.uint32)
    idx = np.nonzero(bits)[0]
    np.bitwise_or.at(w, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return w


def scene_small(n, seed, sh_degree=3, mul=6.0):
    g = scene.synthetic_gaussians(n, seed, sh_degree)
    g["scale"] *= np.float32(mul)
    return g


if __name__ == "__main__":
    ident = camera.ModelTransform()
    odd = camera.ModelTransform(pos=np.array([0.3, -0.2, 0.5], np.float32), rot=np.array([20, -35, 50], np.float32),
                                scale=np.array([1.2, 0.9, 1.1], np.float32))
    only = sys.argv[1:]

    def want(name):
        return not only or any(o in name for o in only)

    if want("sh3_identity"):
        make("frame_sh3_identity_96x64_n600_seed101", [(scene_small(600, 101), ident)], camera.orbit_pose(17), 96, 64)
    if want("2models"):
        make("frame_sh3_trs_2models_112x80_n500_seed102",
             [(scene_small(500, 102), odd), (scene_small(400, 103), camera.ModelTransform(pos=np.array([0, 0, 1.5], np.float32)))],
             camera.orbit_pose(200), 112, 80)
    if want("sh0_nosh"):
        make("frame_sh0_nosh_size_80x48_n400_seed104", [(scene_small(400, 104, 0), ident)], camera.orbit_pose(90), 80, 48,
             size=1.5, sh_deg=0)
    # round 2: one fixture per feature either side of the plain path
    if want("norm8_half"):
        g = scene_small(600, 105)
        g["sh"] *= np.float32(4.0)  # push a good part of the coefficients past the snorm8 range
        make("frame_pod_norm8_half_96x64_n600_seed105", [(g, odd)], camera.orbit_pose(33), 96, 64, pod=(2, 1))  # the app's default pod
    if want("half_single"):
        make("frame_pod_half_single_80x48_n400_seed106", [(scene_small(400, 106), ident)], camera.orbit_pose(140), 80, 48, pod=(1, 0))
    if want("mask"):
        shapes = [dict(kind=0, pos=(0.3, 0.0, 0.2), quat=tuple(camera.quat_from_euler_zyx(0.4, -0.3, 0.2)), scale=(2.5, 2.0, 3.0)),
                  dict(kind=1, pos=(0.0, 0.3, 0.0), quat=(0.0, 0.0, 0.0, 1.0), scale=(1.5, 1.2, 1.8))]
        make("frame_mask_box_minus_ellipsoid_96x64_n700_seed107", [(scene_small(700, 107), odd)], camera.orbit_pose(120), 96, 64,
             mask=("0 - 1", shapes))
    if want("hsv_edit"):
        make("frame_hsv_edit_highlight_96x64_n600_seed108", [(scene_small(600, 108), ident)], camera.orbit_pose(60), 96, 64,
             selection=7, sel_edit=dict(flag=1, color=(0.37, 1.4, 0.7), contrast=0.3, exposure=-0.75, gamma=1.8, alpha=0.6),
             highlight=(1.0, 0.5, 0.0, 0.25))
    if want("hidden_edit"):
        make("frame_hidden_edit_80x48_n400_seed109", [(scene_small(400, 109), ident)], camera.orbit_pose(75), 80, 48,
             selection=9, sel_edit=dict(flag=3, color=(0.0, 1.0, 1.0), contrast=0.0, exposure=0.0, gamma=1.0, alpha=1.0))
    if want("ellipse"):
        make("frame_ellipse_mode_80x48_n400_seed110", [(scene_small(400, 110), ident)], camera.orbit_pose(150), 80, 48, display_mode=1)
    if want("point"):
        make("frame_point_mode_size15_80x48_n500_seed111", [(scene_small(500, 111), odd)], camera.orbit_pose(210), 80, 48,
             display_mode=2, size=1.5)
    # more of round 2: the SH degrees in between, no_sh0, a union mask on a Half/Half pod, three layered models
    if want("sh1"):
        make("frame_sh1_80x48_n400_seed112", [(scene_small(400, 112), odd)], camera.orbit_pose(5), 80, 48, sh_deg=1)
    if want("sh2_nosh0"):
        make("frame_sh2_nosh0_80x48_n400_seed113", [(scene_small(400, 113), ident)], camera.orbit_pose(100), 80, 48, sh_deg=2, no_sh0=1)
    if want("half_half_union"):
        shapes = [dict(kind=1, pos=(0.8, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0), scale=(1.2, 2.0, 1.2)),
                  dict(kind=0, pos=(-0.8, 0.2, 0.1), quat=tuple(camera.quat_from_euler_zyx(0.1, 0.7, -0.2)), scale=(1.0, 1.5, 2.0))]
        make("frame_pod_half_half_mask_union_96x64_n600_seed114", [(scene_small(600, 114), ident)], camera.orbit_pose(45), 96, 64,
             pod=(1, 1), mask=("0 | 1", shapes))
    # round 3: a fixture the DEFAULT pipeline meets at full strength — 320 x 240 = 300 tiles (> 256: blocks of several tiles),
    # two layered models, opaque enough that most tiles saturate (speculation, depth slabs, and — rendered after a frame from
    # `prior_cam` — a repair round); and one on INRIA-convention constants (alpha_max 0.99, alpha_min 1/255, k = 3), the values
    # SURVEY 8c expects the real crate to use, so that a later reconciliation has a float64 anchor
    if want("large"):
        make("frame_large_2models_320x240_seed201",
             [(scene_small(5500, 201, 3, 8.0), odd), (scene_small(4500, 202, 3, 8.0), camera.ModelTransform(pos=np.array([0.4, 0.1, 1.2], np.float32)))],
             camera.orbit_pose(40), 320, 240, prior_cam=camera.orbit_pose(100), ambiguity_tol=1e-3)
    if want("inria_params"):
        make("frame_inria_params_96x64_n600_seed204", [(scene_small(600, 204), odd)], camera.orbit_pose(25), 96, 64,
             params=dict(alpha_max=0.99, alpha_min=1.0 / 255.0, max_std_dev=3.0))
    if want("3models"):
        make("frame_sh3_3models_layered_112x80_seed115",
             [(scene_small(350, 115), odd), (scene_small(300, 116), camera.ModelTransform(pos=np.array([0.0, 0.4, -1.2], np.float32))),
              (scene_small(300, 117), camera.ModelTransform(pos=np.array([1.0, 0.0, 1.0], np.float32), scale=np.array([0.8, 0.8, 0.8], np.float32)))],
             camera.orbit_pose(180), 112, 80, pod=(2, 1))

    # the depth test (spec §6 "Depth test") against per-pixel depth buffers drawn from geometry seen by the fixture's own camera
    if want("depth_plane_odd"):
        cam = camera.orbit_pose(30)
        # 83 x 51: partial last tile column and row, and a last pixel-pair row half outside the image; the slanted plane
        # through the model changes the limit inside every tile and every pixel pair
        plane = [dict(kind="plane", point=(0.1, 0.0, -0.2), normal=(0.8, 0.35, 0.5))]
        make("frame_depth_plane_odd_83x51_n500_seed301", [(scene_small(500, 301), ident)], cam, 83, 51,
             depth=surface_depth(cam, 83, 51, plane))
    if want("depth_gizmo"):
        # the app's default pod (Norm8 + Half) and the case the gizmos exist for: box + ellipsoid drawn into the buffer, a mask,
        # a stored selection with a colour edit and a highlight
        cam = camera.orbit_pose(70)
        g = scene_small(600, 302)
        g["sh"] *= np.float32(4.0)
        gizmo = [dict(kind="box", pos=(0.5, 0.1, 0.4), quat=tuple(camera.quat_from_euler_zyx(0.3, 0.5, -0.2)), scale=(1.2, 0.9, 1.0)),
                 dict(kind="ellipsoid", pos=(-0.7, -0.2, 0.1), quat=tuple(camera.quat_from_euler_zyx(-0.4, 0.2, 0.1)), scale=(1.0, 1.3, 0.9))]
        shapes = [dict(kind=0, pos=(0.0, 0.0, 0.0), quat=tuple(camera.quat_from_euler_zyx(0.2, -0.1, 0.3)), scale=(2.6, 2.2, 2.8))]
        make("frame_depth_gizmo_norm8_half_edit_96x64_n600_seed302", [(g, odd)], cam, 96, 64, pod=(2, 1), mask=("0", shapes),
             selection=13, sel_edit=dict(flag=1, color=(0.2, 1.2, 0.9), contrast=0.2, exposure=0.5, gamma=1.2, alpha=0.8),
             highlight=(0.0, 1.0, 0.5, 0.3), depth=surface_depth(cam, 96, 64, gizmo))
    if want("depth_2models"):
        # two layered models with TRS and an occluder between them: pixels closed by depth in the near model go on to the far one
        cam = camera.orbit_pose(200)
        near_mt = camera.ModelTransform(pos=np.array([0.2, 0.0, 1.6], np.float32), rot=np.array([10, 25, -15], np.float32),
                                        scale=np.array([0.8, 0.9, 0.8], np.float32))
        models = [(scene_small(500, 303), odd), (scene_small(400, 304), near_mt)]
        mid = 0.5 * (odd.world_center().astype(np.float64) + near_mt.world_center().astype(np.float64))
        occ = [dict(kind="box", pos=tuple(mid + np.array([0.6, 0.3, 0.0])), quat=tuple(camera.quat_from_euler_zyx(0.2, 0.6, 0.1)),
                    scale=(2.0, 1.4, 0.15))]
        make("frame_depth_2models_trs_occluder_112x80_seed303", models, cam, 112, 80, depth=surface_depth(cam, 112, 80, occ))
    if want("depth_specials"):
        # a strip of special values inside the splat-covered middle of the frame, over a slanted plane
        cam = camera.orbit_pose(110)
        d = surface_depth(cam, 80, 48, [dict(kind="plane", point=(0.0, 0.0, 0.0), normal=(-0.3, 1.0, 0.6))])
        specials = [np.nan, 0.0, -0.0, -0.25, 1e-40, np.nextafter(np.float32(1), np.float32(0)), 1.0, 1.5, np.inf]
        for j, v in enumerate(specials):
            d[16:33, 13 + 6 * j: 19 + 6 * j] = np.float32(v)
        make("frame_depth_specials_80x48_n500_seed305", [(scene_small(500, 305), ident)], cam, 80, 48, depth=d)
    if want("depth_ellipse"):
        cam = camera.orbit_pose(160)
        shapes = [dict(kind="ellipsoid", pos=(0.3, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0), scale=(0.9, 1.4, 0.7)),
                  dict(kind="plane", point=(0.0, -0.3, 0.0), normal=(0.2, 1.0, -0.4))]
        make("frame_depth_ellipse_mode_80x48_n400_seed306", [(scene_small(400, 306), odd)], cam, 80, 48, display_mode=1,
             depth=surface_depth(cam, 80, 48, shapes))
