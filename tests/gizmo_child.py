"""Run by tests/test_gpu_gizmos.py in a child process (GSX_OVERLAY_BATCH_BOXES is read when a viewer is created): draws the named
scenes and prints, per scene, a digest of the overlay's colour, of the effective depth, of the `Less` framebuffer and the frame's
sort count — the limit keys are not exported; they are made from E in the raster launch, and the `Less` frame is composited through them.
    python -m tests.gizmo_child <width> <height> <scene> ...        (``random200`` is overlay_ref's, lines only)"""
import hashlib
import json
import sys

import numpy as np

from tests import gizmo_ref as G, overlay_ref as R
from tests import test_gpu_gizmos as T
from wgpu_3dgs_viewer_app_amd.viewer import DepthCompare


def main():
    size = (int(sys.argv[1]), int(sys.argv[2]))
    out = {}
    for name in sys.argv[3:]:
        if name == "random200":
            gizmos, lines, depth, cam = None, R.scenes(*size)[name][0], None, R.scene_camera()
        else:
            gizmos, lines, depth = G.scenes(*size)[name]
            cam = G.matrices(name, *size)[0]
        with T._viewer() as v:
            v.set_mask_gizmos(gizmos)
            v.update_hit_pairs(lines)
            v.set_depth_test(DepthCompare.Less)
            if depth is not None:
                v.update_depth_buffer(depth)
            fb = T._frame(v, cam, size)
            rgba, eff = v.download_overlay()
            out[name] = [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in (rgba, eff, fb)] + [
                int(v.frame_stats("m")["n_sorted"]), int((eff < 1.0).sum())]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
