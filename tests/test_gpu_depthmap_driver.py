"""GPU: the depth map calls through the C++ gs:: facade (include/gsx.hpp), played by tests/depthmap_driver.cpp — two models, the
planes, the device pointers, unproject, the front surface, two refusals — which checks itself what is exact (the transmittance
against the rendered frame, two calls, the statistics against the planes) and prints the figures compared here with the Python
facade's on the same LCG scene.  The two hosts restate the camera in float32 with different operation orders (as
tests/test_gpu_cpp_driver.py says), so the matrices differ by an ulp or two and the counts agree closely, not exactly."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_gpu_cpp_driver import lcg_scene
from wgpu_3dgs_viewer_app_amd import _lib, camera
from wgpu_3dgs_viewer_app_amd.viewer import GaussianDisplayMode, GaussianShDegree, MultiModelViewer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("depthmap") / "depthmap_driver")
    lib = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "depthmap_driver.cpp"), "-o", exe,
                           "-L" + lib, "-lgsx", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_facade_two_models_planes_pointers_unproject(driver):
    n, (w, h) = 3000, (96, 64)
    out = subprocess.run([driver, str(n)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    m = re.search(r"depthmap_driver n=(\d+) models=(\d+) covered=(\d+) crossed=(\d+) layer0=(\d+) layer1=(\d+) front=(\d+) ok", out.stdout)
    assert m, out.stdout
    cpp = [int(x) for x in m.groups()]
    g = lcg_scene(n, 12345)
    cam = camera.CameraOrbitControl(pos=np.array((2.0, 1.5, -6.0), np.float32))
    with MultiModelViewer() as v:
        for key, part in (("a", g[: n // 2]), ("b", g[n // 2:])):
            v.add_model(key, part.shape[0])
            v.models[key].gaussian_buffers.gaussians_buffer.update_range(0, part)
        v.update_gaussian_transform(1.0, GaussianDisplayMode.Splat, GaussianShDegree.new(3), False)
        v.update_camera(cam, (w, h))
        dm = v.render_depth_map(["a", "b"])
        front = v.render_depth_map(["a", "b"], threshold=1.0, planes=False)
    none = _lib.GSX_DEPTH_MAP_NONE
    assert cpp[0] == n and cpp[1] == dm.models == 2 and cpp[4] + cpp[5] == cpp[3] and cpp[6] >= cpp[3]
    want = (dm.n_covered, dm.n_crossed, int((dm.layer == 0).sum()), int((dm.layer == 1).sum()), front.n_crossed)
    assert int((dm.layer != none).sum()) == dm.n_crossed
    for got, ref in zip(cpp[2:], want):
        assert ref > 0 and abs(got - ref) <= 0.01 * ref + 2, (cpp, want)
