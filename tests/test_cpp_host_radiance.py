"""mirt_host::trace_radiance of the C++ mirror (host/probe_demo.cpp), run once on the device: the records it prints are the Python
wrappers' for the same scene, rays and params."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
import hbm_worlds

ROOT = Path(__file__).resolve().parent.parent
DEMO = ROOT / "weekend-raytracer-wgpu_amd" / "host" / "probe_demo"


@pytest.mark.gpu
def test_cpp_trace_radiance_matches_the_python_wrappers():
    subprocess.run(["make", "-C", str(DEMO.parent)], check=True, capture_output=True)
    r = subprocess.run([str(DEMO), "6"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = np.array([[int(v) for v in line.split()[2:]] for line in r.stdout.splitlines() if line.startswith("ray ")], np.uint64)
    assert rows.shape == (5, 4) and (rows[:, 3] == 6).all()
    assert re.search(r"^kernel: radiance_rays_kernel<false,true>$", r.stdout, re.M)
    # the same scene, rays and params through the Python wrappers
    arr = hbm_worlds.sphere_array([[0, -1000, 0], [-2.5, 1, 0], [0, 1, 0], [2.5, 1, 0]], [1000, 1, 1, 1], [0, 0, 0, 0])
    mat = _abi.MirtMaterial()
    mat.id = 0
    mat.desc1.width, mat.desc1.height, mat.desc1.offset = 1, 1, 0
    mat.desc2.width, mat.desc2.height, mat.desc2.offset = 0, 0, 0xffffffff
    ctx = m.Context(0)
    try:
        ctx.set_scene(hbm_worlds.scene_from_arrays(hbm_worlds.look(64, 64, (0, 2, 9), (0, 1.9, 8)), arr, [mat], np.array([[0.5, 0.5, 0.5]], np.float32)), hbm=True)
        rays = m.make_radiance_rays((0, 2, 9), [[-2.5, -1, -9], [0, -1, -9], [2.5, -1, -9], [0, -2, -4], [0, 1, 0]])
        rec = ctx.trace_radiance(rays, 6, num_bounces=8, seed=7)
    finally:
        ctx.close()
    assert np.array_equal(rows[:, :3], rec["sum"]) and rec["sum"][:4].any(1).all()
