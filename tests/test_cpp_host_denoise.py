"""mirt_host::denoise of the C++ mirror (host/denoise_demo.cpp), run once on the device: the pixels it prints are the Python wrappers'
for the same scene, frames, guides and parameters, and those are the reference's (tests/denoise_ref.py)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
import denoise_ref as dr
import hbm_worlds

ROOT = Path(__file__).resolve().parent.parent
DEMO = ROOT / "weekend-raytracer-wgpu_amd" / "host" / "denoise_demo"
W, H = 32, 24


@pytest.mark.gpu
def test_cpp_denoise_matches_the_python_wrappers_and_the_reference():
    subprocess.run(["make", "-C", str(DEMO.parent)], check=True, capture_output=True)
    r = subprocess.run([str(DEMO), "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = np.array([[int(v, 16) for v in line.split()[2:]] for line in r.stdout.splitlines() if line.startswith("px ")], np.uint32)
    assert rows.shape == (W * H, 4)
    assert re.search(r"^samples: 4$", r.stdout, re.M) and re.search(r"^kernel: denoise_atrous_staged_kernel<rgba8>$", r.stdout, re.M)
    # the same scene, frames, guides and parameters through the Python wrappers
    arr = hbm_worlds.sphere_array([[0, -1000, 0], [-2.5, 1, 0], [0, 1, 0], [2.5, 1, 0]], [1000, 1, 1, 1], [0, 0, 0, 0])
    mat = _abi.MirtMaterial()
    mat.id = 0
    mat.desc1.width, mat.desc1.height, mat.desc1.offset = 1, 1, 0
    mat.desc2.width, mat.desc2.height, mat.desc2.offset = 0, 0, 0xffffffff
    cam = m.GpuCamera.new(m.Camera(np.array([0, 2, 9], np.float32), np.array([0, -0.1, -1], np.float32), np.array([0, 1, 0], np.float32),
                                   m.Angle.degrees(40.0), 0.0, 9.0), (W, H)).c
    ctx = m.Context(0)
    try:
        ctx.set_scene(hbm_worlds.scene_from_arrays(cam, arr, [mat], np.array([[0.5, 0.5, 0.5]], np.float32)), hbm=True)
        p = m.make_params(W, H, 2, mode=m.MIRT_MODE_PT, seed=7)
        ctx.accum_reset(p)
        for _ in range(2):
            ctx.accum_frame(p)
        guides = ctx.render_features(p)
        lin = ctx.denoise(p, m.make_denoise_params("accum", levels=3, sigma_colour=1.0, normal_log2=5, f32=True), guides)
        rgba = ctx.denoise(p, m.make_denoise_params("accum", levels=3, sigma_colour=1.0, normal_log2=5), guides)
        want = dr.denoise(ctx.accum_read(p), ctx.accum_samples(), guides, 3, 1.0, 5)
    finally:
        ctx.close()
    assert np.array_equal(rows[:, :3], lin.view(np.uint32).reshape(-1, 4)[:, :3])
    assert np.array_equal(rows[:, 3], np.ascontiguousarray(rgba).view(np.uint32).reshape(-1))
    assert dr.same_f32(lin, want[0]) and np.array_equal(rgba, want[1])
    assert len(np.unique(rows[:, 3])) > 50                          # a picture, not a constant
