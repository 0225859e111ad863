"""mirt_host::reproject and mirt_host::camera_project of the C++ mirror (host/temporal_demo.cpp), run once on the device: the pixels
it prints for the last frame of its pan are the Python wrappers' for the same scene, cameras, frames and parameters, and those are the
reference's (tests/reproject_ref.py)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
import hbm_worlds
import reproject_ref as rr

ROOT = Path(__file__).resolve().parent.parent
DEMO = ROOT / "weekend-raytracer-wgpu_amd" / "host" / "temporal_demo"
W, H, FRAMES = 32, 24, 3
f32 = np.float32


def _camera(k):
    return m.GpuCamera.new(m.Camera(np.array([f32(0.2) * f32(k), 2, 9], f32), np.array([0, -0.1, -1], f32), np.array([0, 1, 0], f32),
                                    m.Angle.degrees(40.0), 0.0, 9.0), (W, H)).c


@pytest.mark.gpu
def test_cpp_reproject_matches_the_python_wrappers_and_the_reference():
    subprocess.run(["make", "-C", str(DEMO.parent)], check=True, capture_output=True)
    r = subprocess.run([str(DEMO), str(FRAMES)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = np.array([[int(v, 16) for v in line.split()[2:]] for line in r.stdout.splitlines() if line.startswith("px ")], np.uint32)
    assert rows.shape == (W * H, 5)
    coverage = [int(c) for c in re.findall(r"^frame \d+: history (\d+) of %d$" % (W * H), r.stdout, re.M)]
    assert len(coverage) == FRAMES and coverage[0] == 0 and all(c > W * H // 2 for c in coverage[1:]), coverage
    assert re.search(r"^kernel: reproject_kernel<true,true>$", r.stdout, re.M)
    # the same scene, cameras, frames and parameters through the Python wrappers
    arr = hbm_worlds.sphere_array([[0, -1000, 0], [-2.5, 1, 0], [0, 1, 0], [2.5, 1, 0]], [1000, 1, 1, 1], [0, 0, 0, 0])
    mat = _abi.MirtMaterial()
    mat.id = 0
    mat.desc1.width, mat.desc1.height, mat.desc1.offset = 1, 1, 0
    mat.desc2.width, mat.desc2.height, mat.desc2.offset = 0, 0, 0xffffffff
    ctx = m.Context(0)
    try:
        ctx.set_scene(hbm_worlds.scene_from_arrays(_camera(0), arr, [mat], np.array([[0.5, 0.5, 0.5]], f32)), hbm=True)
        history = want = prev = None
        for k in range(FRAMES):
            cam = _camera(k)
            ctx.set_camera(cam)
            p = m.make_params(W, H, 2, mode=m.MIRT_MODE_PT, seed=7 + k)
            ctx.accum_reset(p)
            ctx.accum_frame(p)
            guides = ctx.render_features(p)
            colour = ctx.denoise(p, m.make_denoise_params("accum", levels=3, sigma_colour=1.0, normal_log2=5, f32=True), guides)
            if k == 0:
                history, rgba = colour, ctx.denoise(p, m.make_denoise_params("accum"), guides)
            else:
                want = rr.reproject(colour, guides, history, prev[0], prev[1], cam, W, H, max_history=4.0, depth_tolerance=0.05, clamp=True)
                history, rgba = ctx.reproject(p, m.make_reproject_params(prev[1], cam), colour, guides, history, prev[0], rgba8=True)
            assert int((history[..., 3] > 1).sum()) == coverage[k]
            prev = (guides, cam)
        centre = m.camera_project(prev[1], W, H, (0.0, 1.0, 0.0))
    finally:
        ctx.close()
    assert rr.same_f32_or_nan(rows[:, :4].copy().view(f32).reshape(H, W, 4), history).all()
    assert np.array_equal(rows[:, 4], np.ascontiguousarray(rgba).view(np.uint32).reshape(-1))
    assert rr.same_f32_or_nan(history, want[0]).all() and np.array_equal(rgba, want[1])
    assert len(np.unique(rows[:, 4])) > 50                          # a picture, not a constant
    got = re.search(r"^sphere 2 at: (\w+) (\w+) (\w+)$", r.stdout, re.M)
    assert [int(v, 16) for v in got.groups()] == centre.view(np.uint32).tolist()
    assert 0 <= centre[0] < W and 0 <= centre[1] < H and centre[2] > 0
