"""The pooled kernel's per-step bookkeeping (MI355X): the pick of the deepest queue (a scalar maximum over depth << 3 | 7 - k), the
tail update, the routine dispatch, the push.  All of it moves slot ids and depths, none of it arithmetic, so every case is
checked against the oracle's exact 64-bit sums -- at the smallest shapes where that bookkeeping can go wrong:
every count of scatter queues (the 1...5-queue builds), frames whose last strip is ragged and whose strips wrap rows, sample
counts around the 64 lanes of a step and the 112 slots of a pool, bounce limits that end paths at once.

The "missing" routine is reached through a material whose id the shader does not know; a sphere whose material INDEX is out
of range is refused by the library and the oracle alike before anything is launched (tests/test_gpu_api.py)."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from helpers import simple_camera

pytestmark = pytest.mark.gpu

POOL = m.MIRT_FLAG_KERNEL_POOL
FRAMES = ((48, 32), (37, 5))                  # 37 x 5: strips of 16 pixels wrap rows, the last one holds 9
SPPS = (33, 64, 130)
BOUNCES = (0, 1, 8)
# routine ids of scatterRay in the order the scenes below add them: metal, checkerboard, dielectric, lambertian, missing
ORDER = (1, 3, 2, 0, 4)


def _materials(routines):
    """One material per routine id, and an 8 x 4 image texture for the lambertian one (the texel-tile build needs an image)."""
    rng = np.random.default_rng(11)
    img = (rng.random((4, 8, 3)) * 255).astype(np.uint8)
    T = m.Texture
    make = {0: lambda: m.Material.Lambertian(T.new_from_rgb8(img)), 1: lambda: m.Material.Metal(T.new_from_color((0.8, 0.7, 0.6)), 0.3),
            2: lambda: m.Material.Dielectric(1.5), 3: lambda: m.Material.Checkerboard(even=T.new_from_color((0.9, 0.9, 0.9)), odd=T.new_from_color((0.2, 0.3, 0.1)))}
    gm, texels = m.flatten_materials([make[r]() for r in routines if r < 4])
    if 4 in routines:
        gm.append(m._abi.MirtMaterial(9, m.TextureDescriptor.empty(), m.TextureDescriptor.empty(), 0.0))
    return gm, texels


def _scene(routines, w, h):
    """A ground sphere and five small ones over it; sphere i carries material i mod the table (so materials are shared)."""
    gm, texels = _materials(routines)
    centres = [(0.0, -100.5, 0.0), (-1.6, 0.0, 0.0), (-0.5, 0.0, 0.6), (0.6, 0.0, -0.4), (1.7, 0.1, 0.3), (0.0, 1.1, -1.0)]
    radii = [100.0, 0.5, 0.5, 0.5, 0.5, 0.4]
    spheres = [m.Sphere.new(c, r, i % len(gm)).to_c() for i, (c, r) in enumerate(zip(centres, radii))]
    return m.SceneData(simple_camera(w, h, eye=(0.0, 0.6, 4.0), vfov=50.0, aperture=0.1, focus=4.0), spheres, gm, texels)


def _pt(w, h, spp, bounces=8, flags=POOL, **kw):
    return m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, num_bounces=bounces, flags=flags, **kw)


def _sums(ctx, p):
    ctx.accum_reset(p)
    ctx.accum_add(p)
    return ctx.accum_read(p)


def _check(ctx, oracle, sd, w, h, spp, bounces, what, flags=POOL, kernel="render_pt_pool_kernel<256,112,6,false,false,"):
    p = _pt(w, h, spp, bounces, flags)
    got = _sums(ctx, p)
    assert ctx.last_kernel().startswith(kernel), (what, ctx.last_kernel())
    want = oracle.render_pt_sums(sd, _pt(w, h, spp, bounces, 0))
    assert np.array_equal(got, want), f"{what}: {w}x{h}, spp {spp}, bounces {bounces}: {int((got != want).any(-1).sum())} of {w * h} pixels differ"


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5])
def test_every_queue_count_frame_sample_count_and_bounce_limit(gpu_ctx, oracle, nq):
    """nq distinct routines -> the build with nq scatter queues: its pick, its switch and its push."""
    for w, h in FRAMES:
        sd = _scene(ORDER[:nq], w, h)
        gpu_ctx.set_scene(sd)
        for spp in SPPS:
            for bounces in BOUNCES:
                _check(gpu_ctx, oracle, sd, w, h, spp, bounces, f"{nq} routines",
                       kernel=f"render_pt_pool_kernel<256,112,6,false,false,{nq},")


def test_all_slots_in_one_queue(gpu_ctx, oracle):
    """The eye sits inside one big metal sphere: every path hits until its bounce limit, so after the first steps all 112 slots
    wait in the ONE scatter queue -- keys and depths at their largest."""
    w, h = 48, 32
    gm, texels = _materials((1,))
    sd = m.SceneData(simple_camera(w, h, eye=(0.0, 0.0, 0.0), vfov=70.0), [m.Sphere.new((0.0, 0.0, 0.0), 50.0, 0).to_c()], gm, texels)
    gpu_ctx.set_scene(sd)
    for spp, bounces in ((130, 8), (64, 1), (33, 40)):
        _check(gpu_ctx, oracle, sd, w, h, spp, bounces, "enclosed eye", kernel="render_pt_pool_kernel<256,112,6,false,false,1,")


def test_only_sky(gpu_ctx, oracle):
    """Every sphere is behind the camera: every full step fast-forwards from OP_GEN to OP_GEN and pushes nothing."""
    for w, h in FRAMES:
        sd = _scene(ORDER[:3], w, h)
        sd = m.SceneData(simple_camera(w, h, eye=(0.0, 5.0, 8.0), direction=(0.0, 0.3, 1.0), vfov=40.0), sd.spheres, sd.materials, sd.texels)
        gpu_ctx.set_scene(sd)
        for spp in SPPS:
            _check(gpu_ctx, oracle, sd, w, h, spp, 8, "sky only")


def test_shared_material_and_unknown_material_id(gpu_ctx, oracle):
    """Two routines on six spheres (three spheres per material), and a table whose LAST material has an id the shader does not
    know: its spheres run the missing-material routine."""
    w, h = 48, 32
    for routines in ((0, 1), (3, 4), (4,)):
        sd = _scene(routines, w, h)
        assert len(sd.spheres) > len(sd.materials)
        gpu_ctx.set_scene(sd)
        _check(gpu_ctx, oracle, sd, w, h, 130, 8, f"routines {routines}")
        _check(gpu_ctx, oracle, sd, w, h, 33, 1, f"routines {routines}")


def test_tile_build_and_progressive_frame_share_the_text(gpu_ctx, oracle):
    """The texel-tile build and the progressive-frame build are the same kernel text compiled again."""
    w, h = 37, 5
    sd = _scene(ORDER[:4], w, h)                   # the lambertian material carries the image texture
    gpu_ctx.set_scene(sd)
    _check(gpu_ctx, oracle, sd, w, h, 130, 8, "tile build", flags=POOL | m.MIRT_FLAG_TEXEL_TILES, kernel="render_pt_pool_tile_kernel<")
    # two fused frames of 33 + 97 samples: sums and image of the 130
    gpu_ctx.accum_reset(_pt(w, h, 33))
    for spp in (33, 97):
        img = gpu_ctx.accum_frame(_pt(w, h, spp))
        assert gpu_ctx.last_kernel().startswith("render_pt_pool_frame_kernel<"), gpu_ctx.last_kernel()
    assert np.array_equal(gpu_ctx.accum_read(_pt(w, h, 97)), oracle.render_pt_sums(sd, _pt(w, h, 130, flags=0)))
    assert np.array_equal(img, oracle.render(sd, _pt(w, h, 130, flags=0)))
