"""The scenes of tests/grid_rounding.py are not vacuous, and its predictor restates the builder and the oracle (no GPU).

`decisive_rays` counts camera rays whose flat-scan winner is not listed, under the walk's own rounding slack, in any cell the exact
ray crosses: rays on which a grid that only absorbs the rounding of its walk differs from the flat scan.  The GPU matrix
(test_gpu_grid_rounding.py) is only as strong as these counts."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
import grid_rounding as gr


@pytest.mark.parametrize("name", list(gr.SCENES))
def test_binning_restates_the_builder(name):
    """The numpy binning gives mirt_grid_plan's cells, entries and always-tested count for every scene, at the plan's cell factor:
    the restatement cannot drift from build_grid.  Every scene is small enough for the flat kernels and, where a grid is built,
    leaves the pooled kernel's grid build room for its pools."""
    build, has_grid = gr.SCENES[name]
    sd, w, h = build()
    cen, rad = gr.spheres_of(sd)
    assert 32 <= len(rad) <= 2000 and w <= 96 and h <= 64
    plan = gr.grid_plan(sd)
    if not has_grid:
        assert plan.cell_factor == 0.0 and gr.binning(cen, rad) is None
        return
    assert plan.cell_factor > 0.0 and plan.pool_slots > 0
    g = gr.binning(cen, rad, plan.cell_factor)
    assert (plan.n_cells, plan.n_entries, plan.n_big) == (int(g["dims"].prod()), g["n_entries"], g["n_big"])
    # the enlargement covers the sphere test's rounding up to L_safe for the smallest binned radius
    r_min = np.abs(rad[g["small"]]).astype(np.float64).min()
    assert np.sqrt(r_min ** 2 + gr.K_DISC * g["l_safe"] ** 2) - r_min <= g["e_disc"] * (1 + 1e-9)
    assert g["e_disc"] <= 0.25 * g["cell"] * (1 + 1e-9)


def test_flat_grids_are_flat():
    """The xz grazing world and the field are one cell high: the FLATY builds run them."""
    for name in ("grazing xz", "telephoto 1000", "far origins"):
        sd, _, _ = gr.SCENES[name][0]()
        cen, rad = gr.spheres_of(sd)
        assert gr.binning(cen, rad, gr.grid_plan(sd).cell_factor)["dims"][1] == 1, name
    sd, _, _ = gr.SCENES["grazing xy"][0]()
    cen, rad = gr.spheres_of(sd)
    assert gr.binning(cen, rad, gr.grid_plan(sd).cell_factor)["dims"][2] == 1


@pytest.mark.parametrize("name", ["grazing xy", "grazing xz", "telephoto 1000", "telephoto 4000", "translated 16 far", "mixed radii"])
def test_scenes_have_decisive_rays(name):
    sd, w, h = gr.SCENES[name][0]()
    decisive, phantom, hits, rays = gr.decisive_rays(sd, w, h, 2, gr.grid_plan(sd).cell_factor)
    print(f"{name}: {decisive} decisive rays, {phantom} phantom winners, {hits} hits of {rays} rays")
    assert decisive >= 10, (decisive, phantom, hits, rays)


@pytest.mark.parametrize("name", ["telephoto 100 without ground", "soup"])
def test_controls_have_none(name):
    """Seen from next to the scene the phantom margin stays below the walk's slack: the regime of the existing grid tests.  (The
    ground is left out of the field: at its L the margin is not scale-clean.)"""
    sd, w, h = gr.telephoto(100.0, ground=False) if name.startswith("telephoto") else gr.soup()
    decisive, phantom, hits, rays = gr.decisive_rays(sd, w, h, 2, gr.grid_plan(sd).cell_factor)
    print(f"{name}: {decisive} decisive rays, {phantom} phantom winners, {hits} hits of {rays} rays")
    assert decisive == 0 and hits > 1000


def test_predictor_counts_the_oracles_camera_ray_hits(oracle):
    """One pinhole scene WITH phantom hits (the field from 1000 units), 1 spp, one bounce: the oracle's sample positions come from
    its own random stream (rng_stream), the rays and the sphere test from the predictor -- the hit counts are equal, so the
    restatement of test_sphere is tied to the oracle, not to the kernels."""
    sd, w, h = gr.telephoto(1000.0)
    p = m.make_params(w, h, 1, mode=m.MIRT_MODE_PT, num_bounces=1, flags=m.MIRT_FLAG_COUNT_WORK)
    oracle.render(sd, p)
    want = oracle.stats()
    X, Y = np.meshgrid(np.arange(w), np.arange(h))
    X, Y = X.ravel(), Y.ravel()
    r = np.stack([oracle.rng_stream(int(x + y * w), 0, 0, 2) for x, y in zip(X, Y)])
    u = ((X.astype(np.float32) + r[:, 0]) * (np.float32(1.0) / np.float32(w))).astype(np.float32)
    v = ((Y.astype(np.float32) + r[:, 1]) * (np.float32(1.0) / np.float32(h))).astype(np.float32)
    o, d = gr.camera_rays(sd.camera, w, h, u, v)
    cen, rad = gr.spheres_of(sd)
    best, _ = gr.flat_scan(o, d, cen, rad)
    assert want["rays"] == w * h
    assert int((best >= 0).sum()) == want["hits"]
    _, phantom, _, _ = gr.decisive_rays(sd, w, h, rays=(o, d))
    assert phantom >= 10, phantom                      # the agreement includes hits that only rounding produces
