// set_world_demo — Layer::set_world, Raytracer::set_world and mirt_host::set_spheres of the C++ mirror against objects made from the
// new scene.
//   set_world_demo N M W H   a lattice of N spheres replaced by one of M (another count, other materials); a world beyond the LDS
//                            budget is in device memory and gets the new sphere table in place, a small one is set again; prints one
//                            line per object: "<object>: <equal|DIFFERENT> built_on_device <0|1> spheres <count in the resident tree>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>

#include "mirt_host.hpp"

using namespace mirt_host;

static Scene lattice(uint32_t n, float pitch, uint32_t mat_step)
{
    Scene s;
    s.materials.emplace_back(Lambertian{ Texture::new_from_color({ 0.5f, 0.5f, 0.5f }) });
    s.materials.emplace_back(Metal{ Texture::new_from_color({ 0.7f, 0.6f, 0.5f }), 0.2f });
    s.materials.emplace_back(Lambertian{ Texture::new_from_color({ 0.8f, 0.3f, 0.2f }) });    // parity mode reads material 2's texture on every hit
    s.materials.emplace_back(Dielectric{ 1.5f });
    const uint32_t side = (uint32_t)std::ceil(std::sqrt((double)n));
    if (n) s.spheres.push_back(sphere_new({ 0.0f, -1000.0f, 0.0f }, 1000.0f, 0));
    for (uint32_t i = 1; i < n; ++i) {
        const float x = pitch * ((float)(i % side) - 0.5f * (float)side), z = pitch * ((float)(i / side) - 0.5f * (float)side);
        s.spheres.push_back(sphere_new({ x, 0.2f, z }, 0.15f + 0.01f * (float)(i % 7), (i * mat_step) % 4));
    }
    return s;
}

static void report(const char* what, bool equal, MirtContext* ctx, int* bad)
{
    MirtBvhInfo info{};
    const bool hbm = ctx && mirt_ctx_bvh_info(ctx, &info) == MIRT_OK;
    std::printf("%s: %s built_on_device %u spheres %u\n", what, equal ? "equal" : "DIFFERENT", hbm ? info.built_on_device : 0u,
                hbm ? info.plan.n_leaf_spheres + info.plan.n_always : 0u);
    *bad += !equal;
}

int main(int argc, char** argv)
{
    try {
        if (argc < 5) { std::fprintf(stderr, "usage: set_world_demo N M W H\n"); return 2; }
        const uint32_t n = (uint32_t)std::atoi(argv[1]), m = (uint32_t)std::atoi(argv[2]), w = (uint32_t)std::atoi(argv[3]), h = (uint32_t)std::atoi(argv[4]);
        const Scene a = lattice(n, 0.6f, 1), b = lattice(m, 0.7f, 3);
        Scene ab = a;                                                      // what `a` is after set_world(b.spheres)
        ab.spheres = b.spheres;
        RenderParams rp;
        rp.camera = default_fly_camera();
        rp.camera.eye_pos = { 0.0f, 3.0f, 9.0f };
        rp.camera.eye_dir = { 0.0f, -0.35f, -1.0f };
        rp.viewport_w = w; rp.viewport_h = h;
        rp.sampling.num_samples_per_pixel = 2; rp.sampling.max_samples_per_pixel = 4; rp.sampling.num_bounces = 4;
        rp.validate();
        int bad = 0;
        {
            Raytracer ra(a, rp), rb(ab, rp);
            ra.render_frame();
            ra.set_world(b.spheres);
            bool equal = ra.progress() == 0.0f;
            for (int f = 0; f < 3; ++f) equal = (ra.render_frame() == rb.render_frame()) && equal;
            report("raytracer", equal, ra.context(), &bad);
        }
        {
            const float size[2] = { (float)w, (float)h };
            Layer la(size, rp, a), lb(size, rp, ab);
            la.set_global_data(); lb.set_global_data();
            la.set_world(b.spheres);                                       // nothing resident yet: only `world` changes
            bool equal = la.context() == nullptr && la.world.size() == b.spheres.size();
            la.world = a.spheres;
            la.set_data(rp);
            const std::vector<uint8_t> before = la.register_texture();
            la.set_world(b.spheres, &rp);
            equal = (before != la.register_texture()) && equal;            // the new world shows in the image
            lb.set_data(rp);
            equal = (la.register_texture() == lb.register_texture()) && equal;
            report("layer", equal, la.context(), &bad);
            // the free function on the layer's context: back to the first world's spheres, against a layer that holds them
            MirtBvhInfo info{};
            if (mirt_ctx_bvh_info(la.context(), &info) == MIRT_OK) {
                set_spheres(la.context(), a.spheres);
                la.world = a.spheres;
                la.move_spheres(0, {}, &rp);                               // an empty range: renders what the context holds
                Layer lc(size, rp, a);
                lc.set_global_data();
                lc.set_data(rp);
                report("set_spheres", la.register_texture() == lc.register_texture() && la.register_texture() == before, la.context(), &bad);
            }
        }
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
