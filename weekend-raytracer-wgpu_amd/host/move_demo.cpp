// move_demo — Layer::move_spheres and Raytracer::move_spheres of the C++ mirror against objects made from the moved scene.
//   move_demo N W H      N spheres on a square lattice (a world beyond the LDS budget goes to device memory and is updated in place;
//                        a small one is set again), spheres [7, 7 + N / 4) moved; prints one line per object:
//                        "<object>: <equal|DIFFERENT> refits <mirt_ctx_bvh_refits after the move>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>

#include "mirt_host.hpp"

using namespace mirt_host;

static Scene lattice(uint32_t n)
{
    Scene s;
    s.materials.emplace_back(Lambertian{ Texture::new_from_color({ 0.5f, 0.5f, 0.5f }) });
    s.materials.emplace_back(Metal{ Texture::new_from_color({ 0.7f, 0.6f, 0.5f }), 0.2f });
    s.materials.emplace_back(Lambertian{ Texture::new_from_color({ 0.8f, 0.3f, 0.2f }) });    // parity mode reads material 2's texture on every hit
    s.materials.emplace_back(Dielectric{ 1.5f });
    const uint32_t side = (uint32_t)std::ceil(std::sqrt((double)n));
    s.spheres.push_back(sphere_new({ 0.0f, -1000.0f, 0.0f }, 1000.0f, 0));
    for (uint32_t i = 1; i < n; ++i) {
        const float x = 0.6f * ((float)(i % side) - 0.5f * (float)side), z = 0.6f * ((float)(i / side) - 0.5f * (float)side);
        s.spheres.push_back(sphere_new({ x, 0.2f, z }, 0.15f + 0.01f * (float)(i % 7), i % 4));
    }
    return s;
}

int main(int argc, char** argv)
{
    try {
        if (argc < 4) { std::fprintf(stderr, "usage: move_demo N W H\n"); return 2; }
        const uint32_t n = (uint32_t)std::atoi(argv[1]), w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        const uint32_t first = 7, count = n / 4;
        Scene a = lattice(n), b = a;
        std::vector<MirtSphere> moved;
        for (uint32_t i = 0; i < count; ++i) {
            MirtSphere s = a.spheres[first + i];
            s.center[0] += 0.1f; s.center[1] += 0.05f; s.radius *= 1.25f;
            s.material_idx = 99;                                           // not read: the spheres keep their materials
            moved.push_back(s);
            b.spheres[first + i].center[0] = s.center[0]; b.spheres[first + i].center[1] = s.center[1]; b.spheres[first + i].radius = s.radius;
        }
        RenderParams rp;
        rp.camera = default_fly_camera();
        rp.camera.eye_pos = { 0.0f, 3.0f, 9.0f };                          // above the lattice, looking down at its moved rows
        rp.camera.eye_dir = { 0.0f, -0.35f, -1.0f };
        rp.viewport_w = w; rp.viewport_h = h;
        rp.sampling.num_samples_per_pixel = 2; rp.sampling.max_samples_per_pixel = 4; rp.sampling.num_bounces = 4;
        rp.validate();
        int bad = 0;
        {
            Raytracer ra(a, rp), rb(b, rp);
            ra.render_frame();
            ra.move_spheres(first, moved);
            const bool reset = ra.progress() == 0.0f;
            bool equal = reset;
            for (int f = 0; f < 3; ++f) equal = (ra.render_frame() == rb.render_frame()) && equal;
            std::printf("raytracer: %s refits %u\n", equal ? "equal" : "DIFFERENT", mirt_ctx_bvh_refits(ra.context()));
            bad += !equal;
        }
        {
            const float size[2] = { (float)w, (float)h };
            Layer la(size, rp, a), lb(size, rp, b);
            la.set_global_data(); lb.set_global_data();
            la.move_spheres(first, moved);                                 // nothing resident yet: only `world` changes
            bool equal = la.context() == nullptr && la.world[first].radius == b.spheres[first].radius && la.world[first].material_idx == a.spheres[first].material_idx;
            la.world = a.spheres;
            la.set_data(rp);
            const std::vector<uint8_t> before = la.register_texture();
            la.move_spheres(first, moved, &rp);
            equal = (before != la.register_texture()) && equal;            // the move shows in the image
            lb.set_data(rp);
            equal = (la.register_texture() == lb.register_texture()) && equal;
            std::printf("layer: %s refits %u\n", equal ? "equal" : "DIFFERENT", mirt_ctx_bvh_refits(la.context()));
            bad += !equal;
            try { la.move_spheres(n - 1, moved); std::printf("layer: no error?!\n"); ++bad; }
            catch (const MirtError& e) { std::printf("layer range: %s world %s\n", mirt_status_string(e.status), la.world[n - 1].radius == b.spheres[n - 1].radius ? "kept" : "CHANGED"); }
        }
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
