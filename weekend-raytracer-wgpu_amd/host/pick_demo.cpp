// pick_demo — mirt_host::trace_rays of the C++ mirror: picking and line of sight against a world in device memory.
//   pick_demo W H X Y   three spheres on a ground sphere, set with MIRT_SCENE_HBM; prints the sphere under pixel (X, Y) of a W x H
//                       viewport ("pick: sphere <i> t <t>" or "pick: none"), then whether the eye sees the point straight above
//                       the middle sphere ("sight: clear" / "sight: blocked"; an any-hit query bounded by the distance).
#include <cstdio>
#include <cstdlib>
#include <exception>

#include "mirt_host.hpp"

using namespace mirt_host;

int main(int argc, char** argv)
{
    try {
        if (argc < 5) { std::fprintf(stderr, "usage: pick_demo W H X Y\n"); return 2; }
        const uint32_t w = (uint32_t)std::atoi(argv[1]), h = (uint32_t)std::atoi(argv[2]), x = (uint32_t)std::atoi(argv[3]), y = (uint32_t)std::atoi(argv[4]);
        if (!w || !h || x >= w || y >= h) { std::fprintf(stderr, "pixel (%u, %u) lies outside the %u x %u viewport\n", x, y, w, h); return 2; }
        const MirtSphere spheres[4] = { { { 0.0f, -1000.0f, 0.0f, 0.0f }, 1000.0f, 0u, { 0u, 0u } },
                                        { { -2.5f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } },
                                        { { 0.0f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } },
                                        { { 2.5f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } } };
        MirtMaterial mat{};                                   // one lambertian of one grey texel; ray queries never read it
        mat.id = 0u;
        mat.desc1 = MirtTextureDescriptor{ 1u, 1u, 0u };
        mat.desc2 = MirtTextureDescriptor{ 0u, 0u, 0xffffffffu };
        const float texel[3] = { 0.5f, 0.5f, 0.5f };
        MirtCamera cam{ { 0.0f, 2.0f, 9.0f }, { 0.0f, -0.1f, -1.0f }, { 0.0f, 1.0f, 0.0f }, mirt_degrees_to_radians(40.0f), 0.0f, 9.0f };
        MirtGpuCamera gpu_cam{};
        check(mirt_camera_new(&cam, w, h, &gpu_cam));
        MirtScene sc{};
        sc.camera = &gpu_cam; sc.spheres = spheres; sc.n_spheres = 4u; sc.materials = &mat; sc.n_materials = 1u; sc.texels = texel; sc.n_texels = 1u;

        MirtContext* ctx = nullptr;
        check(mirt_ctx_create(0, &ctx));
        std::unique_ptr<MirtContext, void (*)(MirtContext*)> guard(ctx, mirt_ctx_destroy);
        set_scene(ctx, sc, MIRT_SCENE_HBM);                   // ray queries need the world in device memory

        const MirtRayHit hit = trace_rays(ctx, { pixel_ray(gpu_cam, w, h, x, y) })[0];
        if (hit.sphere == MIRT_RAY_MISS) std::printf("pick: none\n");
        else std::printf("pick: sphere %u t %.9g point %.9g %.9g %.9g\n", hit.sphere, hit.t, hit.point[0], hit.point[1], hit.point[2]);

        // line of sight from the eye to a point: direction = target - eye, so the target lies at t = 1; bound the query just before it
        const Vec3 eye{ cam.eye_pos[0], cam.eye_pos[1], cam.eye_pos[2] }, target{ 0.0f, 3.0f, 0.0f };
        const MirtRay los = make_ray(eye, { target.x - eye.x, target.y - eye.y, target.z - eye.z }, 1.0f);
        const bool blocked = trace_rays(ctx, { los }, MIRT_RAYS_ANY_HIT)[0].sphere != MIRT_RAY_MISS;
        std::printf("sight: %s\n", blocked ? "blocked" : "clear");
        std::printf("kernel: %s\n", mirt_ctx_last_kernel(ctx));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
