// probe_demo — mirt_host::trace_radiance of the C++ mirror: the path tracer for rays the host chooses.
//   probe_demo SPP   three spheres on a ground sphere, set with MIRT_SCENE_HBM; five rays from (0, 2, 9) -- at the three spheres, at the
//                    ground and straight up -- each with its index as RNG stream; prints "ray <i>: <sum r> <sum g> <sum b> <samples>"
//                    (exact sums in units of 2^-20) after SPP samples, then the kernel's name.
#include <cstdio>
#include <cstdlib>
#include <exception>

#include "mirt_host.hpp"

using namespace mirt_host;

int main(int argc, char** argv)
{
    try {
        if (argc < 2 || std::atoi(argv[1]) < 1) { std::fprintf(stderr, "usage: probe_demo SPP\n"); return 2; }
        const uint32_t spp = (uint32_t)std::atoi(argv[1]);
        const MirtSphere spheres[4] = { { { 0.0f, -1000.0f, 0.0f, 0.0f }, 1000.0f, 0u, { 0u, 0u } },
                                        { { -2.5f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } },
                                        { { 0.0f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } },
                                        { { 2.5f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } } };
        MirtMaterial mat{};                                   // one lambertian of one grey texel
        mat.id = 0u;
        mat.desc1 = MirtTextureDescriptor{ 1u, 1u, 0u };
        mat.desc2 = MirtTextureDescriptor{ 0u, 0u, 0xffffffffu };
        const float texel[3] = { 0.5f, 0.5f, 0.5f };
        MirtCamera cam{ { 0.0f, 2.0f, 9.0f }, { 0.0f, -0.1f, -1.0f }, { 0.0f, 1.0f, 0.0f }, mirt_degrees_to_radians(40.0f), 0.0f, 9.0f };
        MirtGpuCamera gpu_cam{};
        check(mirt_camera_new(&cam, 64u, 64u, &gpu_cam));     // a scene carries a camera; a query does not use it
        MirtScene sc{};
        sc.camera = &gpu_cam; sc.spheres = spheres; sc.n_spheres = 4u; sc.materials = &mat; sc.n_materials = 1u; sc.texels = texel; sc.n_texels = 1u;

        MirtContext* ctx = nullptr;
        check(mirt_ctx_create(0, &ctx));
        std::unique_ptr<MirtContext, void (*)(MirtContext*)> guard(ctx, mirt_ctx_destroy);
        set_scene(ctx, sc, MIRT_SCENE_HBM);                   // radiance queries need the world in device memory

        const float dirs[5][3] = { { -2.5f, -1.0f, -9.0f }, { 0.0f, -1.0f, -9.0f }, { 2.5f, -1.0f, -9.0f }, { 0.0f, -2.0f, -4.0f }, { 0.0f, 1.0f, 0.0f } };
        std::vector<MirtRadianceRay> rays;
        for (uint32_t i = 0; i < 5u; ++i) rays.push_back(MirtRadianceRay{ { 0.0f, 2.0f, 9.0f }, i, { dirs[i][0], dirs[i][1], dirs[i][2] }, 0u });
        MirtRadianceParams p{};
        p.spp = spp; p.num_bounces = 8u; p.seed = 7u;
        const std::vector<MirtRadiance> whole = trace_radiance(ctx, rays, p);
        for (size_t i = 0; i < whole.size(); ++i)
            std::printf("ray %zu: %llu %llu %llu %u\n", i, (unsigned long long)whole[i].sum[0], (unsigned long long)whole[i].sum[1],
                        (unsigned long long)whole[i].sum[2], whole[i].samples);
        std::printf("kernel: %s\n", mirt_ctx_last_kernel(ctx));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
