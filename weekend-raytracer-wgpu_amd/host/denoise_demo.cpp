// denoise_demo — mirt_host::denoise of the C++ mirror: the a-trous filter over a progressive accumulation.
//   denoise_demo FRAMES   the scene of probe_demo (three spheres on a ground sphere, MIRT_SCENE_HBM) through a 32 x 24 viewport: FRAMES
//                         progressive frames of 2 spp, guides from render_features at spp 2, then the filter at levels 3, sigma_colour 1,
//                         normal_log2 5 in both output forms; prints "px <i>: <r> <g> <b> <rgba8>" with the float32 bits and the RGBA8 word
//                         in hex, then the samples accumulated and the kernel's name.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>

#include "mirt_host.hpp"

using namespace mirt_host;

int main(int argc, char** argv)
{
    try {
        if (argc < 2 || std::atoi(argv[1]) < 1) { std::fprintf(stderr, "usage: denoise_demo FRAMES\n"); return 2; }
        const int frames = std::atoi(argv[1]);
        const MirtSphere spheres[4] = { { { 0.0f, -1000.0f, 0.0f, 0.0f }, 1000.0f, 0u, { 0u, 0u } },
                                        { { -2.5f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } },
                                        { { 0.0f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } },
                                        { { 2.5f, 1.0f, 0.0f, 0.0f }, 1.0f, 0u, { 0u, 0u } } };
        MirtMaterial mat{};                                   // one lambertian of one grey texel
        mat.id = 0u;
        mat.desc1 = MirtTextureDescriptor{ 1u, 1u, 0u };
        mat.desc2 = MirtTextureDescriptor{ 0u, 0u, 0xffffffffu };
        const float texel[3] = { 0.5f, 0.5f, 0.5f };
        const uint32_t w = 32u, h = 24u;
        MirtCamera cam{ { 0.0f, 2.0f, 9.0f }, { 0.0f, -0.1f, -1.0f }, { 0.0f, 1.0f, 0.0f }, mirt_degrees_to_radians(40.0f), 0.0f, 9.0f };
        MirtGpuCamera gpu_cam{};
        check(mirt_camera_new(&cam, w, h, &gpu_cam));
        MirtScene sc{};
        sc.camera = &gpu_cam; sc.spheres = spheres; sc.n_spheres = 4u; sc.materials = &mat; sc.n_materials = 1u; sc.texels = texel; sc.n_texels = 1u;

        MirtContext* ctx = nullptr;
        check(mirt_ctx_create(0, &ctx));
        std::unique_ptr<MirtContext, void (*)(MirtContext*)> guard(ctx, mirt_ctx_destroy);
        set_scene(ctx, sc, MIRT_SCENE_HBM);                   // feature frames need the world in device memory

        MirtParams p{};
        p.width = w; p.height = h; p.spp = 2u; p.num_bounces = 8u; p.mode = MIRT_MODE_PT; p.seed = 7u;
        std::vector<uint8_t> frame((size_t)w * h * 4u);
        check(mirt_ctx_accum_reset(ctx, &p));
        for (int f = 0; f < frames; ++f) check(mirt_ctx_accum_frame(ctx, &p, frame.data(), frame.size()));
        const std::vector<MirtFeaturePixel> guides = render_features(ctx, p);
        const std::vector<uint8_t> lin = denoise(ctx, p, denoise_params(MIRT_DENOISE_SRC_ACCUM, 3u, 1.0f, 5u, true), guides);
        const std::vector<uint8_t> rgba = denoise(ctx, p, denoise_params(), guides);
        for (size_t i = 0; i < (size_t)w * h; ++i) {
            uint32_t f[4], c;
            std::memcpy(f, lin.data() + 16u * i, 16u);
            std::memcpy(&c, rgba.data() + 4u * i, 4u);
            std::printf("px %zu: %08x %08x %08x %08x\n", i, f[0], f[1], f[2], c);
        }
        std::printf("samples: %u\n", mirt_ctx_accum_samples(ctx));
        std::printf("kernel: %s\n", mirt_ctx_last_kernel(ctx));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
