// temporal_demo — mirt_host::reproject of the C++ mirror: a denoised frame carried across camera motion.
//   temporal_demo FRAMES   the scene of probe_demo (three spheres on a ground sphere, MIRT_SCENE_HBM) through a 32 x 24 viewport while the
//                          camera pans: frame k looks from (0.2 k, 2, 9).  Every frame is a fresh accumulation of 2 spp under seed 7 + k,
//                          its guides from render_features, the a-trous filter at levels 3, sigma_colour 1, normal_log2 5 to float32, and
//                          from the second frame on mirt_ctx_reproject against the previous result (max_history 4, depth_tolerance 0.05,
//                          clamp).  Prints "frame <k>: history <n> of <pixels>" -- the pixels whose record carries a history longer than
//                          1 --, for the last frame "px <i>: <r> <g> <b> <length> <rgba8>" with the float32 bits and the RGBA8 word in
//                          hex, and the kernel's name.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>

#include "mirt_host.hpp"

using namespace mirt_host;

int main(int argc, char** argv)
{
    try {
        if (argc < 2 || std::atoi(argv[1]) < 1) { std::fprintf(stderr, "usage: temporal_demo FRAMES\n"); return 2; }
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
        const size_t n = (size_t)w * h;
        auto camera_of = [&](int k) {
            MirtCamera cam{ { 0.2f * (float)k, 2.0f, 9.0f }, { 0.0f, -0.1f, -1.0f }, { 0.0f, 1.0f, 0.0f }, mirt_degrees_to_radians(40.0f), 0.0f, 9.0f };
            MirtGpuCamera g{};
            check(mirt_camera_new(&cam, w, h, &g));
            return g;
        };
        MirtGpuCamera gpu_cam = camera_of(0);
        MirtScene sc{};
        sc.camera = &gpu_cam; sc.spheres = spheres; sc.n_spheres = 4u; sc.materials = &mat; sc.n_materials = 1u; sc.texels = texel; sc.n_texels = 1u;

        MirtContext* ctx = nullptr;
        check(mirt_ctx_create(0, &ctx));
        std::unique_ptr<MirtContext, void (*)(MirtContext*)> guard(ctx, mirt_ctx_destroy);
        set_scene(ctx, sc, MIRT_SCENE_HBM);                   // feature frames need the world in device memory

        std::vector<float> history;
        std::vector<MirtFeaturePixel> prev_guides;
        std::vector<uint8_t> rgba(n * 4u), frame(n * 4u);
        MirtGpuCamera prev_cam = gpu_cam;
        for (int k = 0; k < frames; ++k) {
            const MirtGpuCamera cam = camera_of(k);
            check(mirt_ctx_set_camera(ctx, &cam));
            MirtParams p{};
            p.width = w; p.height = h; p.spp = 2u; p.num_bounces = 8u; p.mode = MIRT_MODE_PT; p.seed = 7u + (uint64_t)k;
            check(mirt_ctx_accum_reset(ctx, &p));
            check(mirt_ctx_accum_frame(ctx, &p, frame.data(), frame.size()));
            const std::vector<MirtFeaturePixel> guides = render_features(ctx, p);
            const std::vector<uint8_t> lin = denoise(ctx, p, denoise_params(MIRT_DENOISE_SRC_ACCUM, 3u, 1.0f, 5u, true), guides);
            std::vector<float> colour(n * 4u);
            std::memcpy(colour.data(), lin.data(), lin.size());
            if (k == 0) {
                history = colour;                             // a denoise output is a history of length 1
                rgba = denoise(ctx, p, denoise_params(), guides);
            } else {
                history = reproject(ctx, p, reproject_params(prev_cam, cam), colour, guides, history, prev_guides, &rgba);
            }
            size_t with_history = 0;
            for (size_t i = 0; i < n; ++i) with_history += history[4u * i + 3u] > 1.0f ? 1u : 0u;
            std::printf("frame %d: history %zu of %zu\n", k, with_history, n);
            prev_guides = guides;
            prev_cam = cam;
        }
        for (size_t i = 0; i < n; ++i) {
            uint32_t f[4], c;
            std::memcpy(f, history.data() + 4u * i, 16u);
            std::memcpy(&c, rgba.data() + 4u * i, 4u);
            std::printf("px %zu: %08x %08x %08x %08x %08x\n", i, f[0], f[1], f[2], f[3], c);
        }
        const std::array<float, 3> centre = camera_project(prev_cam, w, h, { 0.0f, 1.0f, 0.0f });
        uint32_t cb[3];
        std::memcpy(cb, centre.data(), sizeof cb);
        std::printf("sphere 2 at: %08x %08x %08x\n", cb[0], cb[1], cb[2]);
        std::printf("kernel: %s\n", mirt_ctx_last_kernel(ctx));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
