// mirt_feature_kernel.inc -- first-hit feature frames of a resident MIRT_SCENE_HBM scene (mirt_ctx_render_features*; DESIGN.md 10.8).
// Included once by mirt_kernels.hip behind mirt_trace_kernel.inc (whose vector types it shares), exact build only: there is no
// fast_build:: copy and no counting build.
//
// feature_frame_kernel<BVH>: lane = pixel, 64 consecutive COMPACT pixels per wave, kBlockThreads threads per block, one pixel per thread
// and no loop over pixels; the pixel itself is mirt_feature_item_text.inc.  Lanes of the last wave beyond out_rows x width are not alive: they take part in the wave's loops with their
// tests masked off and store nothing.  A pixel traces the CENTRE ray first -- generate_primary with both jitter draws replaced by 0.5
// and a zero lens, no random draw -- whose nearest hit is the record's `sphere` and `t`, and then its sample set: the centre ray alone
// for spp == 0, else the renderer's own primary rays of samples sample_begin .. sample_begin + spp - 1 (generate_primary itself: jitter,
// lens, pinhole shortcut, the RNG seeded as a render launch seeds it).  The loop over samples has the same trip count in every lane.
// A sample that hits adds the shading normal inv_r * (point - centre) and the albedo its material's scatter routine would attenuate
// with (without the lambertian's grazing factor, without a scatter direction, without a further draw) to two float sums that start
// at +0; the record holds sum / max(spp, 1).
//   BVH = true : nearest_hit_bvh itself, started at kMaxT -- the render kernels' walk.  It reads the tree through per_strip_args(), i.e.
//                from the start of the kernarg segment, which is why RenderArgs is the FIRST kernel argument (mirt_api.hip: fill_bvh_args).
//                Traversal stacks: 64 per wave of RenderArgs.bvh_stack_entries node references, lane-interleaved, the only dynamic LDS.
//   BVH = false: the flat scan, test_sphere over the prepared sphere table in ORIGINAL index order (MIRT_FEATURES_FLAT).
// The camera is wave-uniform and comes from the kernel arguments; no scene table is staged.  A hit reads its PreparedSphere (two
// 16-byte loads) and PreparedMaterial from global memory.  A record (MirtFeaturePixel, 32 bytes) leaves as two 16-byte stores through
// a 4-byte-aligned vector type: consecutive lanes write consecutive records, 2 KB per wave.

MIRT_DEV CamRegs feature_camera(const RenderArgs& A)
{
    CamRegs c;
    c.eye = mk(A.cam.eye[0], A.cam.eye[1], A.cam.eye[2]);
    c.hor = mk(A.cam.horizontal[0], A.cam.horizontal[1], A.cam.horizontal[2]);
    c.ver = mk(A.cam.vertical[0], A.cam.vertical[1], A.cam.vertical[2]);
    c.llc = mk(A.cam.lower_left_corner[0], A.cam.lower_left_corner[1], A.cam.lower_left_corner[2]);
    c.cam_u = mk(A.cam.u[0], A.cam.u[1], A.cam.u[2]);
    c.cam_v = mk(A.cam.v[0], A.cam.v[1], A.cam.v[2]);
    c.lens_radius = A.cam.lens_radius;
    c.pinhole = bits(A.cam._padding5) != 0u;           // written by the host for this launch (launch_features), as launch_render does
    c.inv_w = 1.0f / (float)A.width;
    c.inv_h = 1.0f / (float)A.height;
    return c;
}

template <bool BVH>
MIRT_DEV int feature_nearest_hit(const RenderArgs& A, f3 ro, f3 rd, bool alive, float& closest, Work<false>& work, uint32_t lane, uint32_t* stack)
{
    if constexpr (BVH) {
        return nearest_hit_bvh<false>(ro, rd, alive, closest, work, lane, stack, A.bvh_stack_entries);
    } else {
        const float a = dot(rd, rd);
        const float inv_a = rcp_(a);
        closest = kMaxT;
        int best = -1;
        const float4* sph = reinterpret_cast<const float4*>(A.spheres);      // {centre, r^2}: the first half of PreparedSphere i
        const uint32_t n = A.n_spheres;
        for (uint32_t s = 0; s < n; ++s) test_sphere<false>(sph[2ull * s], s, ro, rd, a, inv_a, alive, closest, best, work);
        return best;
    }
}

// What a hit adds to the sums: sphereIntersection's normal (wgsl:431-440, not turned towards the ray) and the attenuation of the
// material's scatter routine (scatterRay's switch, wgsl:174-202) without its direction.  Runs in the lanes that hit.
// (feature_of_hit_lds, mirt_feature_lds_kernel.inc, is this body with the staged tables: one body for both changes the code objects,
// profiles/r25_isa_identity.md.)
MIRT_DEV void feature_of_hit(const RenderArgs& A, int best, float t, f3 ro, f3 rd, f3& hn, f3& albedo)
{
    const PreparedSphere sp = A.spheres[best];
    const f3 hp = fma3(t, rd, ro);
    hn = sp.inv_r * (hp - mk(sp.cx, sp.cy, sp.cz));
    const PreparedMaterial* m = &A.pmats[sp.material_idx];
    switch (m->id) {
    case 0u:
    case 1u: albedo = albedo_at(A, m, 0, hn); break;
    case 2u: albedo = mk(1, 1, 1); break;
    case 3u: albedo = albedo_at(A, m, sin_product_negative(5.0f * hp.x, 5.0f * hp.y, 5.0f * hp.z) ? 0 : 1, hn); break;
    default: albedo = mk(0.9921f, 0.24705f, 0.57254f); break;
    }
}

template <bool BVH>
__global__ __launch_bounds__(kBlockThreads) void feature_frame_kernel(RenderArgs A, trace_u4* out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const bool alive = i < (uint64_t)A.out_rows * A.width;
    const uint32_t pi = alive ? (uint32_t)i : 0u;                       // dead lanes compute pixel 0's rays and use none of them
    const uint32_t ci = pi / A.width;
    const uint32_t x = pi - ci * A.width, y = abs_row(A, ci);
    uint32_t* const stack = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * (64u * A.bvh_stack_entries);
    const CamRegs C = feature_camera(A);
    Work<false> work;
    work.clear();

#define MIRT_FEATURE_NEAREST feature_nearest_hit<BVH>(A, ro, rd, alive, closest, work, lane, stack)
#define MIRT_FEATURE_OF_HIT feature_of_hit(A, best, closest, ro, rd, hn, al)
#include "mirt_feature_item_text.inc"
#undef MIRT_FEATURE_NEAREST
#undef MIRT_FEATURE_OF_HIT
}

static QueryKernel feature_kernel(const QueryPlan& p)
{
    return with_bools<QueryKernel>([](auto B) { return kernel_handle(feature_frame_kernel<B.value>); }, p.bvh);
}
