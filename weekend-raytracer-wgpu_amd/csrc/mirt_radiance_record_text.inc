// mirt_radiance_record_text.inc -- how a MirtRadiance record leaves, as TEXT: included by mirt_radiance_item_text.inc and by
// radiance_rays_pool_kernel's epilogue with `i`, `out` and the sums acc_r / acc_g / acc_b in scope.  MIRT_RADIANCE_ARGS names the
// arguments reference (A, or the pool kernel's AS).  With MIRT_RADIANCE_ACCUMULATE (wave-uniform) two 16-byte loads precede the stores.
    uint32_t samples = MIRT_RADIANCE_ARGS.spp;
    if (MIRT_RADIANCE_ARGS.flags & kRadianceAccumulate) {
        const trace_u4 o0 = out[2u * i], o1 = out[2u * i + 1u];
        acc_r += (unsigned long long)o0.x | ((unsigned long long)o0.y << 32);
        acc_g += (unsigned long long)o0.z | ((unsigned long long)o0.w << 32);
        acc_b += (unsigned long long)o1.x | ((unsigned long long)o1.y << 32);
        samples += o1.z;
    }
    out[2u * i] = trace_u4{ (uint32_t)acc_r, (uint32_t)(acc_r >> 32), (uint32_t)acc_g, (uint32_t)(acc_g >> 32) };
    out[2u * i + 1u] = trace_u4{ (uint32_t)acc_b, (uint32_t)(acc_b >> 32), samples, 0u };
