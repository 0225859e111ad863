// mirt_lds_block_text.inc -- how a block of a persistent LDS grid begins, as TEXT: included by the three MIRT_QUERY_LDS kernels and by
// mirt_adapt_lds_text.inc with `kWaves` and `units` in scope and GRID a template parameter.  MIRT_LDS_SKY is stage_scene's sky argument.
    if (blockIdx.x * kWaves >= units) return;                               // the whole block: nothing staged, no barrier met
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, !GRID>(A, smem, MIRT_LDS_SKY);
    GridLds G{};
    if constexpr (GRID) G = stage_grid(A, smem + scene_lds_bytes_dev(A.n_spheres, A.n_mats, MIRT_LDS_SKY, false));
    // no block barrier from here on: a wave without units leaves, the others stride over theirs
    const uint32_t lane = threadIdx.x & 63u;
