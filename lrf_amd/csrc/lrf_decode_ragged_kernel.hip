// lrf_decode_ragged_kernel.hip — the decode of a list of images that differ in size and ranks (lrf_qmf_decode_ragged_rgb_u8; host
// side: lrf_encode8.hip, launch plan: plan_decode_ragged in lrf_plan.cpp).  The kernels run the decode bodies of lrf_kernels.hip
// (decode16_tile, decode_strip_tile, decode8_body, decode_body — the very functions k_decode16 / k_decode_strip / k_decode8 /
// k_decode run) with the same sink, DecodeStore; what is new is only where a workgroup learns its image from: not from
// blockIdx.y and kernel arguments, but from a table.
//
//   blocks[blockIdx.x]   -> (image, tile): which image this workgroup works on and which tile (tiled bodies) or group of pixel
//                           quads (the others) inside it
//   descs[image]         -> the image's geometry, ranks, class and the offsets of its factors and of its output
//
// Both indices are uniform over the workgroup (blockIdx.x, then a value loaded through it), and both tables are read-only kernel
// arguments, so the compiler fetches the entry and the ~260 bytes of the descriptor with scalar loads into SGPRs — the same place
// the uniform kernels' arguments live — and the per-lane code of the bodies is what it is in the uniform kernels.
//
//   k_decode_ragged_tiled<STRIP, CLS>  STRIP = false, CLS = -1: all 16-aligned images of a call in one launch, the rank-bound
//                        instantiation picked by the image's class (a uniform switch, as in k_sse_tiled<false, -1>).
//                        STRIP = true, CLS = 0..4: the strip body of one class (under a switch it would take 204 registers)
//   k_decode8_ragged     ranks <= 8 on the geometries the tiled bodies do not cover
//   k_decode_ragged_any  every geometry and rank

// grid: the launch's entries of the block table, 256 threads.  The instantiation with the class switch asks for seven waves per SIMD
// (what k_decode16's largest class runs at): left alone the compiler schedules the switch arms into 94 registers, five waves, and
// 256 x 512x768 at (7,3,3) take 0.126 ms instead of 0.112 (the uniform k_decode16<4, 8>: 0.097); with the request it is 66
// registers and 16 bytes of scratch per lane.  The strip instantiations keep the compiler's choice (62-168 registers by class).
template <bool STRIP, int CLS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CLS < 0 ? 7 : 1))) void k_decode_ragged_tiled(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                             const RaggedDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks)
{
    constexpr int RLM = CLS < 0 || CLS == 4 ? 32 : (CLS >= 2 ? 16 : 8), RCM = CLS < 0 || CLS >= 3 ? 16 : (CLS >= 1 ? 8 : 4);
    __shared__ __attribute__((aligned(16))) float VsL[RLM * 64], VsC[2 * RCM * 64];
    const RaggedBlock b = blocks[blockIdx.x];
    const RaggedDesc& d = descs[b.image];
    const long hw = (long)d.H * d.W;
    DecodeStore sink{rgb + d.rgb_off, hw, d.W};
    const int8_t* Ui = U + d.u_off;
    const int8_t* Vi = V + d.v_off;
#define LRF_RAGGED_TILE(RC, RL)                                                                                          \
    do {                                                                                                                 \
        if constexpr (STRIP) decode_strip_tile<RC, RL>(Ui, Vi, d.H, d.W, d.g, d.R0, d.R1, d.R2, b.tile, d.per_strip, VsL, VsC, sink); \
        else decode16_tile<RC, RL>(Ui, Vi, d.g, d.R0, d.R1, d.R2, b.tile, VsL, VsC, sink);                                \
    } while (0)
    switch (CLS < 0 ? d.cls : CLS) {
    case 0: LRF_RAGGED_TILE(4, 8); break;
    case 1: LRF_RAGGED_TILE(8, 8); break;
    case 2: LRF_RAGGED_TILE(8, 16); break;
    case 3: LRF_RAGGED_TILE(16, 16); break;
    default: LRF_RAGGED_TILE(16, 32); break;
    }
#undef LRF_RAGGED_TILE
}

// b.tile: the image's group of 256 x reps pixel quads.  reps is the launch's (decode8_reps_of its total); a quad's bytes do not
// depend on it — it only says which thread computes the quad
__global__ __launch_bounds__(256) void k_decode8_ragged(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                        const RaggedDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks, int reps)
{
    __shared__ float Vs[3][64 * 8];
    const RaggedBlock b = blocks[blockIdx.x];
    const RaggedDesc& d = descs[b.image];
    DecodeStore sink{rgb + d.rgb_off, (long)d.H * d.W, d.W};
    decode8_body(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, b.tile, reps, Vs, sink);
}

__global__ __launch_bounds__(256) void k_decode_ragged_any(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                           const RaggedDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks)
{
    const RaggedBlock b = blocks[blockIdx.x];
    const RaggedDesc& d = descs[b.image];
    DecodeStore sink{rgb + d.rgb_off, (long)d.H * d.W, d.W};
    decode_body(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, (long)b.tile, sink);
}
