// lrf_sse_ragged_kernel.hip — the squared error of a list of (factors, source) items that differ in size and ranks, straight from
// the factors (lrf_qmf_sse_ragged_rgb_u8; host side: lrf_encode8.hip, launches: plan_decode_ragged in lrf_plan.cpp).  The two
// halves exist already: lrf_decode_ragged_kernel.hip says where a workgroup learns its item from —
//
//   blocks[blockIdx.x]   -> (item, tile): which item this workgroup works on and which tile (tiled bodies) or group of pixel
//                           quads (the others) inside it
//   descs[item]          -> the item's geometry, ranks, class, the offsets of its factors, and in rgb_off where its SOURCE
//                           [3][H][W] is read (several items may name the same source: the candidates of one image do)
//
// both uniform over the workgroup, fetched with scalar loads — and lrf_sweep_sse_kernel.hip has the sink, SseSink, which loads
// the run of source bytes where the decode kernel would store its run and adds up the squared differences.  The kernels below
// are the ragged decode kernels with that sink in place of DecodeStore, ending in sse_block_add(sink.total(), sse + item): the
// decode bodies of lrf_kernels.hip (decode16_tile, decode_strip_tile, decode8_body, decode_body) run unchanged, so the bytes
// compared are the bytes lrf_qmf_decode_ragged_rgb_u8 writes for the same descriptor.
//
// Sums stay integers: uint32 per lane and wave, uint64 per workgroup, ONE 64-bit integer vector atomic per workgroup onto
// sse[item], which the call zeroes on its stream first.  Any order gives the same value: an item's result depends on neither its
// place in the list nor on the other items.
//
//   k_sse_ragged_tiled<STRIP, CLS>  STRIP = false, CLS = -1: all 16-aligned items of a call in one launch under a class switch;
//                        STRIP = true, CLS = 0..4: the strip body of one class, one launch per class present
//   k_sse8_ragged        ranks <= 8 on the geometries the tiled bodies do not cover
//   k_sse_ragged_any     every geometry and rank (1..64)

// grid: the launch's entries of the block table, 256 threads.  Unlike k_decode_ragged_tiled<false, -1> the class-switch
// instantiation asks for no occupancy: left alone the compiler gives it 67 registers, seven waves per SIMD and no scratch (the
// sink keeps two sums where the decoder holds a tile's packed bytes for its stores); with that kernel's request for seven waves
// it is 69 registers and 16 bytes of scratch per lane for the same seven (DESIGN.md section 4.12 has both reports).
template <bool STRIP, int CLS>
__global__ __launch_bounds__(256) void k_sse_ragged_tiled(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const uint8_t* __restrict__ rgb,
                                                          const RaggedDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks,
                                                          unsigned long long* __restrict__ sse)
{
    constexpr int RLM = CLS < 0 || CLS == 4 ? 32 : (CLS >= 2 ? 16 : 8), RCM = CLS < 0 || CLS >= 3 ? 16 : (CLS >= 1 ? 8 : 4);
    __shared__ __attribute__((aligned(16))) float VsL[RLM * 64], VsC[2 * RCM * 64];
    const RaggedBlock b = blocks[blockIdx.x];
    const RaggedDesc& d = descs[b.image];
    const long hw = (long)d.H * d.W;
    SseSink sink{rgb + d.rgb_off, hw, d.W};
    const int8_t* Ui = U + d.u_off;
    const int8_t* Vi = V + d.v_off;
#define LRF_SSE_RAGGED_TILE(RC, RL)                                                                                      \
    do {                                                                                                                 \
        if constexpr (STRIP) decode_strip_tile<RC, RL>(Ui, Vi, d.H, d.W, d.g, d.R0, d.R1, d.R2, b.tile, d.per_strip, VsL, VsC, sink); \
        else decode16_tile<RC, RL>(Ui, Vi, d.g, d.R0, d.R1, d.R2, b.tile, VsL, VsC, sink);                                \
    } while (0)
    switch (CLS < 0 ? d.cls : CLS) {
    case 0: LRF_SSE_RAGGED_TILE(4, 8); break;
    case 1: LRF_SSE_RAGGED_TILE(8, 8); break;
    case 2: LRF_SSE_RAGGED_TILE(8, 16); break;
    case 3: LRF_SSE_RAGGED_TILE(16, 16); break;
    default: LRF_SSE_RAGGED_TILE(16, 32); break;
    }
#undef LRF_SSE_RAGGED_TILE
    sse_block_add(sink.total(), sse + b.image);
}

// b.tile: the item's group of 256 x reps pixel quads; reps is the launch's (decode8_reps_of its total)
__global__ __launch_bounds__(256) void k_sse8_ragged(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const uint8_t* __restrict__ rgb,
                                                     const RaggedDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks, int reps,
                                                     unsigned long long* __restrict__ sse)
{
    __shared__ float Vs[3][64 * 8];
    const RaggedBlock b = blocks[blockIdx.x];
    const RaggedDesc& d = descs[b.image];
    SseSink sink{rgb + d.rgb_off, (long)d.H * d.W, d.W};
    decode8_body(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, b.tile, reps, Vs, sink);
    sse_block_add(sink.total(), sse + b.image);
}

__global__ __launch_bounds__(256) void k_sse_ragged_any(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const uint8_t* __restrict__ rgb,
                                                        const RaggedDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks,
                                                        unsigned long long* __restrict__ sse)
{
    const RaggedBlock b = blocks[blockIdx.x];
    const RaggedDesc& d = descs[b.image];
    SseSink sink{rgb + d.rgb_off, (long)d.H * d.W, d.W};
    decode_body(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, (long)b.tile, sink);
    sse_block_add(sink.total(), sse + b.image);
}
