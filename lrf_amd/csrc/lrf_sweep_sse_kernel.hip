// lrf_sweep_sse_kernel.hip — the squared error of a quality sweep straight from its factors (lrf_qmf_sweep_sse_rgb_u8; host side:
// lrf_encode8.hip).  What lrf_qmf_decode_rgb_u8 followed by lrf_image_metrics_u8(ssim = NULL) computes, without the decoded
// image: the kernels run the decode bodies of lrf_kernels.hip (decode16_tile, decode_strip_tile, decode8_body, decode_body — the
// very functions k_decode16 / k_decode_strip / k_decode8 / k_decode run) with a sink that, where the decode kernel stores a run
// of bytes, loads the same run of the SOURCE image and adds up the squared differences.
//
//   k_sse_tiled<STRIP, CLS>  a workgroup per (triple, image, tile of 16 rows x 32 luma patches).  CLS = -1: the rank-bound
//                        instantiation of the body is picked by the triple's class (a uniform switch) — the 16-aligned body, whose
//                        five instantiations take 47-68 registers, the switch over them 68: one launch for the whole sweep.
//                        CLS = 0..4: that instantiation alone — the strip body, which takes 62-168 registers by class and 204
//                        under a switch (two waves per SIMD for every triple): one launch per class present, each at its own
//                        occupancy (compiler's resource report, gfx950)
//   k_sse8               ranks <= 8 on the geometries the tiled bodies do not cover
//   k_sse_any            every geometry and rank
//
// Work item = ONE (triple, tile), not a loop over the triples of a tile.  The loop would read the tile's 12 KB of source once
// instead of Q times, but the bodies are bound by the vector instructions they issue, not by bytes (k_decode16: VALU busy 73 %),
// and a loop would have to re-stage the three V tables behind two more barriers per triple and wait for the next triple's u rows
// with nothing to overlap them — or hold two triples' rows, which at the (16, 32) rank bounds costs the eight waves per SIMD the
// body depends on.  Instead the triples of one tile are NEIGHBOURS in the grid (blockIdx.x = tile * nq + item), so they are
// dispatched together and all but the first find the source rows in L2.
//
// Sums.  Bytes a (decoded) and s (source): sum (a - s)^2 = sum a a + sum s s - 2 sum a s, three v_dot4_u32_u8 per dword of four
// pixels on the packed words the decode body produces anyway — no unpacking.  A lane keeps the two uint32 sums (at most 64
// pixels x 3 channels x 2 x 255^2 = 2.5e7 each), their difference is the lane's squared error (<= 1.25e7), a wave adds its 64
// lanes in uint32 (<= 8e8), thread 0 adds the four waves in uint64 and issues ONE 64-bit integer vector atomic per workgroup to
// sse[q][b] (zeroed by the host before the launch).  Integer sums: any order gives the same value, so an image's result depends
// on neither B, Q nor its place.  No floating point enters the sum.

// one rank triple of the call: a row of the table the host uploads (and keeps while the call's shape does not change)
struct SseItem {
    long u_base, v_base; // int8 elements from U / V to the factors of the triple's image 0
    long u_img, v_img;   // ... and from one image to the next
    int R0, R1, R2;
    int q;               // row of sse
    int cls;             // tiled kernels: index of the rank bounds (chroma, luma) = (4,8) (8,8) (8,16) (16,16) (16,32)
    int pad;
};

struct SseSink {
    const uint8_t* src; // the source image [3][H][W]
    long hw;
    int W;
    unsigned sq = 0, cross = 0; // sum a a + s s, sum a s (put1 adds (a - s)^2 to sq)
    __device__ __forceinline__ void add4(unsigned a, unsigned s)
    {
        sq = __builtin_amdgcn_udot4(a, a, sq, false);
        sq = __builtin_amdgcn_udot4(s, s, sq, false);
        cross = __builtin_amdgcn_udot4(a, s, cross, false);
    }
    __device__ __forceinline__ void put8(int y, int x, const uint2 (&pk)[3])
    {
        const uint8_t* p = src + (long)y * W + x;
        uint2 s[3];
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] = *reinterpret_cast<const uint2 __attribute__((aligned(1)))*>(p + k * hw);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            add4(pk[k].x, s[k].x);
            add4(pk[k].y, s[k].y);
        }
    }
    __device__ __forceinline__ void put8u(int y, int x, const uint2 (&pk)[3]) { put8(y, x, pk); }
    __device__ __forceinline__ void put4(int ch, int y, int x, unsigned w)
    {
        add4(w, *reinterpret_cast<const uint32_t __attribute__((aligned(1)))*>(src + (long)ch * hw + (long)y * W + x));
    }
    __device__ __forceinline__ void put1(int ch, int y, int x, unsigned v)
    {
        const int d = (int)(v & 255u) - (int)src[(long)ch * hw + (long)y * W + x];
        sq += (unsigned)__mul24(d, d);
    }
    __device__ __forceinline__ unsigned total() const { return sq - 2u * cross; }
};

// every thread of the workgroup (256) calls this once, after its body: lane sums -> wave (uint32) -> workgroup (uint64) -> one atomic
__device__ __forceinline__ void sse_block_add(unsigned t, unsigned long long* __restrict__ dst)
{
    __shared__ unsigned part[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long s = (unsigned long long)part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(dst, s);
    }
}

// grid (tiles x nq, B), 256 threads.  tiles: k_decode16's (STRIP = false) or k_decode_strip's (true) for this geometry.
template <bool STRIP, int CLS>
__global__ __launch_bounds__(256) void k_sse_tiled(const uint8_t* __restrict__ rgb, const int8_t* __restrict__ U, const int8_t* __restrict__ V, int H, int W,
                                                   ImageGeom g, const SseItem* __restrict__ items, int nq, int per_strip, int B,
                                                   unsigned long long* __restrict__ sse)
{
    constexpr int RLM = CLS < 0 || CLS == 4 ? 32 : (CLS >= 2 ? 16 : 8), RCM = CLS < 0 || CLS >= 3 ? 16 : (CLS >= 1 ? 8 : 4);
    __shared__ __attribute__((aligned(16))) float VsL[RLM * 64], VsC[2 * RCM * 64];
    const int tile = blockIdx.x / nq;
    const SseItem it = items[blockIdx.x - tile * nq];
    const long hw = (long)H * W;
    SseSink sink{rgb + (long)blockIdx.y * 3 * hw, hw, W};
    const int8_t* Ui = U + it.u_base + (long)blockIdx.y * it.u_img;
    const int8_t* Vi = V + it.v_base + (long)blockIdx.y * it.v_img;
#define LRF_SSE_TILE(RC, RL)                                                                                      \
    do {                                                                                                          \
        if constexpr (STRIP) decode_strip_tile<RC, RL>(Ui, Vi, H, W, g, it.R0, it.R1, it.R2, tile, per_strip, VsL, VsC, sink); \
        else decode16_tile<RC, RL>(Ui, Vi, g, it.R0, it.R1, it.R2, tile, VsL, VsC, sink);                          \
    } while (0)
    switch (CLS < 0 ? it.cls : CLS) {
    case 0: LRF_SSE_TILE(4, 8); break;
    case 1: LRF_SSE_TILE(8, 8); break;
    case 2: LRF_SSE_TILE(8, 16); break;
    case 3: LRF_SSE_TILE(16, 16); break;
    default: LRF_SSE_TILE(16, 32); break;
    }
#undef LRF_SSE_TILE
    sse_block_add(sink.total(), sse + (long)it.q * B + blockIdx.y);
}

// grid (groups x nq, B), 256 threads; groups = ceil(H ceil(W/4) / (256 reps)): k_decode8's
__global__ __launch_bounds__(256) void k_sse8(const uint8_t* __restrict__ rgb, const int8_t* __restrict__ U, const int8_t* __restrict__ V, int H, int W,
                                              ImageGeom g, const SseItem* __restrict__ items, int nq, int reps, int B, unsigned long long* __restrict__ sse)
{
    __shared__ float Vs[3][64 * 8];
    const int grp = blockIdx.x / nq;
    const SseItem it = items[blockIdx.x - grp * nq];
    const long hw = (long)H * W;
    SseSink sink{rgb + (long)blockIdx.y * 3 * hw, hw, W};
    decode8_body(U + it.u_base + (long)blockIdx.y * it.u_img, V + it.v_base + (long)blockIdx.y * it.v_img, H, W, g, it.R0, it.R1, it.R2, grp, reps, Vs, sink);
    sse_block_add(sink.total(), sse + (long)it.q * B + blockIdx.y);
}

// grid (groups x nq, B), 256 threads; groups = ceil(H ceil(W/4) / 256): k_decode's
__global__ __launch_bounds__(256) void k_sse_any(const uint8_t* __restrict__ rgb, const int8_t* __restrict__ U, const int8_t* __restrict__ V, int H, int W,
                                                 ImageGeom g, const SseItem* __restrict__ items, int nq, int B, unsigned long long* __restrict__ sse)
{
    const int grp = blockIdx.x / nq;
    const SseItem it = items[blockIdx.x - grp * nq];
    const long hw = (long)H * W;
    SseSink sink{rgb + (long)blockIdx.y * 3 * hw, hw, W};
    decode_body(U + it.u_base + (long)blockIdx.y * it.u_img, V + it.v_base + (long)blockIdx.y * it.v_img, H, W, g, it.R0, it.R1, it.R2, (long)grp, sink);
    sse_block_add(sink.total(), sse + (long)it.q * B + blockIdx.y);
}
