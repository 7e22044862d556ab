// lrf_gray_encode_kernel.hip — the kernels of the gray encode lists (lrf_qmf_encode_gray_ragged_u8,
// lrf_qmf_encode_gray_ragged_sweep_u8, lrf_qmf_sse_gray_ragged_u8; host side: lrf_gray_encode_host.inc, tables:
// plan_encode_gray_ragged_sweep in lrf_plan.cpp).  Included by lrf_channels.hip behind lrf_channels_kernel.hip and
// lrf_gray_loader_kernel.hip, whose bodies they run.
//
// The planes stage, uint8 -> X [M][64] fp32 for a list of images of mixed sizes: a pure stream, 1 byte in and 4 out per pixel.
//   blocks[blockIdx.x] -> (image, tile): which image this workgroup works on and which group of 256 items inside it
//   descs[image]       -> the image's size and padding, the offset of its bytes in gray and of its matrix in the X workspace
// Both are uniform over the workgroup (scalar loads).  The per-item bodies are the uniform kernels' (gray_planes16_item,
// gray_planes_item), so X is the same bits by construction; an item's place in its image takes one 32-bit division per thread
// (an image has fewer than 2^30 items), and there is no loop.
//   k_gray_planes16_ragged   images with W % 16 == 0 whose bytes start at a multiple of 16: a lane loads 16 pixels (one 16-byte
//                            load) and stores four 16-byte pieces; the eight lanes of a patch pair write 512 contiguous bytes
//   k_gray_planes_ragged     the others: a lane forms four columns of a patch row from single bytes and stores 16 bytes
__global__ __launch_bounds__(256) void k_gray_planes16_ragged(const uint8_t* __restrict__ gray, float* __restrict__ X,
                                                              const EncGrayDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks)
{
    const RaggedBlock b = blocks[blockIdx.x];
    const EncGrayDesc& d = descs[b.image];
    const unsigned t = (unsigned)b.tile * 256u + threadIdx.x;
    if (t >= (unsigned)d.items) return;
    const int a = (int)(t & 7u);
    const unsigned pair = t >> 3, nch = (unsigned)d.W >> 4;
    const unsigned hh = pair / nch, j = pair - hh * nch;
    gray_planes16_item(gray + d.gray_off, d.H, d.W, d.top, (int)hh, (int)j, a, reinterpret_cast<float4*>(X + d.x_off + (long)pair * 128 + a * 8));
}

__global__ __launch_bounds__(256) void k_gray_planes_ragged(const uint8_t* __restrict__ gray, float* __restrict__ X,
                                                            const EncGrayDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks)
{
    const RaggedBlock b = blocks[blockIdx.x];
    const EncGrayDesc& d = descs[b.image];
    const unsigned e = (unsigned)b.tile * 256u + threadIdx.x;
    if (e >= (unsigned)d.items) return;
    const unsigned m = e >> 4;
    const int a = (int)(e & 15u) >> 1, b0 = (int)(e & 1u) * 4;
    const unsigned hh = m / (unsigned)d.nw, ww = m - hh * (unsigned)d.nw;
    gray_planes_item(gray + d.gray_off, d.H, d.W, d.top, d.left, (int)hh, (int)ww, a, b0, reinterpret_cast<float4*>(X + d.x_off + (long)e * 4));
}

// The scorer: where the decoder's pixels go is a type (GrayU8Out, GrayTensorOut<T>); this sink compares them with the source at
// the same element offset instead of storing them and keeps the lane's sum of squared differences.  A lane of gray_window1_wg
// holds at most 16 pixels: at most 16 * 255^2 < 2^21.
struct GraySseSink {
    const uint8_t* __restrict__ p;
    mutable unsigned acc;
    __device__ __forceinline__ void add(unsigned s, unsigned b) const
    {
        const int dlt = (int)s - (int)b;
        acc += (unsigned)(dlt * dlt);
    }
    __device__ __forceinline__ void add4(unsigned s, unsigned w) const
    {
#pragma unroll
        for (int i = 0; i < 4; i++) add((s >> (8 * i)) & 255u, (w >> (8 * i)) & 255u);
    }
    __device__ __forceinline__ void put1(long e, unsigned b) const { add(p[e], b & 255u); }
    __device__ __forceinline__ void put4(long e, unsigned w) const
    {
        const uint8_t* o = p + e;
        if ((reinterpret_cast<uintptr_t>(o) & 3) == 0)
            add4(*reinterpret_cast<const unsigned*>(o), w);
        else
#pragma unroll
            for (int i = 0; i < 4; i++) add(o[i], (w >> (8 * i)) & 255u);
    }
    __device__ __forceinline__ void put8(long e, unsigned lo, unsigned hi) const
    {
        const uint8_t* o = p + e;
        if ((reinterpret_cast<uintptr_t>(o) & 7) == 0) {
            const uint2 s = *reinterpret_cast<const uint2*>(o);
            add4(s.x, lo);
            add4(s.y, hi);
        } else {
            put4(e, lo);
            put4(e + 4, hi);
        }
    }
};

// gray_window1_wg's body with that sink over whole images (items: y0 = x0 = 0, h = H, w = W, out_off = where the source is
// read, pitch = W) and the workgroup reduction behind it: uint32 per lane and wave (64 * 2^21 < 2^27), uint64 per workgroup, one
// 64-bit integer atomic per workgroup into sse[place].  grid: nitems x wgs; the workgroups an item does not need add nothing.
__global__ __launch_bounds__(256) void k_gray_sse(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const uint8_t* __restrict__ gray,
                                                  const GrayDesc* __restrict__ descs, const GrayItem* __restrict__ items, int wgs,
                                                  unsigned long long* __restrict__ sse)
{
    __shared__ unsigned wsum[4];
    const GraySseSink sink{gray, 0u};
    gray_window1_wg(U, V, sink, descs, items, wgs);
    unsigned s = sink.acc;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(sse + items[blockIdx.x / (unsigned)wgs].place, tot);
    }
}
