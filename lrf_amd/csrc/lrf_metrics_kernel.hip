// lrf_metrics_kernel.hip — PSNR / SSIM of uint8 image pairs [B,C,H,W] (lrf_image_metrics_u8; host side: lrf_metrics.hip).
//
//   k_metrics_pre<V, SSE>   one flat read: SSE = false: max and 255 - min of every image of `a` (the data_range of the SSIM);
//                           SSE = true: sum (a-b)^2 per image (callers that want the PSNR only).  Integer atomics.
//   k_ssim_tiles<V>         one workgroup per (image, channel, tile of 24 x 64 window positions): the 30 x 70 pixels the tile's
//                           windows cover are staged in LDS once (their (a-b)^2 added up on the way, every pixel by the one tile
//                           that owns it), the window sums are formed separably — sums of 7 along the rows by a thread per
//                           (row, 8 columns), then a sliding sum of 7 down each column — as exact integers, and the tile's sum
//                           of S goes to the slot of (image, channel, tile).
//   k_ssim_final            one workgroup per image adds its slots in a fixed order.
//
// Arithmetic ("Metrics on the device").  With Sx, Sy, Sxx, Syy, Sxy the sums over the 49 pixels of a window,
//   S = ((2 ux uy + c1)(2 vxy + c2)) / ((ux^2 + uy^2 + c1)(vx + vy + c2)),  ux = Sx/49, vx = (49 Sxx - Sx^2)/(49*48), ...
// Everything up to the four brackets is an integer that fits 32 bits:
//   P = Sx Sy <= 1.57e8,  Q = Sx^2 + Sy^2 <= 3.13e8,  N1 = 49 Sxy - P (|N1| <= 1.6e8),  N2 = 49 (Sxx + Syy) - Q in [0, 3.2e8]
// so the brackets are P (2/2401) + c1, N1 (2/2352) + c2, Q / 2401 + c1, N2 / 2352 + c2: one float64 multiplication and one
// addition each, then two multiplications and ONE division.  No float64 atomics: a thread adds the S of its (at most six) rows in
// row order, the workgroup adds its 256 threads by a fixed tree, k_ssim_final adds the slots of a channel strided by thread and
// by the same tree.  The tiling depends on (C, H, W) only, so an image's SSIM has the same bits wherever it stands in a batch.
#define LRF_MT_TH 24                       // window positions (rows) per tile
#define LRF_MT_TW 64                       // ... and columns: one thread per column and band of 6 rows
#define LRF_MT_HR (LRF_MT_TH + 6)          // pixel rows a tile's windows cover
#define LRF_MT_HC (LRF_MT_TW + 6)          // ... and columns
#define LRF_MT_PITCH 80                    // bytes per staged row (five 16-byte pieces)
#define LRF_MT_PRE_BYTES (256 * 16 * 8)    // bytes of an image per workgroup of k_metrics_pre

template <int V> struct MtVec;
template <> struct MtVec<16> { typedef uint4 T; };
template <> struct MtVec<4> { typedef unsigned int T; };
template <> struct MtVec<1> { typedef unsigned char T; };

__device__ __forceinline__ unsigned mt_byte(unsigned w, int k) { return (w >> (8 * k)) & 255u; }
// sum (a_k - b_k)^2 over the four bytes of a and b
__device__ __forceinline__ unsigned mt_sse4(unsigned a, unsigned b)
{
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int d = (int)mt_byte(a, k) - (int)mt_byte(b, k);
        s += (unsigned)__mul24(d, d);
    }
    return s;
}
__device__ __forceinline__ void mt_minmax4(unsigned a, unsigned& mx, unsigned& mn255)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned v = mt_byte(a, k);
        mx = max(mx, v);
        mn255 = max(mn255, 255u - v);
    }
}

// What one workgroup of the flat read adds up: bytes lo + V tid, + 256 V, ... below hi of a (and of b: SSE).  a, b aligned to V,
// lo and hi multiples of V.  k_metrics_pre and k_ragged_metrics_pre (lrf_metrics_ragged_kernel.hip) call it.
template <int V, bool SSE>
__device__ __forceinline__ void mt_pre_span(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long lo, long hi, unsigned& mx, unsigned& mn255,
                                            unsigned long long& s)
{
    typedef typename MtVec<V>::T T;
    for (long i = lo + (long)threadIdx.x * V; i < hi; i += 256 * V) {
        const T va = *reinterpret_cast<const T*>(a + i);
        unsigned wa[4] = {0, 0, 0, 0}, wb[4] = {0, 0, 0, 0};
        if constexpr (V == 16) { wa[0] = va.x; wa[1] = va.y; wa[2] = va.z; wa[3] = va.w; }
        else wa[0] = va;
        if constexpr (SSE) {
            const T vb = *reinterpret_cast<const T*>(b + i);
            if constexpr (V == 16) { wb[0] = vb.x; wb[1] = vb.y; wb[2] = vb.z; wb[3] = vb.w; }
            else wb[0] = vb;
            unsigned t = 0;
#pragma unroll
            for (int k = 0; k < (V == 16 ? 4 : 1); k++) t += mt_sse4(wa[k], wb[k]); // (V < 4: the upper bytes of both words are zero)
            s += t;
        } else {
            if constexpr (V == 1) {
                mx = max(mx, wa[0]);
                mn255 = max(mn255, 255u - wa[0]);
            } else {
#pragma unroll
                for (int k = 0; k < (V == 16 ? 4 : 1); k++) mt_minmax4(wa[k], mx, mn255);
            }
        }
    }
}

// grid (ceil(n / LRF_MT_PRE_BYTES), B), 256 threads; n = C H W bytes per image, n % V == 0, a / b aligned to V.
// mm [B][2] = (max, 255 - min) of a, zero before the launch; sse [B], zero before the launch.
template <int V, bool SSE>
__global__ __launch_bounds__(256) void k_metrics_pre(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long n, unsigned* __restrict__ mm,
                                                     unsigned long long* __restrict__ sse)
{
    const long img = (long)blockIdx.y * n;
    const long lo = (long)blockIdx.x * LRF_MT_PRE_BYTES;
    const long hi = min(n, lo + (long)LRF_MT_PRE_BYTES);
    unsigned mx = 0, mn255 = 0;
    unsigned long long s = 0;
    mt_pre_span<V, SSE>(a + img, SSE ? b + img : b, lo, hi, mx, mn255, s);
    __shared__ unsigned s_mx, s_mn;
    __shared__ unsigned long long s_sse;
    if (threadIdx.x == 0) { s_mx = 0; s_mn = 0; s_sse = 0; }
    __syncthreads();
    if constexpr (SSE) {
        if (s) atomicAdd(&s_sse, s);
    } else {
        atomicMax(&s_mx, mx);
        atomicMax(&s_mn, mn255);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (SSE) {
            if (s_sse) atomicAdd(sse + blockIdx.y, s_sse);
        } else {
            atomicMax(mm + 2 * blockIdx.y, s_mx);
            atomicMax(mm + 2 * blockIdx.y + 1, s_mn);
        }
    }
}

// the LDS of one tile (lrf_metrics_tile_body.inc): the staged bytes of a and b, the row sums of 7 — h1: a | b << 16, h2: a^2 + b^2,
// h3: a b —, the tree, the tile's squared error
#define LRF_MT_TILE_LDS \
    __shared__ __attribute__((aligned(16))) unsigned rawA[LRF_MT_HR * LRF_MT_PITCH / 4]; \
    __shared__ __attribute__((aligned(16))) unsigned rawB[LRF_MT_HR * LRF_MT_PITCH / 4]; \
    __shared__ __attribute__((aligned(16))) unsigned h1[LRF_MT_HR * LRF_MT_TW]; \
    __shared__ __attribute__((aligned(16))) unsigned h2[LRF_MT_HR * LRF_MT_TW]; \
    __shared__ __attribute__((aligned(16))) unsigned h3[LRF_MT_HR * LRF_MT_TW]; \
    __shared__ double red[256]; \
    __shared__ unsigned s_sse;

// grid (B C ntx nty), 256 threads.  ntx = ceil((W-6) / 64), nty = ceil((H-6) / 24); W % V == 0 and a / b aligned to V.
// slots [B][C][nty ntx] float64; sse [B] zero before the launch; mm as k_metrics_pre<., false> left it.
template <int V>
__global__ __launch_bounds__(256) void k_ssim_tiles(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int C, int H, int W, int ntx, int nty,
                                                    const unsigned* __restrict__ mm, double* __restrict__ slots, unsigned long long* __restrict__ sse)
{
    typedef typename MtVec<V>::T T;
    LRF_MT_TILE_LDS

    const int tid = threadIdx.x;
    const unsigned nt = (unsigned)(ntx * nty);
    const unsigned plane = blockIdx.x / nt, tile = blockIdx.x - plane * nt; // plane = image * C + channel
    const int ty = (int)(tile / (unsigned)ntx), tx = (int)(tile - (unsigned)ty * (unsigned)ntx);
#include "lrf_metrics_tile_body.inc"
}

// the mean over the channels of (sum of the channel's nt slots) / npix; slots: the image's [C][nt].  All 256 threads of the
// workgroup call it, once; thread 0 holds the result.  k_ssim_final and k_ragged_ssim_final call it.
__device__ __forceinline__ double mt_ssim_mean(const double* __restrict__ slots, int C, int nt, double npix)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int ch = 0; ch < C; ch++) {
        const double* sl = slots + (long)ch * nt;
        double acc = 0.0;
        for (int i = tid; i < nt; i += 256) acc += sl[i];
        __syncthreads();
        red[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        total += red[0] / npix;
    }
    return total / (double)C;
}

// grid (B), 256 threads: ssim[b] = mean over the channels of (sum of the channel's slots) / ((H-6)(W-6))
__global__ __launch_bounds__(256) void k_ssim_final(const double* __restrict__ slots, int C, int nt, double npix, double* __restrict__ ssim)
{
    const double v = mt_ssim_mean(slots + (long)blockIdx.x * C * nt, C, nt, npix);
    if (threadIdx.x == 0) ssim[blockIdx.x] = v;
}
