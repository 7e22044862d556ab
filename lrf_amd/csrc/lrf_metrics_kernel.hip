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

// grid (ceil(n / LRF_MT_PRE_BYTES), B), 256 threads; n = C H W bytes per image, n % V == 0, a / b aligned to V.
// mm [B][2] = (max, 255 - min) of a, zero before the launch; sse [B], zero before the launch.
template <int V, bool SSE>
__global__ __launch_bounds__(256) void k_metrics_pre(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long n, unsigned* __restrict__ mm,
                                                     unsigned long long* __restrict__ sse)
{
    typedef typename MtVec<V>::T T;
    const long img = (long)blockIdx.y * n;
    const long lo = (long)blockIdx.x * LRF_MT_PRE_BYTES;
    const long hi = min(n, lo + (long)LRF_MT_PRE_BYTES);
    unsigned mx = 0, mn255 = 0;
    unsigned long long s = 0;
    for (long i = lo + (long)threadIdx.x * V; i < hi; i += 256 * V) {
        const T va = *reinterpret_cast<const T*>(a + img + i);
        unsigned wa[4] = {0, 0, 0, 0}, wb[4] = {0, 0, 0, 0};
        if constexpr (V == 16) { wa[0] = va.x; wa[1] = va.y; wa[2] = va.z; wa[3] = va.w; }
        else wa[0] = va;
        if constexpr (SSE) {
            const T vb = *reinterpret_cast<const T*>(b + img + i);
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

// grid (B C ntx nty), 256 threads.  ntx = ceil((W-6) / 64), nty = ceil((H-6) / 24); W % V == 0 and a / b aligned to V.
// slots [B][C][nty ntx] float64; sse [B] zero before the launch; mm as k_metrics_pre<., false> left it.
template <int V>
__global__ __launch_bounds__(256) void k_ssim_tiles(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int C, int H, int W, int ntx, int nty,
                                                    const unsigned* __restrict__ mm, double* __restrict__ slots, unsigned long long* __restrict__ sse)
{
    typedef typename MtVec<V>::T T;
    __shared__ __attribute__((aligned(16))) unsigned rawA[LRF_MT_HR * LRF_MT_PITCH / 4];
    __shared__ __attribute__((aligned(16))) unsigned rawB[LRF_MT_HR * LRF_MT_PITCH / 4];
    __shared__ __attribute__((aligned(16))) unsigned h1[LRF_MT_HR * LRF_MT_TW]; // row sums of 7: a | b << 16
    __shared__ __attribute__((aligned(16))) unsigned h2[LRF_MT_HR * LRF_MT_TW]; // a^2 + b^2
    __shared__ __attribute__((aligned(16))) unsigned h3[LRF_MT_HR * LRF_MT_TW]; // a b
    __shared__ double red[256];
    __shared__ unsigned s_sse;

    const int tid = threadIdx.x;
    const unsigned nt = (unsigned)(ntx * nty);
    const unsigned plane = blockIdx.x / nt, tile = blockIdx.x - plane * nt; // plane = image * C + channel
    const int ty = (int)(tile / (unsigned)ntx), tx = (int)(tile - (unsigned)ty * (unsigned)ntx);
    const int y0 = ty * LRF_MT_TH, x0 = tx * LRF_MT_TW;
    const long base = (long)plane * H * W;
    if (tid == 0) s_sse = 0;

    // ---- stage the pixels the tile's windows cover; rows and pieces outside the image are zeros (their windows are not counted)
    constexpr int NCH = ((LRF_MT_HC + 3) / 4 * 4 + V - 1) / V; // pieces of V bytes per row: the 72 bytes the next phase reads, or more
    const bool last_row = ty == nty - 1, last_col = tx == ntx - 1;
    unsigned my_sse = 0;
    for (int it = tid; it < LRF_MT_HR * NCH; it += 256) {
        const int r = it / NCH, col = (it - r * NCH) * V;
        const int y = y0 + r, x = x0 + col;
        const bool in = y < H && x + V <= W;
        T va = T(), vb = T();
        if (in) {
            const long off = base + (long)y * W + x;
            va = *reinterpret_cast<const T*>(a + off);
            vb = *reinterpret_cast<const T*>(b + off);
        }
        *reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(rawA) + r * LRF_MT_PITCH + col) = va;
        *reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(rawB) + r * LRF_MT_PITCH + col) = vb;
        // the squared error of a pixel is added by the tile whose 24 x 64 origin block holds it (the last tile row / column:
        // everything down to / right of it as well); V divides 64, so a piece is owned whole or not at all
        if (in && (r < LRF_MT_TH || last_row) && (col < LRF_MT_TW || last_col)) {
            if constexpr (V == 16) my_sse += mt_sse4(va.x, vb.x) + mt_sse4(va.y, vb.y) + mt_sse4(va.z, vb.z) + mt_sse4(va.w, vb.w);
            else my_sse += mt_sse4(va, vb);
        }
    }
    __syncthreads();
    if (my_sse) atomicAdd(&s_sse, my_sse); // <= 30 * 80 * 255^2 per tile: 32 bits

    // ---- sums of 7 along the rows: a thread per (row, 8 window columns) reads 14 + 2 pixels of a and b
    if (tid < LRF_MT_HR * (LRF_MT_TW / 8)) {
        const int r = tid >> 3, s = tid & 7;
        const uint2* pa = reinterpret_cast<const uint2*>(rawA + r * (LRF_MT_PITCH / 4) + 2 * s);
        const uint2* pb = reinterpret_cast<const uint2*>(rawB + r * (LRF_MT_PITCH / 4) + 2 * s);
        const uint2 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
        const unsigned wa[4] = {a0.x, a0.y, a1.x, a1.y}, wb[4] = {b0.x, b0.y, b1.x, b1.y};
        unsigned p[14], q[14], xy[14];
#pragma unroll
        for (int k = 0; k < 14; k++) {
            const unsigned av = mt_byte(wa[k >> 2], k & 3), bv = mt_byte(wb[k >> 2], k & 3);
            p[k] = av | (bv << 16);
            q[k] = __umul24(av, av) + __umul24(bv, bv);
            xy[k] = __umul24(av, bv);
        }
        unsigned o1[8], o2[8], o3[8];
        unsigned s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) { s1 += p[k]; s2 += q[k]; s3 += xy[k]; }
        o1[0] = s1; o2[0] = s2; o3[0] = s3;
#pragma unroll
        for (int i = 1; i < 8; i++) {
            s1 += p[i + 6] - p[i - 1]; // (both halves stay within 16 bits: each is a sum of 7 bytes again)
            s2 += q[i + 6] - q[i - 1];
            s3 += xy[i + 6] - xy[i - 1];
            o1[i] = s1; o2[i] = s2; o3[i] = s3;
        }
        uint4* d1 = reinterpret_cast<uint4*>(h1 + r * LRF_MT_TW + 8 * s);
        uint4* d2 = reinterpret_cast<uint4*>(h2 + r * LRF_MT_TW + 8 * s);
        uint4* d3 = reinterpret_cast<uint4*>(h3 + r * LRF_MT_TW + 8 * s);
        d1[0] = make_uint4(o1[0], o1[1], o1[2], o1[3]); d1[1] = make_uint4(o1[4], o1[5], o1[6], o1[7]);
        d2[0] = make_uint4(o2[0], o2[1], o2[2], o2[3]); d2[1] = make_uint4(o2[4], o2[5], o2[6], o2[7]);
        d3[0] = make_uint4(o3[0], o3[1], o3[2], o3[3]); d3[1] = make_uint4(o3[4], o3[5], o3[6], o3[7]);
    }
    __syncthreads();

    // ---- sliding sum of 7 down a column: thread = (band of 6 rows, column); then S of each window, in float64
    const unsigned vmax = mm[2 * (plane / (unsigned)C)], vmin = 255u - mm[2 * (plane / (unsigned)C) + 1];
    const double L = (double)(vmax - vmin); // data_range of the first image: max - min
    const double c1 = (0.01 * L) * (0.01 * L), c2 = (0.03 * L) * (0.03 * L);
    const int band = tid >> 6, cx = tid & 63;
    const int r0 = band * (LRF_MT_TH / 4);
    const bool col_ok = x0 + cx < W - 6;
    unsigned v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        v1 += h1[(r0 + k) * LRF_MT_TW + cx];
        v2 += h2[(r0 + k) * LRF_MT_TW + cx];
        v3 += h3[(r0 + k) * LRF_MT_TW + cx];
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LRF_MT_TH / 4; j++) {
        v1 += h1[(r0 + j + 6) * LRF_MT_TW + cx];
        v2 += h2[(r0 + j + 6) * LRF_MT_TW + cx];
        v3 += h3[(r0 + j + 6) * LRF_MT_TW + cx];
        const int sx = (int)(v1 & 0xffffu), sy = (int)(v1 >> 16);
        const int P = __mul24(sx, sy), Q = __mul24(sx, sx) + __mul24(sy, sy);
        const int N1 = __mul24(49, (int)v3) - P;     // 49 Sxy - Sx Sy       (Sxy < 2^22)
        const int N2 = __mul24(49, (int)v2) - Q;     // 49 (Sxx + Syy) - Q   (Sxx + Syy < 2^23)
        const double A1 = (double)P * (2.0 / 2401.0) + c1, A2 = (double)N1 * (2.0 / 2352.0) + c2;
        const double B1 = (double)Q * (1.0 / 2401.0) + c1, B2 = (double)N2 * (1.0 / 2352.0) + c2;
        const double S = (A1 * A2) / (B1 * B2);
        acc += (col_ok && y0 + r0 + j < H - 6) ? S : 0.0;
        v1 -= h1[(r0 + j) * LRF_MT_TW + cx];
        v2 -= h2[(r0 + j) * LRF_MT_TW + cx];
        v3 -= h3[(r0 + j) * LRF_MT_TW + cx];
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        slots[blockIdx.x] = red[0];
        if (s_sse) atomicAdd(sse + plane / (unsigned)C, (unsigned long long)s_sse);
    }
}

// grid (B), 256 threads: ssim[b] = mean over the channels of (sum of the channel's slots) / ((H-6)(W-6))
__global__ __launch_bounds__(256) void k_ssim_final(const double* __restrict__ slots, int C, int nt, double npix, double* __restrict__ ssim)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int ch = 0; ch < C; ch++) {
        const double* sl = slots + ((long)blockIdx.x * C + ch) * nt;
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
    if (tid == 0) ssim[blockIdx.x] = total / (double)C;
}
