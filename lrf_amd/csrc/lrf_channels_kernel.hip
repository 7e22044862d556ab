// lrf_channels_kernel.hip — qmf_encode / qmf_decode of images with a channel count other than three (host side: lrf_channels.hip;
// the reference: patchify "c (h p) (w q) -> (h w) (c p q)" with c inferred, lrf/compression/qmf.py:43-56, decode :309-323).
//
//   k_gray_planes16   C = 1, 8x8 patches, W % 16 == 0, 16-byte aligned rows: a lane loads 16 pixels of one image row (one
//                     16-byte load) and stores the two patch rows they are (four 16-byte stores).  Lanes are dealt (patch pair,
//                     row in patch), so the eight lanes of a patch pair write its 512 bytes of X back to back.
//   k_gray_planes     any size, any alignment: a lane forms four columns of a patch row from single bytes (reflect padding in
//                     both directions) and stores them as one 16-byte piece.
//   k_gray_decode     C = 1, 8x8 patches: the V table [64][R] sits in LDS once per workgroup, packed four ranks to a dword; a
//                     lane forms the 16 pixels of two rows of one patch as int8 dot products (v_dot4c_i32_i8) in int32, clamps
//                     and stores each row of eight bytes as dwords where the output address allows, byte by byte otherwise
//                     (the crop's edges, odd widths).  No floating point.
//   k_chan_matrix     the general route: X [M, C p q] or the planes [C, H, W] (p = 0), one lane per element.
//   k_chan_decode     its decoder, one lane per pixel, int32 sums.
//
// X holds uint8-valued floats, the sums of the decoders are exact integers: |sum| <= R * 128^2 (LRF_ANY_MAX_RANK: 1.05e7).
#define LRF_GRAY_DEC_MAX_RANK 64 // k_gray_decode: the V table in LDS is 64 x this many bytes

__device__ __forceinline__ int chan_reflect(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

__device__ __forceinline__ float4 chan_f4(unsigned w)
{
    return make_float4((float)(w & 255u), (float)((w >> 8) & 255u), (float)((w >> 16) & 255u), (float)(w >> 24));
}

// The per-item bodies of the two planes kernels: k_gray_planes16 / k_gray_planes run them on a batch of equal images, the ragged
// kernels of lrf_gray_encode_kernel.hip on a list of images of mixed sizes, so that X is the same bits by construction.
// gray_planes16_item: row a of the patch pair j of patch row hh — 16 pixels of one image row (one 16-byte load) as the two patch
// rows they are (four 16-byte stores).  img: the image's [H][W] bytes, 16-byte aligned, W % 16 == 0; o: its X at the pair's row a
__device__ __forceinline__ void gray_planes16_item(const uint8_t* __restrict__ img, int H, int W, int top, int hh, int j, int a, float4* __restrict__ o)
{
    const int y = chan_reflect(hh * 8 + a - top, H);
    const uint4 px = *reinterpret_cast<const uint4*>(img + (long)y * W + j * 16);
    o[0] = chan_f4(px.x);
    o[1] = chan_f4(px.y);
    o[16] = chan_f4(px.z);
    o[17] = chan_f4(px.w);
}
// gray_planes_item: columns b0 .. b0 + 3 of row a of patch (hh, ww) from single bytes, reflect padding in both directions, as one
// 16-byte piece of X
__device__ __forceinline__ void gray_planes_item(const uint8_t* __restrict__ img, int H, int W, int top, int left, int hh, int ww, int a, int b0,
                                                 float4* __restrict__ o)
{
    const uint8_t* row = img + (long)chan_reflect(hh * 8 + a - top, H) * W;
    const int x0 = ww * 8 + b0 - left;
    float4 v;
    v.x = (float)row[chan_reflect(x0, W)];
    v.y = (float)row[chan_reflect(x0 + 1, W)];
    v.z = (float)row[chan_reflect(x0 + 2, W)];
    v.w = (float)row[chan_reflect(x0 + 3, W)];
    *o = v;
}

// grid (ceil(nh * (W / 16) * 8 / 256), B).  Item t = (patch pair, row a in the patch): pair = t / 8 counts the pairs of an
// image in row-major order, which is the order of X (nw = W / 8 is even), so X + pair * 128 + a * 8 are the first patch's eight
// floats and + 64 the second's.
__global__ __launch_bounds__(256) void k_gray_planes16(const uint8_t* __restrict__ gray, int H, int W, int top, long items, float* __restrict__ X)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= items) return;
    const int a = (int)(t & 7);
    const long pair = t >> 3;
    const int nch = W >> 4;
    const int hh = (int)(pair / nch), j = (int)(pair - (long)hh * nch);
    gray_planes16_item(gray + (long)blockIdx.y * H * W, H, W, top, hh, j, a,
                       reinterpret_cast<float4*>(X + (long)blockIdx.y * (items >> 3) * 128 + pair * 128 + a * 8));
}

// grid (ceil(M * 16 / 256), B).  Item e = (patch m, row a, half): four floats of X at m * 64 + a * 8 + half * 4.
__global__ __launch_bounds__(256) void k_gray_planes(const uint8_t* __restrict__ gray, int H, int W, int top, int left, int nw, long items,
                                                     float* __restrict__ X)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= items) return;
    const long m = e >> 4;
    const int a = (int)(e & 15) >> 1, b0 = (int)(e & 1) * 4;
    const int hh = (int)(m / nw), ww = (int)(m - (long)hh * nw);
    gray_planes_item(gray + (long)blockIdx.y * H * W, H, W, top, left, hh, ww, a, b0,
                     reinterpret_cast<float4*>(X + (long)blockIdx.y * (items >> 4) * 64 + e * 4));
}

__device__ __forceinline__ int chan_dot4(unsigned a, unsigned b, int acc)
{
#if __has_builtin(__builtin_amdgcn_sdot4)
    return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false);
#else
    for (int i = 0; i < 4; i++) acc += (int)(int8_t)(a >> (8 * i)) * (int)(int8_t)(b >> (8 * i));
    return acc;
#endif
}

__device__ __forceinline__ unsigned chan_clamp_u8(int v)
{
    return (unsigned)min(max(v, 0), 255);
}

// The pieces of k_gray_decode that the gray loader's kernels (lrf_gray_loader_kernel.hip) run too, so that the arithmetic exists once.
// gray_stage_v: vs[r4][n] = ranks 4 r4 .. 4 r4 + 3 of V[n] as one dword (zero above R), by the whole workgroup of 256 threads; the
// caller places the barrier.
__device__ __forceinline__ void gray_stage_v(const int8_t* __restrict__ Vb, int R, unsigned* __restrict__ vs)
{
    const int r4n = (R + 3) >> 2;
    for (int i = threadIdx.x; i < r4n * 64; i += 256) {
        const int r4 = i >> 6, n = i & 63;
        unsigned w = 0;
        for (int k = 0; k < 4; k++) {
            const int r = r4 * 4 + k;
            if (r < R) w |= (unsigned)(uint8_t)Vb[n * R + r] << (8 * k);
        }
        vs[i] = w;
    }
}
// ranks 4 r4 .. 4 r4 + 3 of the row u of U as one dword (zero above R).  u_words: U's rows can be read as dwords (R % 4 == 0
// and an aligned base)
__device__ __forceinline__ unsigned gray_u_word(const int8_t* __restrict__ u, int r4, int R, int u_words)
{
    if (u_words) return *reinterpret_cast<const unsigned*>(u + r4 * 4);
    unsigned uw = 0;
    for (int k = 0; k < 4; k++) {
        const int r = r4 * 4 + k;
        if (r < R) uw |= (unsigned)(uint8_t)u[r] << (8 * k);
    }
    return uw;
}
// acc[8 row + b]: pixel (2 ap + row, b) of the patch whose row of U is u, as the int32 sum of int8 products (v_dot4c_i32_i8): a
// lane's 16 columns of one r4 are 64 consecutive bytes of vs (four ds_read_b128)
__device__ __forceinline__ void gray_patch_rows(const int8_t* __restrict__ u, int R, int u_words, const unsigned* __restrict__ vs, int ap, int (&acc)[16])
{
    const int r4n = (R + 3) >> 2;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0;
    for (int r4 = 0; r4 < r4n; r4++) {
        const unsigned uw = gray_u_word(u, r4, R, u_words);
        const uint4* vrow = reinterpret_cast<const uint4*>(vs + r4 * 64 + ap * 16);
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const uint4 vv = vrow[g];
            acc[4 * g + 0] = chan_dot4(uw, vv.x, acc[4 * g + 0]);
            acc[4 * g + 1] = chan_dot4(uw, vv.y, acc[4 * g + 1]);
            acc[4 * g + 2] = chan_dot4(uw, vv.z, acc[4 * g + 2]);
            acc[4 * g + 3] = chan_dot4(uw, vv.w, acc[4 * g + 3]);
        }
    }
}
// the eight clamped bytes of one row of gray_patch_rows' sums as two dwords
__device__ __forceinline__ uint2 gray_row_bytes(const int (&acc)[16], int row)
{
    return make_uint2(chan_clamp_u8(acc[8 * row + 0]) | chan_clamp_u8(acc[8 * row + 1]) << 8 | chan_clamp_u8(acc[8 * row + 2]) << 16 |
                          chan_clamp_u8(acc[8 * row + 3]) << 24,
                      chan_clamp_u8(acc[8 * row + 4]) | chan_clamp_u8(acc[8 * row + 5]) << 8 | chan_clamp_u8(acc[8 * row + 6]) << 16 |
                          chan_clamp_u8(acc[8 * row + 7]) << 24);
}

// grid (ceil(M * 4 / 256), B), R <= LRF_GRAY_DEC_MAX_RANK.  Item t = (patch m, row pair ap): rows 2 ap and 2 ap + 1 of patch m
// (gray_stage_v, gray_patch_rows).
__global__ __launch_bounds__(256) void k_gray_decode(const int8_t* __restrict__ U, const int8_t* __restrict__ V, int H, int W, int top, int left,
                                                     int nw, int M, int R, int u_words, uint8_t* __restrict__ gray)
{
    __shared__ __attribute__((aligned(16))) unsigned vs[(LRF_GRAY_DEC_MAX_RANK / 4) * 64];
    gray_stage_v(V + (long)blockIdx.y * 64 * R, R, vs);
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= M * 4) return;
    const int m = t >> 2, ap = t & 3;
    int acc[16];
    gray_patch_rows(U + (long)blockIdx.y * M * R + (long)m * R, R, u_words, vs, ap, acc);
    const int hh = m / nw, ww = m - hh * nw;
    const int x0 = ww * 8 - left;
    uint8_t* out = gray + (long)blockIdx.y * H * W;
#pragma unroll
    for (int row = 0; row < 2; row++) {
        const int y = hh * 8 + 2 * ap + row - top;
        if (y < 0 || y >= H) continue;
        const uint2 px = gray_row_bytes(acc, row);
        const unsigned lo = px.x, hi = px.y;
        uint8_t* o = out + (long)y * W + x0; // formed as an address only: bytes outside [0, W) of the row are not touched
        if (x0 >= 0 && x0 + 8 <= W && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            if ((reinterpret_cast<uintptr_t>(o) & 7) == 0) {
                *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
            } else {
                reinterpret_cast<unsigned*>(o)[0] = lo;
                reinterpret_cast<unsigned*>(o)[1] = hi;
            }
        } else {
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const int x = x0 + b;
                if (x >= 0 && x < W) out[(long)y * W + x] = (uint8_t)((b < 4 ? lo >> (8 * b) : hi >> (8 * (b - 4))) & 255u);
            }
        }
    }
}

// The general route (any C, any patch size or none): X [M, C p q], columns in (c, a, b) order, or the planes themselves
// [C][H][W] for p = 0 (qmf.py:164-171, 193-194).  One lane per element; grid (ceil(elems / 256), B).
__global__ __launch_bounds__(256) void k_chan_matrix(const uint8_t* __restrict__ img8, int C, int H, int W, int p, int q, int top, int left,
                                                     int nw, long elems, float* __restrict__ X)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    const uint8_t* img = img8 + (long)blockIdx.y * C * H * W;
    float v;
    if (p == 0) {
        v = (float)img[e];
    } else {
        const int N = C * p * q;
        const long m = e / N;
        const int n = (int)(e - m * N);
        const int c = n / (p * q), rem = n - c * p * q, a = rem / q, b = rem - a * q;
        const int hh = (int)(m / nw), ww = (int)(m - (long)hh * nw);
        const int y = chan_reflect(hh * p + a - top, H), x = chan_reflect(ww * q + b - left, W);
        v = (float)img[(long)c * H * W + (long)y * W + x];
    }
    X[(long)blockIdx.y * elems + e] = v;
}

// p > 0: U [B][M][R], V [B][C p q][R];  p = 0: U [B][C][H][R], V [B][C][W][R].  One lane per pixel; grid (ceil(C H W / 256), B).
__global__ __launch_bounds__(256) void k_chan_decode(const int8_t* __restrict__ U, const int8_t* __restrict__ V, int C, int H, int W, int p, int q,
                                                     int top, int left, int nw, long u_img, long v_img, int R, uint8_t* __restrict__ out)
{
    const long n = (long)C * H * W;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int c = (int)(e / ((long)H * W));
    const long rem = e - (long)c * H * W;
    const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
    const int8_t *u, *v;
    if (p == 0) {
        u = U + (long)blockIdx.y * u_img + ((long)c * H + y) * R;
        v = V + (long)blockIdx.y * v_img + ((long)c * W + x) * R;
    } else {
        const int yy = y + top, xx = x + left;
        const long m = (long)(yy / p) * nw + (xx / q);
        const int col = c * p * q + (yy % p) * q + (xx % q);
        u = U + (long)blockIdx.y * u_img + m * R;
        v = V + (long)blockIdx.y * v_img + (long)col * R;
    }
    int acc = 0;
    for (int r = 0; r < R; r++) acc += (int)u[r] * (int)v[r];
    out[(long)blockIdx.y * n + e] = (uint8_t)min(max(acc, 0), 255);
}
