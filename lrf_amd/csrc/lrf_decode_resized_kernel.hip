// lrf_decode_resized_kernel.hip — boxes of any size and position resampled to one output size straight from the factors
// (lrf_qmf_decode_resized_crops_rgb_u8; host side: lrf_decode_resized_host.inc, launch plan: plan_decode_resized in lrf_plan.cpp).
// A box is sampled bilinearly from a level L of its image: the uniform decoder's image (f = 1) or the image of
// lrf_qmf_decode_scaled_rgb_u8 at f = 2, 4, 8 (resized_level); the taps and their weights in 1/256 are resized_tap, per axis, and
//   out = ((256 - ty) (256 - tx) L[iy0][ix0] + (256 - ty) tx L[iy0][ix1] + ty (256 - tx) L[iy1][ix0] + ty tx L[iy1][ix1] + 32768) >> 16
// in integers (at most 2^16 x 255 + 2^15: int32).
//
//   items[blockIdx.x / wgs] -> (image, f, y0, x0, hb, wb, flip, place): one box; sorted by launch
//   descs[image]            -> the image's geometry, ranks and the offsets of its factors (RaggedDesc; rgb_off unused)
//
// Both are uniform over the workgroup, as in lrf_decode_crops_kernel.hip.  The grid is nitems x wgs in grid.x, wgs what every box of
// the call needs (they share the output size: no workgroup is idle); which output pixels
// a thread answers for is resized_tile_of / resized_thread_of (staged) and scaled_pixel_of (direct) of lrf_plan.h, the functions
// tests/test_decode_resized_plan.py enumerates on the CPU.
//
//   k_decode_resized<MODE>         staged: a workgroup decodes the level pixels its 16 x 64 output tile reads once into LDS, then
//                                  interpolates from there.  MODE 0: f = 1, ranks <= 8 (decode8_quad, V tables in LDS); 1: f = 1,
//                                  every rank (decode_quad); 2: f = 2, 4, 8 (scaled_pixel_rgb)
//   k_decode_resized_direct<F1>    boxes whose tile footprint does not fit LDS (resized_staged): a thread one output pixel and its
//                                  up to four distinct taps (decode_quad / scaled_pixel_rgb)
// Both are thin kernels over a workgroup function (decode_resized_wg, decode_resized_direct_wg) that takes where the pixels go as a
// type: DecodeU8Out for these, DecodeTensorOut<T> for k_decode_resized_t<MODE, T> and k_decode_resized_direct_t<F1, T>, which write
// a model's tensor (lrf_qmf_decode_resized_crops_tensor; lrf_decode_tensor_kernel.hip) and are otherwise the same kernels.

// The sink of the decode bodies aimed at the LDS tile: level pixel (y, x) lands at [ch][y - fy0][x - fx0], what lies outside
// the footprint is dropped.
struct ResizedLdsSink {
    uint8_t* L; // [3][LRF_RS_FH][LRF_RS_FW], 16-byte aligned
    int fy0, fx0, fh, fw;
    __device__ __forceinline__ void put1(int ch, int y, int x, unsigned v) const
    {
        const int r = y - fy0, c = x - fx0;
        if ((unsigned)r < (unsigned)fh && (unsigned)c < (unsigned)fw) L[(ch * LRF_RS_FH + r) * LRF_RS_FW + c] = (uint8_t)v;
    }
    __device__ __forceinline__ void put4(int ch, int y, int x, unsigned w) const
    {
        const int r = y - fy0, c = x - fx0;
        if ((unsigned)r >= (unsigned)fh) return;
        if (c >= 0 && c + 3 < fw && (c & 3) == 0)
            *reinterpret_cast<uint32_t*>(L + (ch * LRF_RS_FH + r) * LRF_RS_FW + c) = w;
        else
#pragma unroll
            for (int i = 0; i < 4; i++) put1(ch, y, x + i, (w >> (8 * i)) & 255u);
    }
    __device__ __forceinline__ void put8(int y, int x, const uint2 (&pk)[3]) const
    {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            put4(k, y, x, pk[k].x);
            put4(k, y, x + 4, pk[k].y);
        }
    }
    __device__ __forceinline__ void put8u(int y, int x, const uint2 (&pk)[3]) const { put8(y, x, pk); }
};

// one pixel of a decode body kept in a register: R | G << 8 | B << 16
struct ResizedRegSink {
    unsigned px = 0;
    __device__ __forceinline__ void put1(int ch, int, int, unsigned v) { px |= (v & 255u) << (8 * ch); }
};

__device__ __forceinline__ int resized_blend(int ty, int tx, int a, int b, int c, int d)
{
    return ((256 - ty) * ((256 - tx) * a + tx * b) + ty * ((256 - tx) * c + tx * d) + 32768) >> 16;
}

// OUT: where the pixels go, DecodeU8Out or DecodeTensorOut<T> (lrf_decode_tensor_kernel.hip): box `place` is [3][oh][ow] (for a tensor in
// NHWC [oh][ow][3]) at 3 oh ow place elements.
template <int MODE, class OUT>
__device__ __forceinline__ void decode_resized_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                  const RaggedDesc* __restrict__ descs, const ResizedItem* __restrict__ items, int oh, int ow, int wgs)
{
    __shared__ __attribute__((aligned(16))) uint8_t L[3 * LRF_RS_FH * LRF_RS_FW];
    __shared__ float Vs[3][MODE == 0 ? 64 * 8 : 1];
    __shared__ int tapy[LRF_RS_TH][3], tapx[LRF_RS_TW][3]; // (i0, i1) relative to the footprint, t
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const ResizedItem it = items[ii];
    const RaggedDesc& d = descs[it.image];
    const int f = MODE == 2 ? it.f : 1;
    const int Hs = (int)scaled_dim(d.H, f), Ws = (int)scaled_dim(d.W, f);
    const ResizedTile t = resized_tile_of(oh, ow, wg);
    const ResizedSpan sy = resized_span(t.r0, t.r0 + t.nr - 1, oh, it.y0, it.hb, f, Hs);
    const ResizedSpan sx = resized_span(t.c0, t.c0 + t.nc - 1, ow, it.x0, it.wb, f, Ws);
    // Unreachable: plan_decode_resized sends a box here only when resized_span_bound, an upper bound of every tile's span, fits the
    // LDS tile (tests/test_decode_resized_plan.py enumerates both).  The guard keeps a disagreement between plan and kernel from
    // writing past the LDS tile; it is uniform and stands before the barrier.
    if (sy.n > LRF_RS_FH || sx.n > LRF_RS_FW) return;
    const int tid = (int)threadIdx.x;
    // the taps of the tile's rows and columns, once: a 64-bit division each
    if (tid < LRF_RS_TW) {
        if (tid < t.nc) {
            const ResizedTap a = resized_tap(t.c0 + tid, ow, it.x0, it.wb, f, Ws);
            tapx[tid][0] = a.i0 - sx.lo; tapx[tid][1] = a.i1 - sx.lo; tapx[tid][2] = a.t;
        }
    } else if (tid < LRF_RS_TW + LRF_RS_TH) {
        const int r = tid - LRF_RS_TW;
        if (r < t.nr) {
            const ResizedTap a = resized_tap(t.r0 + r, oh, it.y0, it.hb, f, Hs);
            tapy[r][0] = a.i0 - sy.lo; tapy[r][1] = a.i1 - sy.lo; tapy[r][2] = a.t;
        }
    }
    // the footprint: level rows sy.lo .. + sy.n - 1, columns sx.lo .. + sx.n - 1, as bytes [ch][row][column]
    if constexpr (MODE == 2) {
        for (int o = tid; o < sy.n * sx.n; o += 256) {
            const int r = o / sx.n, c = o - r * sx.n;
            const unsigned px = scaled_pixel_rgb(U, V, d, f, sy.lo + r, sx.lo + c);
#pragma unroll
            for (int k = 0; k < 3; k++) L[(k * LRF_RS_FH + r) * LRF_RS_FW + c] = (uint8_t)(px >> (8 * k));
        }
    } else {
        ResizedLdsSink sink{L, sy.lo, sx.lo, sy.n, sx.n};
        const int w4 = (sx.n + 3) >> 2;
        if constexpr (MODE == 0) {
            const int8_t *Ui = U + d.u_off, *Vi = V + d.v_off;
            const int8_t* Uc[3] = {Ui, Ui + (long)d.g.p[0].M * d.R0, Ui + (long)d.g.p[0].M * d.R0 + (long)d.g.p[1].M * d.R1};
            const int8_t* Vc[3] = {Vi, Vi + 64 * d.R0, Vi + 64 * d.R0 + 64 * d.R1};
            const int Rc[3] = {d.R0, d.R1, d.R2};
            decode8_stage_v(Vc, Rc, Vs);
            __syncthreads();
            for (int o = tid; o < sy.n * w4; o += 256) {
                const int r = o / w4, c = (o - r * w4) * 4;
                decode8_quad(Uc, Rc, d.H, d.W, d.g, sy.lo + r, sx.lo + c, sx.lo + sx.n, Vs, sink);
            }
        } else {
            for (int o = tid; o < sy.n * w4; o += 256) {
                const int r = o / w4, c = (o - r * w4) * 4;
                decode_quad(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, sy.lo + r, sx.lo + c, sx.lo + sx.n, sink);
            }
        }
    }
    __syncthreads();
    const ResizedPx p = resized_thread_of(t, tid);
    if (p.n == 0) return;
    const int lr = p.r - t.r0, lc = p.c - t.c0;
    const int ty = tapy[lr][2];
    const uint8_t* row0 = L + tapy[lr][0] * LRF_RS_FW;
    const uint8_t* row1 = L + tapy[lr][1] * LRF_RS_FW;
    unsigned pk[3][1] = {{0u}, {0u}, {0u}}; // byte j: column p.c + j, or (flip) the mirrored order the output holds them in
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j >= p.n) break;
        const int x0 = tapx[lc + j][0], x1 = tapx[lc + j][1], tx = tapx[lc + j][2];
        const int sh = 8 * (it.flip ? 3 - j : j);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int o = k * LRF_RS_FH * LRF_RS_FW;
            pk[k][0] |= (unsigned)resized_blend(ty, tx, row0[o + x0], row0[o + x1], row1[o + x0], row1[o + x1]) << sh;
        }
    }
    const long hw = (long)oh * ow, base = (long)it.place * 3 * hw;
    // four pixels leave as one run (bytes: a dword per channel; a tensor: lrf_decode_tensor_kernel.hip), the tile's last columns one by one;
    // the order under flip is the pixels', whatever an element's size
    if (p.n == 4)
        out.template run<4>(base, hw, ow, p.r, it.flip ? ow - 1 - (p.c + 3) : p.c, pk);
    else {
        for (int j = 0; j < p.n; j++) {
            const int sh = 8 * (it.flip ? 3 - j : j);
            const unsigned v[3] = {(pk[0][0] >> sh) & 255u, (pk[1][0] >> sh) & 255u, (pk[2][0] >> sh) & 255u};
            out.one(base, hw, ow, p.r, resized_out_col(p.c + j, ow, it.flip), v);
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_decode_resized(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                        const RaggedDesc* __restrict__ descs, const ResizedItem* __restrict__ items, int oh, int ow, int wgs)
{
    decode_resized_wg<MODE>(U, V, DecodeU8Out{rgb}, descs, items, oh, ow, wgs);
}
template <int MODE, class T>
__global__ __launch_bounds__(256) void k_decode_resized_t(const int8_t* __restrict__ U, const int8_t* __restrict__ V, T* __restrict__ out, TensorFmt f,
                                                          const RaggedDesc* __restrict__ descs, const ResizedItem* __restrict__ items, int oh, int ow, int wgs)
{
    decode_resized_wg<MODE>(U, V, DecodeTensorOut<T>{out, f}, descs, items, oh, ow, wgs);
}

// Correct rather than fast, like k_decode_crops_any: no sharing between threads.  F1: the launch's level is 1.
template <bool F1, class OUT>
__device__ __forceinline__ void decode_resized_direct_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                         const RaggedDesc* __restrict__ descs, const ResizedItem* __restrict__ items, int oh, int ow, int wgs)
{
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const ResizedItem it = items[ii];
    const CropSpan o = scaled_pixel_of(0, 0, oh, ow, wg, (int)threadIdx.x);
    if (o.ny == 0) return;
    const RaggedDesc& d = descs[it.image];
    const int f = F1 ? 1 : it.f;
    const int Hs = (int)scaled_dim(d.H, f), Ws = (int)scaled_dim(d.W, f);
    const ResizedTap ay = resized_tap(o.y, oh, it.y0, it.hb, f, Hs), ax = resized_tap(o.x, ow, it.x0, it.wb, f, Ws);
    auto level_px = [&](int y, int x) -> unsigned {
        if constexpr (F1) {
            ResizedRegSink s;
            decode_quad(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, y, x, x + 1, s);
            return s.px;
        } else
            return scaled_pixel_rgb(U, V, d, f, y, x);
    };
    const unsigned p00 = level_px(ay.i0, ax.i0);
    const unsigned p01 = ax.i1 != ax.i0 ? level_px(ay.i0, ax.i1) : p00;
    unsigned p10 = p00, p11 = p01;
    if (ay.i1 != ay.i0) {
        p10 = level_px(ay.i1, ax.i0);
        p11 = ax.i1 != ax.i0 ? level_px(ay.i1, ax.i1) : p10;
    }
    const long hw = (long)oh * ow;
    unsigned v[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
        v[k] = (unsigned)resized_blend(ay.t, ax.t, (p00 >> (8 * k)) & 255, (p01 >> (8 * k)) & 255, (p10 >> (8 * k)) & 255, (p11 >> (8 * k)) & 255);
    out.one((long)it.place * 3 * hw, hw, ow, o.y, resized_out_col(o.x, ow, it.flip), v);
}

template <bool F1>
__global__ __launch_bounds__(256) void k_decode_resized_direct(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                               const RaggedDesc* __restrict__ descs, const ResizedItem* __restrict__ items, int oh, int ow,
                                                               int wgs)
{
    decode_resized_direct_wg<F1>(U, V, DecodeU8Out{rgb}, descs, items, oh, ow, wgs);
}
template <bool F1, class T>
__global__ __launch_bounds__(256) void k_decode_resized_direct_t(const int8_t* __restrict__ U, const int8_t* __restrict__ V, T* __restrict__ out, TensorFmt f,
                                                                 const RaggedDesc* __restrict__ descs, const ResizedItem* __restrict__ items, int oh,
                                                                 int ow, int wgs)
{
    decode_resized_direct_wg<F1>(U, V, DecodeTensorOut<T>{out, f}, descs, items, oh, ow, wgs);
}
