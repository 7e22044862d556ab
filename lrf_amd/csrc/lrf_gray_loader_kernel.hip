// lrf_gray_loader_kernel.hip — the resident-factor loader for gray images (lrf_qmf_decode_gray_ragged_u8,
// lrf_qmf_decode_gray_crops_u8, lrf_qmf_decode_gray_resized_crops_u8 and the _tensor forms; host side: lrf_gray_loader_host.inc,
// launch plans: plan_gray_windows / plan_gray_resized in lrf_plan.cpp).  Exact integers throughout (include/lrf_hip.h): level 1
// is clamp(P, 0, 255) of the plane P = U V^T, level f = 2, 4, 8 is clamp(s, 0, 255 n) / n with s the sum of P over the f x f
// block of IMAGE pixels (n of them: partial at the bottom and right edge) — pooled before the clamp, no floating point.
//
//   items[blockIdx.x / wgs] -> (image, f, y0, x0, h, w, flip, place, out_off, pitch): one window or box; sorted by launch
//   descs[image]            -> the image's size, rank, padding and the offsets of its factors (GrayDesc)
//
// Both are uniform over the workgroup.  The grid is nitems x wgs in grid.x, wgs what the largest item of the launch needs; the
// workgroups an item does not need exit before the barrier.  Every workgroup first loads its image's V table into LDS as
// k_gray_decode does (gray_stage_v: four ranks to a dword, 4 KB at rank 64).
//
//   k_gray_window1    level 1, whole images and windows: k_gray_decode's body (gray_patch_rows: a thread two rows of one patch,
//                     v_dot4c_i32_i8) over the patches the window touches, 64 to a workgroup (gray_tile_of); a row of eight
//                     bytes leaves as 8 / 4-byte pieces where the address allows, byte by byte at the window's edges
//   k_gray_windowf    levels 2, 4, 8: a thread four adjacent level pixels of a row (crop_quad_of), each by gray_level_px
//   k_gray_resized    staged, the structure of k_decode_resized: the taps of the tile's rows and columns once into LDS, the
//                     tile's footprint of level pixels once into LDS as bytes (gray_level_px), one barrier, then the blend; one
//                     channel: a third of the colour tile's LDS
//   k_gray_resized_direct   boxes the staged rule refuses: a thread one output pixel and its up to four taps; correct rather
//                     than fast
// gray_level_px: a block is aligned to the image, not to the padded patch grid, so it straddles up to 2 x 2 patches; per patch
// the lane reads its row of U once per rank quad and adds the dot products of the block's pixels inside that patch.  The final
// division is an integer division: exact for every n.
// Where the pixels go is a type: GrayU8Out for the _u8 entries, GrayTensorOut<T> (tensor_value / tensor_store_elems of
// lrf_decode_tensor_kernel.hip, channel 0) for the _tensor entries, which are otherwise the same kernels.

struct GrayU8Out {
    uint8_t* __restrict__ p;
    __device__ __forceinline__ void put1(long e, unsigned b) const { p[e] = (uint8_t)b; }
    // four / eight adjacent pixels, byte i of the dwords pixel i
    __device__ __forceinline__ void put4(long e, unsigned w) const
    {
        uint8_t* o = p + e;
        if ((reinterpret_cast<uintptr_t>(o) & 3) == 0)
            *reinterpret_cast<unsigned*>(o) = w;
        else
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = (uint8_t)(w >> (8 * i));
    }
    __device__ __forceinline__ void put8(long e, unsigned lo, unsigned hi) const
    {
        uint8_t* o = p + e;
        if ((reinterpret_cast<uintptr_t>(o) & 7) == 0)
            *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
        else {
            put4(e, lo);
            put4(e + 4, hi);
        }
    }
};

template <class T>
struct GrayTensorOut {
    T* __restrict__ p;
    TensorFmt f;
    __device__ __forceinline__ void put1(long e, unsigned b) const { p[e] = tensor_value<T>(b, 0, f); }
    __device__ __forceinline__ void put4(long e, unsigned w) const
    {
        T v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = tensor_value<T>(w >> (8 * i), 0, f);
        tensor_store_elems<T, 4>(p + e, v);
    }
    __device__ __forceinline__ void put8(long e, unsigned lo, unsigned hi) const
    {
        T v[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[i] = tensor_value<T>(lo >> (8 * i), 0, f);
            v[4 + i] = tensor_value<T>(hi >> (8 * i), 0, f);
        }
        tensor_store_elems<T, 8>(p + e, v);
    }
};

// whether the rows of an image's U can be read as dwords
__device__ __forceinline__ int gray_u_words(const int8_t* Ui, int R)
{
    return (R & 3) == 0 && (reinterpret_cast<uintptr_t>(Ui) & 3) == 0;
}

// Pixel (i, j) of level f of the image d (f = 1: the decoder's byte).  Ui: the image's U; vs: its V table (gray_stage_v).
__device__ __forceinline__ unsigned gray_level_px(const int8_t* __restrict__ Ui, const GrayDesc& d, int u_words, const unsigned* __restrict__ vs, int f,
                                                  int i, int j)
{
    const int ya = scaled_lo(i, f), yb = scaled_hi(i, f, d.H), xa = scaled_lo(j, f), xb = scaled_hi(j, f, d.W);
    const int r4n = (d.R + 3) >> 2;
    const int pyb = yb + d.top, pxb = xb + d.left; // the block in padded coordinates
    int s = 0;
    for (int py = ya + d.top; py < pyb;) {
        const int pr = py >> 3, pye = pyb < 8 * pr + 8 ? pyb : 8 * pr + 8;
        for (int px = xa + d.left; px < pxb;) {
            const int pc = px >> 3, pxe = pxb < 8 * pc + 8 ? pxb : 8 * pc + 8;
            const int8_t* u = Ui + (long)(pr * d.nw + pc) * d.R;
            for (int r4 = 0; r4 < r4n; r4++) {
                const unsigned uw = gray_u_word(u, r4, d.R, u_words);
                const unsigned* vr = vs + r4 * 64;
                for (int a = py; a < pye; a++)
                    for (int b = px; b < pxe; b++) s = chan_dot4(uw, vr[(a & 7) * 8 + (b & 7)], s);
            }
            px = pxe;
        }
        py = pye;
    }
    if (f == 1) return chan_clamp_u8(s);
    const int n = (yb - ya) * (xb - xa);
    return (unsigned)min(max(s, 0), 255 * n) / (unsigned)n;
}

template <class OUT>
__device__ __forceinline__ void gray_window1_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                const GrayDesc* __restrict__ descs, const GrayItem* __restrict__ items, int wgs)
{
    __shared__ __attribute__((aligned(16))) unsigned vs[(LRF_GRAY_DEC_MAX_RANK / 4) * 64];
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const GrayItem it = items[ii];
    const GrayDesc d = descs[it.image];
    if (wg >= gray_tile_wgs(d.top, d.left, it.y0, it.x0, it.h, it.w)) return; // (uniform: before the barrier)
    gray_stage_v(V + d.v_off, d.R, vs);
    __syncthreads();
    const GrayTile t = gray_tile_of(d.top, d.left, it.y0, it.x0, it.h, it.w, wg, (int)threadIdx.x);
    if (t.px.ny == 0 || t.px.nx == 0) return;
    const int8_t* Ui = U + d.u_off;
    int acc[16];
    gray_patch_rows(Ui + (long)(t.pr * d.nw + t.pc) * d.R, d.R, gray_u_words(Ui, d.R), vs, t.ap, acc);
    const int xa = 8 * t.pc - d.left;
#pragma unroll
    for (int row = 0; row < 2; row++) {
        const int y = 8 * t.pr + 2 * t.ap + row - d.top;
        if (y < t.px.y || y >= t.px.y + t.px.ny) continue;
        const uint2 b8 = gray_row_bytes(acc, row);
        const long e = it.out_off + (long)(y - it.y0) * it.pitch + (xa - it.x0); // formed as an offset only: pixels outside the window are not touched
        if (t.px.nx == 8)
            out.put8(e, b8.x, b8.y);
        else {
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const int x = xa + b;
                if (x >= t.px.x && x < t.px.x + t.px.nx) out.put1(e + b, ((b < 4 ? b8.x >> (8 * b) : b8.y >> (8 * (b - 4))) & 255u));
            }
        }
    }
}

template <class OUT>
__device__ __forceinline__ void gray_windowf_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                const GrayDesc* __restrict__ descs, const GrayItem* __restrict__ items, int wgs)
{
    __shared__ unsigned vs[(LRF_GRAY_DEC_MAX_RANK / 4) * 64];
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const GrayItem it = items[ii];
    const GrayDesc d = descs[it.image];
    if (wg >= crop_quad_wgs(it.h, it.w)) return; // (uniform: before the barrier)
    gray_stage_v(V + d.v_off, d.R, vs);
    __syncthreads();
    const CropSpan q = crop_quad_of(it.y0, it.x0, it.h, it.w, wg, (int)threadIdx.x);
    if (q.nx == 0) return;
    const int8_t* Ui = U + d.u_off;
    const int u_words = gray_u_words(Ui, d.R);
    unsigned w = 0;
    for (int k = 0; k < q.nx; k++) w |= gray_level_px(Ui, d, u_words, vs, it.f, q.y, q.x + k) << (8 * k);
    const long e = it.out_off + (long)(q.y - it.y0) * it.pitch + (q.x - it.x0);
    if (q.nx == 4)
        out.put4(e, w);
    else
        for (int k = 0; k < q.nx; k++) out.put1(e + k, (w >> (8 * k)) & 255u);
}

// `resized_blend`'s formula (lrf_decode_resized_kernel.hip lives in another unit)
__device__ __forceinline__ int gray_blend(int ty, int tx, int a, int b, int c, int d)
{
    return ((256 - ty) * ((256 - tx) * a + tx * b) + ty * ((256 - tx) * c + tx * d) + 32768) >> 16;
}

template <class OUT>
__device__ __forceinline__ void gray_resized_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                const GrayDesc* __restrict__ descs, const GrayItem* __restrict__ items, int oh, int ow, int wgs)
{
    __shared__ __attribute__((aligned(16))) uint8_t L[LRF_RS_FH * LRF_RS_FW];
    __shared__ unsigned vs[(LRF_GRAY_DEC_MAX_RANK / 4) * 64];
    __shared__ int tapy[LRF_RS_TH][3], tapx[LRF_RS_TW][3]; // (i0, i1) relative to the footprint, t
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const GrayItem it = items[ii];
    const GrayDesc d = descs[it.image];
    const int f = it.f;
    const int Hs = (int)scaled_dim(d.H, f), Ws = (int)scaled_dim(d.W, f);
    const ResizedTile t = resized_tile_of(oh, ow, wg);
    const ResizedSpan sy = resized_span(t.r0, t.r0 + t.nr - 1, oh, it.y0, it.h, f, Hs);
    const ResizedSpan sx = resized_span(t.c0, t.c0 + t.nc - 1, ow, it.x0, it.w, f, Ws);
    // Unreachable: plan_gray_resized sends a box here only when resized_span_bound, an upper bound of every tile's span, fits the
    // LDS tile.  The guard keeps a disagreement between plan and kernel from writing past the LDS tile; it is uniform and stands
    // before the barriers.
    if (sy.n > LRF_RS_FH || sx.n > LRF_RS_FW) return;
    const int tid = (int)threadIdx.x;
    if (tid < LRF_RS_TW) {
        if (tid < t.nc) {
            const ResizedTap a = resized_tap(t.c0 + tid, ow, it.x0, it.w, f, Ws);
            tapx[tid][0] = a.i0 - sx.lo; tapx[tid][1] = a.i1 - sx.lo; tapx[tid][2] = a.t;
        }
    } else if (tid < LRF_RS_TW + LRF_RS_TH) {
        const int r = tid - LRF_RS_TW;
        if (r < t.nr) {
            const ResizedTap a = resized_tap(t.r0 + r, oh, it.y0, it.h, f, Hs);
            tapy[r][0] = a.i0 - sy.lo; tapy[r][1] = a.i1 - sy.lo; tapy[r][2] = a.t;
        }
    }
    gray_stage_v(V + d.v_off, d.R, vs);
    __syncthreads();
    // the footprint: level rows sy.lo .. + sy.n - 1, columns sx.lo .. + sx.n - 1, as bytes [row][column]
    const int8_t* Ui = U + d.u_off;
    const int u_words = gray_u_words(Ui, d.R);
    for (int o = tid; o < sy.n * sx.n; o += 256) {
        const int r = o / sx.n, c = o - r * sx.n;
        L[r * LRF_RS_FW + c] = (uint8_t)gray_level_px(Ui, d, u_words, vs, f, sy.lo + r, sx.lo + c);
    }
    __syncthreads();
    const ResizedPx p = resized_thread_of(t, tid);
    if (p.n == 0) return;
    const int lr = p.r - t.r0, lc = p.c - t.c0;
    const int ty = tapy[lr][2];
    const uint8_t* row0 = L + tapy[lr][0] * LRF_RS_FW;
    const uint8_t* row1 = L + tapy[lr][1] * LRF_RS_FW;
    unsigned pk = 0; // byte j: column p.c + j, or (flip) the mirrored order the output holds them in
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j >= p.n) break;
        const int x0 = tapx[lc + j][0], x1 = tapx[lc + j][1], tx = tapx[lc + j][2];
        pk |= (unsigned)gray_blend(ty, tx, row0[x0], row0[x1], row1[x0], row1[x1]) << (8 * (it.flip ? 3 - j : j));
    }
    const long e = it.out_off + (long)p.r * it.pitch;
    if (p.n == 4)
        out.put4(e + (it.flip ? ow - 1 - (p.c + 3) : p.c), pk);
    else
        for (int j = 0; j < p.n; j++) out.put1(e + resized_out_col(p.c + j, ow, it.flip), (pk >> (8 * (it.flip ? 3 - j : j))) & 255u);
}

template <class OUT>
__device__ __forceinline__ void gray_resized_direct_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                       const GrayDesc* __restrict__ descs, const GrayItem* __restrict__ items, int oh, int ow, int wgs)
{
    __shared__ unsigned vs[(LRF_GRAY_DEC_MAX_RANK / 4) * 64];
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const GrayItem it = items[ii];
    const GrayDesc d = descs[it.image];
    gray_stage_v(V + d.v_off, d.R, vs);
    __syncthreads();
    const CropSpan o = scaled_pixel_of(0, 0, oh, ow, wg, (int)threadIdx.x);
    if (o.ny == 0) return;
    const int f = it.f;
    const int Hs = (int)scaled_dim(d.H, f), Ws = (int)scaled_dim(d.W, f);
    const ResizedTap ay = resized_tap(o.y, oh, it.y0, it.h, f, Hs), ax = resized_tap(o.x, ow, it.x0, it.w, f, Ws);
    const int8_t* Ui = U + d.u_off;
    const int u_words = gray_u_words(Ui, d.R);
    const unsigned p00 = gray_level_px(Ui, d, u_words, vs, f, ay.i0, ax.i0);
    const unsigned p01 = ax.i1 != ax.i0 ? gray_level_px(Ui, d, u_words, vs, f, ay.i0, ax.i1) : p00;
    unsigned p10 = p00, p11 = p01;
    if (ay.i1 != ay.i0) {
        p10 = gray_level_px(Ui, d, u_words, vs, f, ay.i1, ax.i0);
        p11 = ax.i1 != ax.i0 ? gray_level_px(Ui, d, u_words, vs, f, ay.i1, ax.i1) : p10;
    }
    out.put1(it.out_off + (long)o.y * it.pitch + resized_out_col(o.x, ow, it.flip), (unsigned)gray_blend(ay.t, ax.t, (int)p00, (int)p01, (int)p10, (int)p11));
}

#define LRF_GRAY_KERNEL_ARGS const int8_t *__restrict__ U, const int8_t *__restrict__ V
__global__ __launch_bounds__(256) void k_gray_window1(LRF_GRAY_KERNEL_ARGS, uint8_t* __restrict__ out, const GrayDesc* __restrict__ descs,
                                                      const GrayItem* __restrict__ items, int wgs)
{
    gray_window1_wg(U, V, GrayU8Out{out}, descs, items, wgs);
}
template <class T>
__global__ __launch_bounds__(256) void k_gray_window1_t(LRF_GRAY_KERNEL_ARGS, T* __restrict__ out, TensorFmt f, const GrayDesc* __restrict__ descs,
                                                        const GrayItem* __restrict__ items, int wgs)
{
    gray_window1_wg(U, V, GrayTensorOut<T>{out, f}, descs, items, wgs);
}
__global__ __launch_bounds__(256) void k_gray_windowf(LRF_GRAY_KERNEL_ARGS, uint8_t* __restrict__ out, const GrayDesc* __restrict__ descs,
                                                      const GrayItem* __restrict__ items, int wgs)
{
    gray_windowf_wg(U, V, GrayU8Out{out}, descs, items, wgs);
}
template <class T>
__global__ __launch_bounds__(256) void k_gray_windowf_t(LRF_GRAY_KERNEL_ARGS, T* __restrict__ out, TensorFmt f, const GrayDesc* __restrict__ descs,
                                                        const GrayItem* __restrict__ items, int wgs)
{
    gray_windowf_wg(U, V, GrayTensorOut<T>{out, f}, descs, items, wgs);
}
__global__ __launch_bounds__(256) void k_gray_resized(LRF_GRAY_KERNEL_ARGS, uint8_t* __restrict__ out, const GrayDesc* __restrict__ descs,
                                                      const GrayItem* __restrict__ items, int oh, int ow, int wgs)
{
    gray_resized_wg(U, V, GrayU8Out{out}, descs, items, oh, ow, wgs);
}
template <class T>
__global__ __launch_bounds__(256) void k_gray_resized_t(LRF_GRAY_KERNEL_ARGS, T* __restrict__ out, TensorFmt f, const GrayDesc* __restrict__ descs,
                                                        const GrayItem* __restrict__ items, int oh, int ow, int wgs)
{
    gray_resized_wg(U, V, GrayTensorOut<T>{out, f}, descs, items, oh, ow, wgs);
}
__global__ __launch_bounds__(256) void k_gray_resized_direct(LRF_GRAY_KERNEL_ARGS, uint8_t* __restrict__ out, const GrayDesc* __restrict__ descs,
                                                             const GrayItem* __restrict__ items, int oh, int ow, int wgs)
{
    gray_resized_direct_wg(U, V, GrayU8Out{out}, descs, items, oh, ow, wgs);
}
template <class T>
__global__ __launch_bounds__(256) void k_gray_resized_direct_t(LRF_GRAY_KERNEL_ARGS, T* __restrict__ out, TensorFmt f,
                                                               const GrayDesc* __restrict__ descs, const GrayItem* __restrict__ items, int oh, int ow,
                                                               int wgs)
{
    gray_resized_direct_wg(U, V, GrayTensorOut<T>{out, f}, descs, items, oh, ow, wgs);
}
#undef LRF_GRAY_KERNEL_ARGS
