// lrf_decode_scaled_kernel.hip — compressed images at 1/2, 1/4, 1/8 scale straight from their factors
// (lrf_qmf_decode_scaled_rgb_u8, lrf_qmf_decode_scaled_crops_rgb_u8; host side: lrf_decode_scaled_host.inc, launch plan:
// plan_decode_scaled in lrf_plan.cpp).  Output pixel (i, j) at scale f is the decoder's image before its colour conversion,
// averaged over image rows f i .. min(f i + f, H) - 1 and the columns likewise, then converted: per plane the block's integers
// are summed exactly in int32 (at most 64 pixels x 64 ranks x 2^14: 2^26), m = float(S) / float(n) is one conversion and one
// IEEE division, and the colour chain is decode_colour of lrf_kernels.hip.  A luma patch is u . V^T, so the sum over a block
// of it is u . (the sum of those V rows): the pooling moves from the pixels onto a table per image.
//
//   items[blockIdx.x / wgs] -> (image, f, y0, x0, h, w, out_off, pool_off): a window of the scaled image; sorted by launch
//   descs[image]            -> the image's geometry, ranks and the offsets of its factors (RaggedDesc; rgb_off unused)
//
// Both are uniform over the workgroup, as in lrf_decode_crops_kernel.hip.  The grid is nitems x wgs in grid.x, wgs the most an
// item of the launch needs; which pixels a thread answers for is scaled_tile_of / scaled_pixel_of (lrf_plan.h), the functions
// tests/test_decode_scaled_plan.py enumerates on the CPU.
//
//   k_pool_v                       per (image, f) of the tiled items: the pooled tables as int16 sums, luma [R_Y][(8/f)^2] (f x f
//                                  entries of V each), Cb and Cr [R_c][(16/f)^2] (f/2 x f/2 entries each: V itself at f = 2)
//   k_decode_scaled_tiled<F, CLS>  images whose sides are multiples of 16 (no padding, chroma row = y >> 1, a block never
//                                  straddles a patch), one instantiation per scale and rank-bound class of the tiled decoders
//   k_decode_scaled_any            every geometry and rank: a thread one output pixel (scaled_pixel_rgb)
//   k_decode_scaled_tiled_t<F, CLS, T>, k_decode_scaled_any_t<T>   the same two writing a model's tensor instead of bytes
//                                  (lrf_qmf_decode_scaled_crops_tensor; the epilogue: lrf_decode_tensor_kernel.hip)

__global__ __launch_bounds__(256) void k_pool_v(const int8_t* __restrict__ V, int16_t* __restrict__ pool, const RaggedDesc* __restrict__ descs,
                                                const ScaledPoolJob* __restrict__ jobs)
{
    const ScaledPoolJob job = jobs[blockIdx.x];
    const RaggedDesc& d = descs[job.image];
    const int8_t* Vc = V + d.v_off;
    int16_t* out = pool + job.pool_off;
    const int Rc[3] = {d.R0, d.R1, d.R2};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int fp = c ? job.f / 2 : job.f, np = 8 / fp, R = Rc[c]; // the pool's side and the pooled entries per patch side
        const int n = R * np * np;
        for (int e = threadIdx.x; e < n; e += 256) {
            const int r = e / (np * np), q = e - r * np * np, a = q / np, b = q - a * np;
            int s = 0; // at most 64 entries of int8: 2^13
            for (int dy = 0; dy < fp; dy++)
                for (int dx = 0; dx < fp; dx++) s += Vc[((a * fp + dy) * 8 + b * fp + dx) * R + r];
            out[e] = (int16_t)s;
        }
        out += n;
        Vc += 64 * R;
    }
}

// byte r of an int8 row held as dwords
__device__ __forceinline__ int scaled_u_at(const unsigned* w, int r) { return (int)(int8_t)(w[r >> 2] >> (8 * (r & 3))); }

// NC pixels of row oy of the scaled image from column ox into a tensor, ch[j][k] their colours before the clamp; `whole`: the
// window holds them all, else those of columns xlo .. xhi - 1.  All three channels are packed first: NHWC stores them interleaved.
template <int NC, class T>
__device__ __forceinline__ void scaled_store_row(const DecodeTensorOut<T>& out, const ScaledItem& it, long hw, int oy, int ox, bool whole, int xlo, int xhi,
                                                 const float (&ch)[NC][3])
{
    unsigned pk[3][NC == 8 ? 2 : 1];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if constexpr (NC == 8) {
            pk[k][0] = decode16_pack4(ch[0][k], ch[1][k], ch[2][k], ch[3][k]);
            pk[k][1] = decode16_pack4(ch[4][k], ch[5][k], ch[6][k], ch[7][k]);
        } else if constexpr (NC == 4)
            pk[k][0] = decode16_pack4(ch[0][k], ch[1][k], ch[2][k], ch[3][k]);
        else
            pk[k][0] = decode16_pack4(ch[0][k], ch[1][k], 0.f, 0.f);
    }
    const int r = oy - it.y0;
    if (whole)
        out.template run<NC>(it.out_off, hw, it.w, r, ox - it.x0, pk);
    else {
#pragma unroll
        for (int j = 0; j < NC; j++)
            if (ox + j >= xlo && ox + j < xhi) {
                const int sh = 8 * (j & 3);
                const unsigned v[3] = {(pk[0][j >> 2] >> sh) & 255u, (pk[1][j >> 2] >> sh) & 255u, (pk[2][j >> 2] >> sh) & 255u};
                out.one(it.out_off, hw, it.w, r, ox + j - it.x0, v);
            }
    }
}

// A thread owns one chroma patch: 16 x 16 image pixels = NC x NC output pixels, the four luma patches (2 pr + a, 2 pc + b) and one
// row of U per chroma plane.  The u rows are loaded as decode16_tile loads them (unaligned dwords, issued before the tables are
// staged); the pooled tables sit in LDS as int32 [r][q], rows past the plane's rank zero, and every lane reads the same entry
// at the same time (a broadcast).  Output rows orow and orow + NL of the patch read the same luma entries — from the upper and
// the lower luma patches — so an entry read serves four patches.  A row's NC bytes leave as one piece (8, 4, 2 bytes at
// f = 2, 4, 8) where the window holds them all, byte-wise at its edges.
template <int F, int CLS>
__global__ __launch_bounds__(256) void k_decode_scaled_tiled(const int8_t* __restrict__ U, const int16_t* __restrict__ pool, uint8_t* __restrict__ rgb,
                                                             const RaggedDesc* __restrict__ descs, const ScaledItem* __restrict__ items, int wgs)
{
    constexpr int RL = CLS == 4 ? 32 : (CLS >= 2 ? 16 : 8), RC = CLS >= 3 ? 16 : (CLS >= 1 ? 8 : 4);
    constexpr int NL = 8 / F, NC = 16 / F, QL = NL * NL, QC = NC * NC;
    __shared__ __attribute__((aligned(16))) int TL[RL * QL], TC[2 * RC * QC];
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const ScaledItem it = items[ii];
    if (wg >= scaled_tiled_wgs(F, it.y0, it.x0, it.h, it.w)) return; // (uniform: before the barrier)
    const RaggedDesc& d = descs[it.image];
    const ScaledTile t = scaled_tile_of(F, it.y0, it.x0, it.h, it.w, wg, (int)threadIdx.x);
    const int R0 = d.R0, R1 = d.R1, R2 = d.R2, nwl = d.g.p[0].nw, nwc = d.g.p[1].nw;
    const int8_t* Ul = U + d.u_off;
    const int8_t* Ub = Ul + (long)d.g.p[0].M * R0;
    const int8_t* Ur = Ub + (long)d.g.p[1].M * R1;
    unsigned wl[4][RL / 4], wb[RC / 4], wr[RC / 4];
#pragma unroll
    for (int p = 0; p < 4; p++) decode_u_load<RL>(Ul + ((long)(2 * t.pr + (p >> 1)) * nwl + 2 * t.pc + (p & 1)) * R0, R0, wl[p]);
    decode_u_load<RC>(Ub + ((long)t.pr * nwc + t.pc) * R1, R1, wb);
    decode_u_load<RC>(Ur + ((long)t.pr * nwc + t.pc) * R2, R2, wr);
    const int16_t* pY = pool + it.pool_off;
    const int16_t* pCb = pY + R0 * QL;
    const int16_t* pCr = pCb + R1 * QC;
    for (int e = threadIdx.x; e < RL * QL; e += 256) TL[e] = e < R0 * QL ? (int)pY[e] : 0;
    for (int e = threadIdx.x; e < RC * QC; e += 256) {
        TC[e] = e < R1 * QC ? (int)pCb[e] : 0;
        TC[RC * QC + e] = e < R2 * QC ? (int)pCr[e] : 0;
    }
    __syncthreads();
    if (t.px.ny == 0) return;
    const long hw = (long)it.h * it.w;
    const int ox = t.pc * NC;
    const bool whole = t.px.nx == NC;
    constexpr float inv = 1.f / (float)(F * F); // n = f^2 in the interior: the division is an exact scaling
    // one output row of the patch per step: row orow of the upper (half = 0) or lower luma patches.  The row loop stays a loop:
    // unrolled, the compiler keeps every table entry of the patch in registers (209 to 512 of them, scratch at the large classes)
#pragma unroll
    for (int half = 0; half < 2; half++) {
#pragma unroll 1
        for (int orow = 0; orow < NL; orow++) {
            const int oy = t.pr * NC + orow + half * NL;
            if (oy < t.px.y || oy >= t.px.y + t.px.ny) continue;
            int Y[2][NL], C[2][NC];
#pragma unroll
            for (int j = 0; j < NL; j++) Y[0][j] = Y[1][j] = 0;
#pragma unroll
            for (int j = 0; j < NC; j++) C[0][j] = C[1][j] = 0;
#pragma unroll
            for (int r = 0; r < RL; r++)
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int tv = TL[r * QL + orow * NL + j];
                    Y[0][j] += scaled_u_at(wl[2 * half], r) * tv;
                    Y[1][j] += scaled_u_at(wl[2 * half + 1], r) * tv;
                }
#pragma unroll
            for (int r = 0; r < RC; r++)
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    C[0][j] += scaled_u_at(wb, r) * TC[r * QC + (orow + half * NL) * NC + j];
                    C[1][j] += scaled_u_at(wr, r) * TC[(RC + r) * QC + (orow + half * NL) * NC + j];
                }
            float ch[NC][3];
#pragma unroll
            for (int j = 0; j < NC; j++) {
                // a chroma sample lies under 2 x 2 image pixels: the block's sum counts it four times
                const float c0 = (float)Y[j >= NL ? 1 : 0][j % NL] * inv;
                const float c1 = (float)(4 * C[0][j]) * inv + -128.f, c2 = (float)(4 * C[1][j]) * inv + -128.f;
                decode_colour(c0, c1, c2, ch[j]);
            }
            uint8_t* row = rgb + it.out_off + (long)(oy - it.y0) * it.w - it.x0; // column x of the scaled image at row[x]
#pragma unroll
            for (int k = 0; k < 3; k++) {
                unsigned pk[NC == 8 ? 2 : 1];
                if constexpr (NC == 8) {
                    pk[0] = decode16_pack4(ch[0][k], ch[1][k], ch[2][k], ch[3][k]);
                    pk[1] = decode16_pack4(ch[4][k], ch[5][k], ch[6][k], ch[7][k]);
                } else if constexpr (NC == 4)
                    pk[0] = decode16_pack4(ch[0][k], ch[1][k], ch[2][k], ch[3][k]);
                else
                    pk[0] = decode16_pack4(ch[0][k], ch[1][k], 0.f, 0.f);
                uint8_t* dst = row + k * hw;
                if (whole) {
                    if constexpr (NC == 8) *reinterpret_cast<uint2 __attribute__((aligned(1)))*>(dst + ox) = make_uint2(pk[0], pk[1]);
                    else if constexpr (NC == 4) *reinterpret_cast<uint32_t __attribute__((aligned(1)))*>(dst + ox) = pk[0];
                    else *reinterpret_cast<uint16_t __attribute__((aligned(1)))*>(dst + ox) = (uint16_t)pk[0];
                } else {
#pragma unroll
                    for (int j = 0; j < NC; j++)
                        if (ox + j >= t.px.x && ox + j < t.px.x + t.px.nx) dst[ox + j] = (uint8_t)(pk[j >> 2] >> (8 * (j & 3)));
                }
            }
        }
    }
}

// k_decode_scaled_tiled_t is the same kernel for a tensor (lrf_decode_tensor_kernel.hip; it.out_off counts elements): the body up to
// the colours is repeated, not shared.  Shared through an inlined function the compiler allocated k_decode_scaled_tiled<8, 4>
// 127 VGPRs instead of 86 (4 waves per SIMD instead of 5) with the same text, so the byte kernel stays as it was written.
template <int F, int CLS, class T>
__global__ __launch_bounds__(256) void k_decode_scaled_tiled_t(const int8_t* __restrict__ U, const int16_t* __restrict__ pool, T* __restrict__ tensor, TensorFmt fmt,
                                                               const RaggedDesc* __restrict__ descs, const ScaledItem* __restrict__ items, int wgs)
{
    constexpr int RL = CLS == 4 ? 32 : (CLS >= 2 ? 16 : 8), RC = CLS >= 3 ? 16 : (CLS >= 1 ? 8 : 4);
    constexpr int NL = 8 / F, NC = 16 / F, QL = NL * NL, QC = NC * NC;
    __shared__ __attribute__((aligned(16))) int TL[RL * QL], TC[2 * RC * QC];
    const DecodeTensorOut<T> out{tensor, fmt};
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const ScaledItem it = items[ii];
    if (wg >= scaled_tiled_wgs(F, it.y0, it.x0, it.h, it.w)) return; // (uniform: before the barrier)
    const RaggedDesc& d = descs[it.image];
    const ScaledTile t = scaled_tile_of(F, it.y0, it.x0, it.h, it.w, wg, (int)threadIdx.x);
    const int R0 = d.R0, R1 = d.R1, R2 = d.R2, nwl = d.g.p[0].nw, nwc = d.g.p[1].nw;
    const int8_t* Ul = U + d.u_off;
    const int8_t* Ub = Ul + (long)d.g.p[0].M * R0;
    const int8_t* Ur = Ub + (long)d.g.p[1].M * R1;
    unsigned wl[4][RL / 4], wb[RC / 4], wr[RC / 4];
#pragma unroll
    for (int p = 0; p < 4; p++) decode_u_load<RL>(Ul + ((long)(2 * t.pr + (p >> 1)) * nwl + 2 * t.pc + (p & 1)) * R0, R0, wl[p]);
    decode_u_load<RC>(Ub + ((long)t.pr * nwc + t.pc) * R1, R1, wb);
    decode_u_load<RC>(Ur + ((long)t.pr * nwc + t.pc) * R2, R2, wr);
    const int16_t* pY = pool + it.pool_off;
    const int16_t* pCb = pY + R0 * QL;
    const int16_t* pCr = pCb + R1 * QC;
    for (int e = threadIdx.x; e < RL * QL; e += 256) TL[e] = e < R0 * QL ? (int)pY[e] : 0;
    for (int e = threadIdx.x; e < RC * QC; e += 256) {
        TC[e] = e < R1 * QC ? (int)pCb[e] : 0;
        TC[RC * QC + e] = e < R2 * QC ? (int)pCr[e] : 0;
    }
    __syncthreads();
    if (t.px.ny == 0) return;
    const long hw = (long)it.h * it.w;
    const int ox = t.pc * NC;
    const bool whole = t.px.nx == NC;
    constexpr float inv = 1.f / (float)(F * F); // n = f^2 in the interior: the division is an exact scaling
    // one output row of the patch per step: row orow of the upper (half = 0) or lower luma patches.  The row loop stays a loop:
    // unrolled, the compiler keeps every table entry of the patch in registers (209 to 512 of them, scratch at the large classes)
#pragma unroll
    for (int half = 0; half < 2; half++) {
#pragma unroll 1
        for (int orow = 0; orow < NL; orow++) {
            const int oy = t.pr * NC + orow + half * NL;
            if (oy < t.px.y || oy >= t.px.y + t.px.ny) continue;
            int Y[2][NL], C[2][NC];
#pragma unroll
            for (int j = 0; j < NL; j++) Y[0][j] = Y[1][j] = 0;
#pragma unroll
            for (int j = 0; j < NC; j++) C[0][j] = C[1][j] = 0;
#pragma unroll
            for (int r = 0; r < RL; r++)
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int tv = TL[r * QL + orow * NL + j];
                    Y[0][j] += scaled_u_at(wl[2 * half], r) * tv;
                    Y[1][j] += scaled_u_at(wl[2 * half + 1], r) * tv;
                }
#pragma unroll
            for (int r = 0; r < RC; r++)
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    C[0][j] += scaled_u_at(wb, r) * TC[r * QC + (orow + half * NL) * NC + j];
                    C[1][j] += scaled_u_at(wr, r) * TC[(RC + r) * QC + (orow + half * NL) * NC + j];
                }
            float ch[NC][3];
#pragma unroll
            for (int j = 0; j < NC; j++) {
                // a chroma sample lies under 2 x 2 image pixels: the block's sum counts it four times
                const float c0 = (float)Y[j >= NL ? 1 : 0][j % NL] * inv;
                const float c1 = (float)(4 * C[0][j]) * inv + -128.f, c2 = (float)(4 * C[1][j]) * inv + -128.f;
                decode_colour(c0, c1, c2, ch[j]);
            }
            scaled_store_row<NC>(out, it, hw, oy, ox, whole, t.px.x, t.px.x + t.px.nx, ch);
        }
    }
}

// Every geometry and rank, the definition as it stands: the block's luma integers summed patch by patch (u . the sum of the V
// rows the block holds of that patch), its chroma integers through the nearest-neighbour rows and columns with the number of
// block pixels over each (scaled_chroma_run), the true division by the block's pixel count.
// scaled_pixel_rgb: pixel (oy, ox) of image d at scale f as its three bytes, R | G << 8 | B << 16 (k_decode_scaled_any stores them;
// the resized crops of lrf_decode_resized_kernel.hip interpolate between them).
__device__ __forceinline__ unsigned scaled_pixel_rgb(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const RaggedDesc& d, int f, int oy, int ox)
{
    const int ya = scaled_lo(oy, f), yb = scaled_hi(oy, f, d.H), xa = scaled_lo(ox, f), xb = scaled_hi(ox, f, d.W);
    const int8_t *Ui = U + d.u_off, *Vi = V + d.v_off;
    const int8_t* Uc[3] = {Ui, Ui + (long)d.g.p[0].M * d.R0, Ui + (long)d.g.p[0].M * d.R0 + (long)d.g.p[1].M * d.R1};
    const int8_t* Vc[3] = {Vi, Vi + 64 * d.R0, Vi + 64 * d.R0 + 64 * d.R1};
    const int Rc[3] = {d.R0, d.R1, d.R2};
    int S[3] = {0, 0, 0};
    { // luma, padded coordinates
        const PlaneGeom& pg = d.g.p[0];
        const int Ya = ya + pg.top_crop, Yb = yb + pg.top_crop, Xa = xa + pg.left_crop, Xb = xb + pg.left_crop, R = Rc[0];
        for (int py = Ya >> 3; py <= (Yb - 1) >> 3; py++)
            for (int px = Xa >> 3; px <= (Xb - 1) >> 3; px++) {
                const int y0 = Ya > 8 * py ? Ya : 8 * py, y1 = Yb < 8 * py + 8 ? Yb : 8 * py + 8;
                const int x0 = Xa > 8 * px ? Xa : 8 * px, x1 = Xb < 8 * px + 8 ? Xb : 8 * px + 8;
                const int8_t* u = Uc[0] + ((long)py * pg.nw + px) * R;
                for (int r = 0; r < R; r++) {
                    int vs = 0;
                    for (int yy = y0; yy < y1; yy++)
                        for (int xx = x0; xx < x1; xx++) vs += Vc[0][((yy & 7) * 8 + (xx & 7)) * R + r];
                    S[0] += (int)u[r] * vs;
                }
            }
    }
    for (int y = ya; y < yb;) {
        int qy, qx;
        const int my = scaled_chroma_run(y, yb, d.H, d.g.p[1].h, &qy);
        for (int x = xa; x < xb;) {
            const int mx = scaled_chroma_run(x, xb, d.W, d.g.p[1].w, &qx);
#pragma unroll
            for (int c = 1; c < 3; c++) {
                const PlaneGeom& pg = d.g.p[c];
                const int yy = qy + pg.top_crop, xx = qx + pg.left_crop, R = Rc[c];
                const int8_t* u = Uc[c] + ((long)(yy >> 3) * pg.nw + (xx >> 3)) * R;
                const int8_t* v = Vc[c] + ((yy & 7) * 8 + (xx & 7)) * R;
                int acc = 0;
                for (int r = 0; r < R; r++) acc += (int)u[r] * (int)v[r];
                S[c] += my * mx * acc;
            }
            x += mx;
        }
        y += my;
    }
    const float n = (float)((yb - ya) * (xb - xa));
    float ch[3];
    decode_colour(__fdiv_rn((float)S[0], n), __fdiv_rn((float)S[1], n) + -128.f, __fdiv_rn((float)S[2], n) + -128.f, ch);
    unsigned px = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) px |= (unsigned)(uint8_t)__builtin_amdgcn_fmed3f(ch[k], 0.f, 255.f) << (8 * k);
    return px;
}

template <class OUT>
__device__ __forceinline__ void decode_scaled_any_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                     const RaggedDesc* __restrict__ descs, const ScaledItem* __restrict__ items, int wgs)
{
    const int ii = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ii * (unsigned)wgs);
    const ScaledItem it = items[ii];
    const CropSpan o = scaled_pixel_of(it.y0, it.x0, it.h, it.w, wg, (int)threadIdx.x);
    if (o.ny == 0) return;
    const unsigned px = scaled_pixel_rgb(U, V, descs[it.image], it.f, o.y, o.x);
    const unsigned v[3] = {px & 255u, (px >> 8) & 255u, (px >> 16) & 255u};
    out.one(it.out_off, (long)it.h * it.w, it.w, o.y - it.y0, o.x - it.x0, v);
}

__global__ __launch_bounds__(256) void k_decode_scaled_any(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                           const RaggedDesc* __restrict__ descs, const ScaledItem* __restrict__ items, int wgs)
{
    decode_scaled_any_wg(U, V, DecodeU8Out{rgb}, descs, items, wgs);
}
template <class T>
__global__ __launch_bounds__(256) void k_decode_scaled_any_t(const int8_t* __restrict__ U, const int8_t* __restrict__ V, T* __restrict__ out, TensorFmt f,
                                                             const RaggedDesc* __restrict__ descs, const ScaledItem* __restrict__ items, int wgs)
{
    decode_scaled_any_wg(U, V, DecodeTensorOut<T>{out, f}, descs, items, wgs);
}
