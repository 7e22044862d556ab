// lrf_decode_crops_kernel.hip — windows of compressed images straight from their factors (lrf_qmf_decode_crops_rgb_u8; host side:
// lrf_encode8.hip, launch plan: plan_decode_crops in lrf_plan.cpp).  A pixel depends on one row of U per plane and on the three
// V tables, so a window needs the U rows of the patches it touches and nothing else.  The kernels run the decode bodies of
// lrf_kernels.hip — decode_strip_core (what k_decode_strip runs over a whole image), decode8_quad, decode_quad — with the
// sink of the whole-image kernels, DecodeStore, aimed at the crop: its base is moved back by the window's origin, so the body
// stores at IMAGE coordinates (which the chroma sampling needs: min(floor(float(y) * (float(h_c) / float(H))), h_c - 1) is a
// function of the image's row and height, not of the window's) and the byte lands at crop coordinates.
//
//   crops[blockIdx.x / wgs] -> (image, y0, x0, out): the window and the index of its [3][h][w] output; sorted by launch
//   descs[image]            -> the image's geometry, ranks and the offsets of its factors (RaggedDesc; rgb_off unused)
//
// Both are uniform over the workgroup, as in lrf_decode_ragged_kernel.hip.  The grid is ncrops x wgs in grid.x, wgs the worst
// case over the alignments a window of (h, w) can have (crop_tiled_wgs / crop_quad_wgs, lrf_plan.h); which pixels a thread of
// workgroup `wg` of a crop answers for is crop_tile_of / crop_quad_of there — the functions tests/test_decode_crops_plan.py
// enumerates on the CPU.
//
//   k_decode_crops_tiled<CLS>  images of the tiled decoders (DEC_TILE16, DEC_STRIP), one instantiation per rank-bound class:
//                              tiles over the padded luma plane from the 16-row strip and the patch column of the window's origin
//   k_decode8_crops            ranks <= 8 elsewhere: the window's pixel quads
//   k_decode_crops_any         every geometry and rank
// Each is a thin kernel over a workgroup function (decode_crops_tiled_wg, decode8_crops_wg, decode_crops_any_wg) that takes where
// the crop goes as a type: CropBytes for these three, CropTensor<T> for k_decode_crops_tiled_t, k_decode8_crops_t and
// k_decode_crops_any_t, which write the model's tensor (lrf_decode_tensor_kernel.hip) and are otherwise the same kernels.

__device__ __forceinline__ DecodeStore crop_sink(uint8_t* __restrict__ rgb, const CropEntry& e, int h, int w)
{
    const long hw = (long)h * w;
    return DecodeStore{rgb + (long)e.out * 3 * hw - ((long)e.y0 * w + e.x0), hw, w};
}
// the same for a tensor (lrf_decode_tensor_kernel.hip): crop e.out is [3][h][w] or [h][w][3] elements at 3 h w e.out
template <class T>
__device__ __forceinline__ TensorStore<T> crop_sink(T* __restrict__ out, const TensorFmt& f, const CropEntry& e, int h, int w)
{
    const long hw = (long)h * w;
    return TensorStore<T>{out + (long)e.out * 3 * hw - ((long)e.y0 * w + e.x0) * (f.nhwc ? 3 : 1), hw, w, f};
}
// what the kernels below aim at the crop: the bytes (CropBytes) or a tensor (CropTensor<T>)
struct CropBytes {
    uint8_t* __restrict__ rgb;
    __device__ __forceinline__ DecodeStore sink(const CropEntry& e, int h, int w) const { return crop_sink(rgb, e, h, w); }
};
template <class T>
struct CropTensor {
    T* __restrict__ out;
    TensorFmt f;
    __device__ __forceinline__ TensorStore<T> sink(const CropEntry& e, int h, int w) const { return crop_sink(out, f, e, h, w); }
};

template <int CLS, class OUT>
__device__ __forceinline__ void decode_crops_tiled_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                      const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    constexpr int RL = CLS == 4 ? 32 : (CLS >= 2 ? 16 : 8), RC = CLS >= 3 ? 16 : (CLS >= 1 ? 8 : 4);
    __shared__ __attribute__((aligned(16))) float VsL[RL * 64], VsC[2 * RC * 64];
    const int ci = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ci * (unsigned)wgs);
    const CropEntry e = crops[ci];
    const RaggedDesc& d = descs[e.image];
    const int top = d.g.p[0].top_crop, left = d.g.p[0].left_crop;
    if (!crop_tile_wg_live(top, left, e.y0, e.x0, h, w, wg)) return; // (uniform: before the body's barrier)
    const CropTile t = crop_tile_of(top, left, e.y0, e.x0, h, w, wg, (int)threadIdx.x);
    auto sink = out.sink(e, h, w);
    decode_strip_core<RC, RL>(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, t.strip, t.ww, t.rp, t.px.ny > 0 && t.px.nx > 0, t.px.y,
                              t.px.y + t.px.ny, t.px.x, t.px.x + t.px.nx, VsL, VsC, sink);
}

template <class OUT>
__device__ __forceinline__ void decode8_crops_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                 const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    __shared__ float Vs[3][64 * 8];
    const int ci = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ci * (unsigned)wgs);
    const CropEntry e = crops[ci];
    const RaggedDesc& d = descs[e.image];
    const int8_t *Ui = U + d.u_off, *Vi = V + d.v_off;
    const int8_t* Uc[3] = {Ui, Ui + (long)d.g.p[0].M * d.R0, Ui + (long)d.g.p[0].M * d.R0 + (long)d.g.p[1].M * d.R1};
    const int8_t* Vc[3] = {Vi, Vi + 64 * d.R0, Vi + 64 * d.R0 + 64 * d.R1};
    const int Rc[3] = {d.R0, d.R1, d.R2};
    decode8_stage_v(Vc, Rc, Vs);
    __syncthreads();
    const CropSpan q = crop_quad_of(e.y0, e.x0, h, w, wg, (int)threadIdx.x);
    if (q.ny == 0) return;
    auto sink = out.sink(e, h, w);
    decode8_quad(Uc, Rc, d.H, d.W, d.g, q.y, q.x, q.x + q.nx, Vs, sink);
}

template <class OUT>
__device__ __forceinline__ void decode_crops_any_wg(const int8_t* __restrict__ U, const int8_t* __restrict__ V, const OUT& out,
                                                    const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    const int ci = (int)(blockIdx.x / (unsigned)wgs), wg = (int)(blockIdx.x - (unsigned)ci * (unsigned)wgs);
    const CropEntry e = crops[ci];
    const RaggedDesc& d = descs[e.image];
    const CropSpan q = crop_quad_of(e.y0, e.x0, h, w, wg, (int)threadIdx.x);
    if (q.ny == 0) return;
    auto sink = out.sink(e, h, w);
    decode_quad(U + d.u_off, V + d.v_off, d.H, d.W, d.g, d.R0, d.R1, d.R2, q.y, q.x, q.x + q.nx, sink);
}

template <int CLS>
__global__ __launch_bounds__(256) void k_decode_crops_tiled(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                            const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    decode_crops_tiled_wg<CLS>(U, V, CropBytes{rgb}, descs, crops, h, w, wgs);
}
__global__ __launch_bounds__(256) void k_decode8_crops(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                       const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    decode8_crops_wg(U, V, CropBytes{rgb}, descs, crops, h, w, wgs);
}
__global__ __launch_bounds__(256) void k_decode_crops_any(const int8_t* __restrict__ U, const int8_t* __restrict__ V, uint8_t* __restrict__ rgb,
                                                          const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    decode_crops_any_wg(U, V, CropBytes{rgb}, descs, crops, h, w, wgs);
}

// the same three with the tensor sink: T = float, _Float16, __bf16 (lrf_qmf_decode_crops_tensor)
template <int CLS, class T>
__global__ __launch_bounds__(256) void k_decode_crops_tiled_t(const int8_t* __restrict__ U, const int8_t* __restrict__ V, T* __restrict__ out, TensorFmt f,
                                                              const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    decode_crops_tiled_wg<CLS>(U, V, CropTensor<T>{out, f}, descs, crops, h, w, wgs);
}
template <class T>
__global__ __launch_bounds__(256) void k_decode8_crops_t(const int8_t* __restrict__ U, const int8_t* __restrict__ V, T* __restrict__ out, TensorFmt f,
                                                         const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    decode8_crops_wg(U, V, CropTensor<T>{out, f}, descs, crops, h, w, wgs);
}
template <class T>
__global__ __launch_bounds__(256) void k_decode_crops_any_t(const int8_t* __restrict__ U, const int8_t* __restrict__ V, T* __restrict__ out, TensorFmt f,
                                                            const RaggedDesc* __restrict__ descs, const CropEntry* __restrict__ crops, int h, int w, int wgs)
{
    decode_crops_any_wg(U, V, CropTensor<T>{out, f}, descs, crops, h, w, wgs);
}
