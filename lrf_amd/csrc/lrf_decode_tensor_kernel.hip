// lrf_decode_tensor_kernel.hip — the epilogue of the decode entries that write a model's tensor instead of bytes
// (lrf_qmf_decode_crops_tensor, lrf_qmf_decode_scaled_crops_tensor, lrf_qmf_decode_resized_crops_tensor; host side:
// lrf_decode_tensor_host.inc).  The byte b a uint8 entry defines for (crop, channel k, row, column) leaves as
//   out = rne_T(fl32(fl32(float(b) * scale[k]) + bias[k]))          (include/lrf_hip.h, lrf_tensor_format)
// two fp32 roundings, never an fma: what torch's b.float().mul(s).add(o).to(T) gives on the CPU.  The value is made where the
// byte already sits in a register — in the sink of the decode bodies (TensorStore, beside DecodeStore) and in the output
// policies of the scaled and resized kernels (DecodeTensorOut, beside DecodeU8Out) — so no uint8 batch exists in between.
//
//   T        float, _Float16 or __bf16: a template parameter of every kernel (the conversion and the store widths follow it)
//   layout   NCHW [3][h][w] or NHWC [h][w][3] per crop: TensorFmt::nhwc, a branch uniform over the launch
//
// Stores: a thread holds runs of 2, 4 or 8 adjacent pixels of a row.  NCHW: a run of a channel is contiguous; NHWC: the three
// channels of the run are (6, 12 or 24 elements).  A crop's base and its row pitch are multiples of the element size and of
// nothing more (w, ow, x0 are arbitrary), so the runs leave as pieces of 16, 8 and 4 bytes typed with the element's alignment,
// as the uint8 sinks type theirs with aligned(1).

#ifndef LRF_DECODE_TENSOR_KERNEL_HIP // (lrf_encode8.hip and lrf_channels.hip both include it: once per unit)
#define LRF_DECODE_TENSOR_KERNEL_HIP
// TensorFmt, the kernels' argument: lrf_internal.h

template <class T>
__device__ __forceinline__ T tensor_value(unsigned b, int k, const TensorFmt& f)
{
    // (selects, not an indexed read of the argument: k is a constant wherever the caller's channel loop is unrolled)
    const float s = k == 0 ? f.scale[0] : (k == 1 ? f.scale[1] : f.scale[2]), o = k == 0 ? f.bias[0] : (k == 1 ? f.bias[1] : f.bias[2]);
    return (T)__fadd_rn(__fmul_rn((float)(b & 255u), s), o); // float -> _Float16 / __bf16: round to nearest even, overflow to inf
}

typedef unsigned tensor_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned tensor_u32x2 __attribute__((ext_vector_type(2)));
template <int A>
struct TensorWords;
template <>
struct TensorWords<2> {
    typedef tensor_u32x4 __attribute__((aligned(2))) x4;
    typedef tensor_u32x2 __attribute__((aligned(2))) x2;
    typedef unsigned __attribute__((aligned(2))) x1;
};
template <>
struct TensorWords<4> {
    typedef tensor_u32x4 __attribute__((aligned(4))) x4;
    typedef tensor_u32x2 __attribute__((aligned(4))) x2;
    typedef unsigned __attribute__((aligned(4))) x1;
};

// NW dwords to p, of which only A-byte alignment is known
template <int A, int NW>
__device__ __forceinline__ void tensor_store_words(void* p, const unsigned (&w)[NW])
{
    typedef TensorWords<A> TW;
    unsigned char* q = (unsigned char*)p;
    constexpr int N4 = NW / 4, REST = NW % 4;
#pragma unroll
    for (int i = 0; i < N4; i++) {
        const tensor_u32x4 v = {w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
        *reinterpret_cast<typename TW::x4*>(q + 16 * i) = v;
    }
    if constexpr (REST >= 2) {
        const tensor_u32x2 v = {w[4 * N4], w[4 * N4 + 1]};
        *reinterpret_cast<typename TW::x2*>(q + 16 * N4) = v;
    }
    if constexpr (REST & 1) *reinterpret_cast<typename TW::x1*>(q + 16 * N4 + 4 * (REST - 1)) = w[NW - 1];
}

// N adjacent elements (N even for the 16-bit types: two of them a dword)
template <class T, int N>
__device__ __forceinline__ void tensor_store_elems(T* dst, const T (&v)[N])
{
    if constexpr (sizeof(T) == 4) {
        unsigned w[N];
#pragma unroll
        for (int i = 0; i < N; i++) w[i] = __builtin_bit_cast(unsigned, v[i]);
        tensor_store_words<4, N>(dst, w);
    } else {
        static_assert(sizeof(T) == 2 && N % 2 == 0, "16-bit elements leave in pairs");
        unsigned w[N / 2];
#pragma unroll
        for (int i = 0; i < N / 2; i++)
            w[i] = (unsigned)__builtin_bit_cast(unsigned short, v[2 * i]) | (unsigned)__builtin_bit_cast(unsigned short, v[2 * i + 1]) << 16;
        tensor_store_words<2, N / 2>(dst, w);
    }
}

// NP adjacent pixels of a row, channel k as the bytes of pk[k] (byte i of dword i / 4: pixel i), to where pixel 0 of the run lies:
// NCHW at px0 + k * hw, NHWC the 3 NP elements from px0
template <class T, int NP>
__device__ __forceinline__ void tensor_store_run(T* px0, long hw, const unsigned (&pk)[3][(NP + 3) / 4], const TensorFmt& f)
{
    if (f.nhwc) {
        T v[3 * NP];
#pragma unroll
        for (int i = 0; i < NP; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) v[3 * i + k] = tensor_value<T>(pk[k][i >> 2] >> (8 * (i & 3)), k, f);
        tensor_store_elems<T, 3 * NP>(px0, v);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            T v[NP];
#pragma unroll
            for (int i = 0; i < NP; i++) v[i] = tensor_value<T>(pk[k][i >> 2] >> (8 * (i & 3)), k, f);
            tensor_store_elems<T, NP>(px0 + k * hw, v);
        }
    }
}

// The sink of the decode bodies (lrf_kernels.hip: put8 / put8u / put4 / put1) for a tensor: DecodeStore's counterpart.  `out` is
// the crop moved back by the window's origin in pixels, so the body's image coordinates index it (lrf_decode_crops_kernel.hip).
template <class T>
struct TensorStore {
    T* out;
    long hw;
    int W;
    TensorFmt f;
    __device__ __forceinline__ T* at(int y, int x) const { return out + ((long)y * W + x) * (f.nhwc ? 3 : 1); }
    __device__ __forceinline__ void put8(int y, int x, const uint2 (&pk)[3]) const
    {
        const unsigned w[3][2] = {{pk[0].x, pk[0].y}, {pk[1].x, pk[1].y}, {pk[2].x, pk[2].y}};
        tensor_store_run<T, 8>(at(y, x), hw, w, f);
    }
    __device__ __forceinline__ void put8u(int y, int x, const uint2 (&pk)[3]) const { put8(y, x, pk); }
    __device__ __forceinline__ void put4(int ch, int y, int x, unsigned w) const
    {
        T* dst = at(y, x);
        T v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = tensor_value<T>(w >> (8 * i), ch, f);
        if (f.nhwc) {
#pragma unroll
            for (int i = 0; i < 4; i++) dst[3 * i + ch] = v[i];
        } else
            tensor_store_elems<T, 4>(dst + (long)ch * hw, v);
    }
    __device__ __forceinline__ void put1(int ch, int y, int x, unsigned v) const { at(y, x)[f.nhwc ? (long)ch : (long)ch * hw] = tensor_value<T>(v, ch, f); }
};

// Where the scaled and the resized kernels leave the pixels they hold in registers.  `base`: the crop's first element ([3][h][w]
// or [h][w][3]) from the output's start, hw = h w, w the crop's width, (r, c) the pixel in the crop.
//   run<NP>   NP = 2, 4, 8 adjacent pixels of row r from column c, channel k as the bytes of pk[k]
//   one       one pixel, v[k] its byte of channel k
struct DecodeU8Out {
    uint8_t* __restrict__ rgb;
    template <int NP>
    __device__ __forceinline__ void run(long base, long hw, int w, int r, int c, const unsigned (&pk)[3][(NP + 3) / 4]) const
    {
        static_assert(NP == 4, "the scaled kernel stores its bytes itself (scaled_store_row): only the resized kernels' dword comes here");
        uint8_t* dst = rgb + base + (long)r * w + c;
#pragma unroll
        for (int k = 0; k < 3; k++) *reinterpret_cast<uint32_t __attribute__((aligned(1)))*>(dst + k * hw) = pk[k][0];
    }
    __device__ __forceinline__ void one(long base, long hw, int w, int r, int c, const unsigned (&v)[3]) const
    {
        uint8_t* dst = rgb + base + (long)r * w + c;
#pragma unroll
        for (int k = 0; k < 3; k++) dst[k * hw] = (uint8_t)v[k];
    }
};

template <class T>
struct DecodeTensorOut {
    T* __restrict__ out;
    TensorFmt f;
    template <int NP>
    __device__ __forceinline__ void run(long base, long hw, int w, int r, int c, const unsigned (&pk)[3][(NP + 3) / 4]) const
    {
        tensor_store_run<T, NP>(out + base + ((long)r * w + c) * (f.nhwc ? 3 : 1), hw, pk, f);
    }
    __device__ __forceinline__ void one(long base, long hw, int w, int r, int c, const unsigned (&v)[3]) const
    {
        T* dst = out + base + ((long)r * w + c) * (f.nhwc ? 3 : 1);
        const long step = f.nhwc ? 1 : hw;
#pragma unroll
        for (int k = 0; k < 3; k++) dst[k * step] = tensor_value<T>(v[k], k, f);
    }
};
#endif
