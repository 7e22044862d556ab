// lrf_metrics_ragged_kernel.hip — squared error and SSIM of n uint8 image pairs that differ in size (lrf_image_metrics_ragged_u8,
// lrf_qmf_ssim_ragged_rgb_u8; host side: lrf_metrics.hip; the tables: plan_metrics_ragged, lrf_plan.h).  Included behind
// lrf_metrics_kernel.hip, whose tile body (lrf_metrics_tile_body.inc) and device functions do the arithmetic: a pair's numbers have the bits lrf_image_metrics_u8 gives
// for that pair alone.
//
//   k_ragged_metrics_pre<SSE>  one flat read of every range of the span table: SSE = false: max and 255 - min of every DISTINCT
//                              a image (pairs that share one read it once); SSE = true: sum (a-b)^2 per pair.  Integer atomics.
//   k_ragged_ssim_tiles<V>     one workgroup per (pair, channel, tile of 24 x 64 window positions) — k_ssim_tiles' tiling of
//                              (H_i, W_i) — found by a prefix search over the pairs' first workgroups (a uniform search: scalar
//                              loads); lrf_metrics_tile_body.inc for the pairs whose load width is V, one launch per width that occurs
//                              (one set of LDS per kernel); the tile's sum of S goes to the slot of its workgroup, the tile's
//                              squared error by one 64-bit integer atomic to sse[i].
//   k_ragged_ssim_final        one workgroup per pair adds its slots channel by channel (mt_ssim_mean) with the pair's own tile
//                              count and (H-6)(W-6).
// No floating-point atomics; nothing depends on the order of the list or on the other pairs.

// the last entry whose wg0 <= wg (the entries' wg0 ascend from 0)
template <class D>
__device__ __forceinline__ int mt_find(const D* __restrict__ d, int n, unsigned wg)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((unsigned)d[mid].wg0 <= wg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// grid (the spans' workgroups), 256 threads.  SSE = false: mm [n][2] = (max, 255 - min) of span i's bytes of a; SSE = true:
// sse [n] = sum (a-b)^2 over span i.  Both zero before the launch.
template <bool SSE>
__global__ __launch_bounds__(256) void k_ragged_metrics_pre(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                            const MetricsSpanDesc* __restrict__ spans, int n, unsigned* __restrict__ mm,
                                                            unsigned long long* __restrict__ sse)
{
    const int i = mt_find(spans, n, blockIdx.x);
    const MetricsSpanDesc d = spans[i];
    const long lo = (long)(blockIdx.x - (unsigned)d.wg0) * LRF_MT_PRE_BYTES;
    const long hi = min(d.n, lo + (long)LRF_MT_PRE_BYTES);
    const uint8_t* pa = a + d.a_off;
    const uint8_t* pb = SSE ? b + d.b_off : b;
    unsigned mx = 0, mn255 = 0;
    unsigned long long s = 0;
    switch (d.vec) {
    case 16: mt_pre_span<16, SSE>(pa, pb, lo, hi, mx, mn255, s); break;
    case 4: mt_pre_span<4, SSE>(pa, pb, lo, hi, mx, mn255, s); break;
    default: mt_pre_span<1, SSE>(pa, pb, lo, hi, mx, mn255, s); break;
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
            if (s_sse) atomicAdd(sse + i, s_sse);
        } else {
            atomicMax(mm + 2 * i, s_mx);
            atomicMax(mm + 2 * i + 1, s_mn);
        }
    }
}

// grid (the pairs' workgroups), 256 threads, one launch per load width V that occurs in the list: a workgroup whose pair reads
// at another width leaves at once (the launch of that width computes it).  slots: one float64 per workgroup; sse [n] zero before
// the launch; mm: per entry of the source table, as k_ragged_metrics_pre<false> left it.
template <int V>
__global__ __launch_bounds__(256) void k_ragged_ssim_tiles(const uint8_t* __restrict__ a_all, const uint8_t* __restrict__ b_all, int C,
                                                           const MetricsPairDesc* __restrict__ pairs, int n, const unsigned* __restrict__ mm_all,
                                                           double* __restrict__ slots, unsigned long long* __restrict__ sse_all)
{
    typedef typename MtVec<V>::T T;
    LRF_MT_TILE_LDS

    const int tid = threadIdx.x;
    const int i = mt_find(pairs, n, blockIdx.x);
    const MetricsPairDesc d = pairs[i];
    if (d.vec != V) return; // (uniform: the whole workgroup)
    // what lrf_metrics_tile_body.inc reads: the pair's images, its source's min / max and its sse entry; `plane` is the channel
    const uint8_t* __restrict__ a = a_all + d.a_off;
    const uint8_t* __restrict__ b = b_all + d.b_off;
    const unsigned* __restrict__ mm = mm_all + 2 * d.src;
    unsigned long long* __restrict__ sse = sse_all + i;
    const int H = d.H, W = d.W, ntx = d.ntx, nty = d.nt / d.ntx;
    const unsigned local = blockIdx.x - (unsigned)d.wg0;
    const unsigned plane = local / (unsigned)d.nt, tile = local - plane * (unsigned)d.nt;
    const int ty = (int)(tile / (unsigned)ntx), tx = (int)(tile - (unsigned)ty * (unsigned)ntx);
#include "lrf_metrics_tile_body.inc"
}

// grid (n), 256 threads: ssim[i] = mean over the channels of (sum of the channel's slots) / ((H_i-6)(W_i-6))
__global__ __launch_bounds__(256) void k_ragged_ssim_final(const double* __restrict__ slots, int C, const MetricsPairDesc* __restrict__ pairs,
                                                           double* __restrict__ ssim)
{
    const MetricsPairDesc d = pairs[blockIdx.x];
    const double v = mt_ssim_mean(slots + d.wg0, C, d.nt, (double)(d.H - 6) * (double)(d.W - 6));
    if (threadIdx.x == 0) ssim[blockIdx.x] = v;
}
