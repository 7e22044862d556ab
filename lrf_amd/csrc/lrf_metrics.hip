// lrf_metrics.hip — lrf_image_metrics_u8: the squared error and the SSIM of B uint8 image pairs on the device, what the R-D sweep
// scores every (image, quality) pair with (the reference: lrf/utils/metrics.py:57-91 on the host, one image at a time).  Kernels
// and arithmetic: lrf_metrics_kernel.hip.  Launch sequence on the context's stream, nothing synchronises:
//   sse only:  memset sse, k_metrics_pre<., true>
//   with ssim: memset sse and the min / max words, k_metrics_pre<., false> (reads a), k_ssim_tiles (reads a and b once, writes a
//              float64 slot per tile and adds the tiles' squared errors), k_ssim_final (adds the slots of an image in order)
#include "lrf_host.h"
#include "lrf_metrics_kernel.hip"

// widest piece (16, 4 or 1 bytes) every row / image of `unit` bytes can be read in from both pointers
static int metrics_vec(const uint8_t* a, const uint8_t* b, long unit)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | (uintptr_t)unit;
    return (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1);
}

extern "C" int lrf_image_metrics_u8(lrf_ctx* c, const uint8_t* a, const uint8_t* b, int B, int C, int H, int W, uint64_t* sse, double* ssim)
{
    if (!c || !a || !b || !sse) return set_err(LRF_EINVAL, "NULL argument");
    if (B < 1 || B > 65535 || C < 1 || H < 1 || W < 1) return set_err(LRF_EINVAL, "B=%d C=%d H=%d W=%d out of range", B, C, H, W);
    if (ssim && (H < 7 || W < 7)) return set_err(LRF_EINVAL, "win_size exceeds image extent (%dx%d, window 7x7)", H, W);
    const long n = (long)C * H * W;
    if (n >= (1L << 40)) return set_err(LRF_EINVAL, "image of %ld samples too large", n);
    LRF_ON_DEVICE(c);
    unsigned long long* d_sse = reinterpret_cast<unsigned long long*>(sse);
    const dim3 pre_grid((unsigned)((n + LRF_MT_PRE_BYTES - 1) / LRF_MT_PRE_BYTES), (unsigned)B);
    if (!ssim) {
        Prof p(c, LRF_K_METRICS);
        HIP_TRY(hipMemsetAsync(sse, 0, (size_t)B * sizeof(uint64_t), c->stream));
        switch (metrics_vec(a, b, n)) {
        case 16: hipLaunchKernelGGL((k_metrics_pre<16, true>), pre_grid, dim3(256), 0, c->stream, a, b, n, (unsigned*)nullptr, d_sse); break;
        case 4: hipLaunchKernelGGL((k_metrics_pre<4, true>), pre_grid, dim3(256), 0, c->stream, a, b, n, (unsigned*)nullptr, d_sse); break;
        default: hipLaunchKernelGGL((k_metrics_pre<1, true>), pre_grid, dim3(256), 0, c->stream, a, b, n, (unsigned*)nullptr, d_sse); break;
        }
        LAUNCH_CHECK();
        return LRF_OK;
    }
    const int ntx = (W - 6 + LRF_MT_TW - 1) / LRF_MT_TW, nty = (H - 6 + LRF_MT_TH - 1) / LRF_MT_TH;
    const long nt = (long)ntx * nty, nslots = (long)B * C * nt;
    if (nslots >= (1L << 31)) return set_err(LRF_EINVAL, "%ld tiles in one call: split the batch", nslots);
    // workspace: the slots, then (max, 255 - min) per image
    int rc;
    if ((rc = ensure(c, c->metrics, (size_t)nslots * sizeof(double) + (size_t)B * 2 * sizeof(unsigned)))) return rc;
    double* slots = (double*)c->metrics.p;
    unsigned* mm = (unsigned*)(slots + nslots);
    Prof p(c, LRF_K_METRICS);
    HIP_TRY(hipMemsetAsync(sse, 0, (size_t)B * sizeof(uint64_t), c->stream));
    HIP_TRY(hipMemsetAsync(mm, 0, (size_t)B * 2 * sizeof(unsigned), c->stream));
    switch (metrics_vec(a, a, n)) {
    case 16: hipLaunchKernelGGL((k_metrics_pre<16, false>), pre_grid, dim3(256), 0, c->stream, a, (const uint8_t*)nullptr, n, mm, d_sse); break;
    case 4: hipLaunchKernelGGL((k_metrics_pre<4, false>), pre_grid, dim3(256), 0, c->stream, a, (const uint8_t*)nullptr, n, mm, d_sse); break;
    default: hipLaunchKernelGGL((k_metrics_pre<1, false>), pre_grid, dim3(256), 0, c->stream, a, (const uint8_t*)nullptr, n, mm, d_sse); break;
    }
    LAUNCH_CHECK();
    const dim3 grid((unsigned)nslots);
    switch (metrics_vec(a, b, W)) {
    case 16: hipLaunchKernelGGL((k_ssim_tiles<16>), grid, dim3(256), 0, c->stream, a, b, C, H, W, ntx, nty, (const unsigned*)mm, slots, d_sse); break;
    case 4: hipLaunchKernelGGL((k_ssim_tiles<4>), grid, dim3(256), 0, c->stream, a, b, C, H, W, ntx, nty, (const unsigned*)mm, slots, d_sse); break;
    default: hipLaunchKernelGGL((k_ssim_tiles<1>), grid, dim3(256), 0, c->stream, a, b, C, H, W, ntx, nty, (const unsigned*)mm, slots, d_sse); break;
    }
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ssim_final, dim3((unsigned)B), dim3(256), 0, c->stream, (const double*)slots, C, (int)nt, (double)(H - 6) * (double)(W - 6), ssim);
    LAUNCH_CHECK();
    return LRF_OK;
}
