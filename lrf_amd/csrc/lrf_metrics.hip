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

// ---- pairs that differ in size (kernels: lrf_metrics_ragged_kernel.hip; the tables: plan_metrics_ragged) -------------------------
// Launch sequence on the context's stream, nothing synchronises: the table (pairs, then spans) through the pinned slots of the
// crop table, memset sse, then
//   sse only:  k_ragged_metrics_pre<true> over the pairs
//   with ssim: memset the min / max words, k_ragged_metrics_pre<false> over the distinct a images, k_ragged_ssim_tiles<V> per
//              load width V that occurs (at most three), k_ragged_ssim_final
#include "lrf_metrics_ragged_kernel.hip"
static_assert(LRF_MTR_TH == LRF_MT_TH && LRF_MTR_TW == LRF_MT_TW && LRF_MTR_PRE_BYTES == LRF_MT_PRE_BYTES, "plan_metrics_ragged tiles as the kernels do");
static_assert(sizeof(MetricsPairDesc) == 48 && sizeof(MetricsSpanDesc) == 32, "no padding bytes");

int refuse_metrics(const MetricsRefusal& r)
{
    const long i = (long)r.pair;
    switch (r.check) {
    case MTR_N: return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)r.a);
    case MTR_C: return set_err(LRF_EINVAL, "C=%ld out of range [1,65535]", (long)r.a);
    case MTR_SIZE: return set_err(LRF_EINVAL, "pair %ld: size %ldx%ld out of range (the 7x7 window needs sides >= 7)", i, (long)r.a, (long)r.b);
    case MTR_NEGATIVE: return set_err(LRF_EINVAL, "pair %ld: negative offset", i);
    case MTR_A: return set_err(LRF_EINVAL, "pair %ld: its a image leaves the buffer of %ld bytes", i, (long)r.a);
    case MTR_B: return set_err(LRF_EINVAL, "pair %ld: its b image leaves the buffer of %ld bytes", i, (long)r.a);
    default: return set_err(LRF_EINVAL, "%ld workgroups in one launch: split the list", (long)r.a);
    }
}

size_t metrics_ragged_workspace(const MetricsRaggedPlan& p) { return (size_t)p.tile_wgs * sizeof(double) + p.spans.size() * 2 * sizeof(unsigned); }

// the launches of an accepted plan; the caller holds the device and the timer
int metrics_ragged_launch(lrf_ctx* c, const MetricsRaggedPlan& p, int C, const uint8_t* a, const uint8_t* b, uint64_t* sse, double* ssim)
{
    const int n = (int)p.pairs.size(), ns = (int)p.spans.size();
    int rc;
    if (ssim && (rc = ensure(c, c->metrics, metrics_ragged_workspace(p)))) return rc;
    const size_t pb = (size_t)n * sizeof(MetricsPairDesc), sb = (size_t)ns * sizeof(MetricsSpanDesc);
    std::vector<char> tab(pb + sb);
    memcpy(tab.data(), p.pairs.data(), pb);
    memcpy(tab.data() + pb, p.spans.data(), sb);
    if ((rc = stage_crop_bytes(c, tab.data(), tab.size()))) return rc;
    const MetricsPairDesc* d_pairs = (const MetricsPairDesc*)c->crop_tab.p;
    const MetricsSpanDesc* d_spans = (const MetricsSpanDesc*)((const char*)c->crop_tab.p + pb);
    unsigned long long* d_sse = reinterpret_cast<unsigned long long*>(sse);
    HIP_TRY(hipMemsetAsync(sse, 0, (size_t)n * sizeof(uint64_t), c->stream));
    if (!ssim) {
        hipLaunchKernelGGL((k_ragged_metrics_pre<true>), dim3((unsigned)p.span_wgs), dim3(256), 0, c->stream, a, b, d_spans, ns, (unsigned*)nullptr, d_sse);
        LAUNCH_CHECK();
        return LRF_OK;
    }
    double* slots = (double*)c->metrics.p;
    unsigned* mm = (unsigned*)(slots + p.tile_wgs);
    HIP_TRY(hipMemsetAsync(mm, 0, (size_t)ns * 2 * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL((k_ragged_metrics_pre<false>), dim3((unsigned)p.span_wgs), dim3(256), 0, c->stream, a, (const uint8_t*)nullptr, d_spans, ns, mm, d_sse);
    LAUNCH_CHECK();
    bool w16 = false, w4 = false, w1 = false; // the load widths that occur: one launch each
    for (const MetricsPairDesc& d : p.pairs) (d.vec == 16 ? w16 : (d.vec == 4 ? w4 : w1)) = true;
    const dim3 grid((unsigned)p.tile_wgs);
    if (w16) hipLaunchKernelGGL((k_ragged_ssim_tiles<16>), grid, dim3(256), 0, c->stream, a, b, C, d_pairs, n, (const unsigned*)mm, slots, d_sse);
    if (w4) hipLaunchKernelGGL((k_ragged_ssim_tiles<4>), grid, dim3(256), 0, c->stream, a, b, C, d_pairs, n, (const unsigned*)mm, slots, d_sse);
    if (w1) hipLaunchKernelGGL((k_ragged_ssim_tiles<1>), grid, dim3(256), 0, c->stream, a, b, C, d_pairs, n, (const unsigned*)mm, slots, d_sse);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ragged_ssim_final, dim3((unsigned)n), dim3(256), 0, c->stream, (const double*)slots, C, d_pairs, ssim);
    LAUNCH_CHECK();
    return LRF_OK;
}

extern "C" int lrf_image_metrics_ragged_u8(lrf_ctx* c, int64_t n, const lrf_image_pair* pairs, int C, const uint8_t* a, int64_t a_len, const uint8_t* b,
                                           int64_t b_len, uint64_t* sse, double* ssim)
{
    if (!c || !pairs || !a || !b || !sse) return set_err(LRF_EINVAL, "NULL argument");
    const MetricsCall k = {C, a_len, b_len, reinterpret_cast<uintptr_t>(a), reinterpret_cast<uintptr_t>(b), ssim != nullptr};
    const MetricsRaggedPlan p = plan_metrics_ragged(n, pairs, k);
    if (p.refusal.check != MTR_OK) return refuse_metrics(p.refusal);
    LRF_ON_DEVICE(c);
    Prof prof(c, LRF_K_METRICS);
    return metrics_ragged_launch(c, p, C, a, b, sse, ssim);
}
