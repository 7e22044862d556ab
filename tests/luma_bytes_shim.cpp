// Test-only C entries for tests/test_luma_bytes_plan.py: the row -> patch mapping of k_bcd_p's luma-from-bytes body
// (luma_byte_off, lrf_amd/csrc/lrf_plan.h) and the decision which calls take it (plan_luma_bytes, lrf_plan.cpp).  Built with the
// host compiler, no device.
#include <math.h>

#include "../lrf_amd/csrc/lrf_plan.h"

// off[ch][m][n] = luma_byte_off(m, n, ch, H W, W, W / 8) for every element of the luma matrix of an H x W image
extern "C" void lrf_test_luma_offsets(int H, int W, int* off)
{
    const int M = (H / 8) * (W / 8), nwl = W / 8;
    for (int ch = 0; ch < 3; ch++)
        for (int m = 0; m < M; m++)
            for (int n = 0; n < 64; n++) off[((long)ch * M + m) * 64 + n] = luma_byte_off(m, n, ch, H * W, W, nwl);
}

// the fp32 formula of ycc_of(r, g, b, 0) (lrf_device.h) on the bytes at those offsets: the luma matrix [M][64]
extern "C" void lrf_test_luma_from_bytes(const unsigned char* img, int H, int W, float* out)
{
    const int M = (H / 8) * (W / 8), nwl = W / 8, hw = H * W;
    for (int m = 0; m < M; m++)
        for (int n = 0; n < 64; n++) {
            const float r = img[luma_byte_off(m, n, 0, hw, W, nwl)], g = img[luma_byte_off(m, n, 1, hw, W, nwl)], b = img[luma_byte_off(m, n, 2, hw, W, nwl)];
            float acc = 0.f;
            acc = fmaf(0.299f, r, acc);
            acc = fmaf(0.587f, g, acc);
            acc = fmaf(0.114f, b, acc);
            out[(long)m * 64 + n] = 0.f + acc;
        }
}

// plan_bcd on the planes (M, R) with LRF_PERSIST = persist on the validated device, then plan_luma_bytes with the first nluma
// planes as the images' luma planes
extern "C" int lrf_test_plan_luma_bytes(int nplanes, const int* M, const int* R, int K, int first_mode, int persist, int nluma, long H, long W,
                                        unsigned long rgb_addr, int rgb_released, int luma_bytes_setting)
{
    Tables t;
    for (int i = 0; i < nplanes; i++) add_plane(t, 0, 0, 0, 0, 0, M[i], R[i], -1);
    PlanSettings s;
    s.persist = persist;
    s.persist_arch = true;
    s.luma_bytes = luma_bytes_setting;
    const BcdPlan p = plan_bcd(t.planes, K, -16, 15, first_mode, s);
    return plan_luma_bytes(p, t.planes, nluma, H, W, (uintptr_t)rgb_addr, rgb_released != 0, s) ? 1 : 0;
}
