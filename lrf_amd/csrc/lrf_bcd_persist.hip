// lrf_bcd_persist.hip — the iterations of a large call of the 64-column path in ONE launch (k_bcd_p<F16, NP32, FIRST>,
// lrf_bcdp_kernel.hip: iterations 2..K, or all K at ranks <= 16): its launch (bcdp_launch: queue state, error word, grid).
// Which calls take it: plan_bcd (lrf_plan.cpp).
// lrf/factorization/qmf.py:93-139, 197-214 (the num_iters loop).
#include "lrf_host.h"
#include "lrf_gs.h"
#include "lrf_bcdw_kernel.hip"
#include "lrf_bcdw16_kernel.hip"
#include "lrf_bcdw32_kernel.hip"
#include "lrf_bcdp_kernel.hip"

template <bool F16, int NP32, bool FIRST = false>
static int bcdp_launch_t(lrf_ctx* c, int attr_bit, int wgs, int wave_lds, const float* X, const PlaneDesc* pl, const BlockDesc* bl, int nblocks,
                         int nplanes, int plane0, const BcdpTabs& t16, const BcdpTabs& t64, int8_t* U, int8_t* V, GsParams gp, int niter,
                         const LumaSrc& ls = LumaSrc{nullptr, 0, 0, 0, 0})
{
    if (!(c->attr_persist & (1u << attr_bit))) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_bcd_p<F16, NP32, FIRST>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_BCDW_WAVES * wave_lds));
        c->attr_persist |= 1u << attr_bit;
    }
    Prof p(c, LRF_K_BCD_PERSIST);
    hipLaunchKernelGGL((k_bcd_p<F16, NP32, FIRST>), dim3((unsigned)wgs), dim3(64 * LRF_BCDW_WAVES), (size_t)LRF_BCDW_WAVES * wave_lds, c->stream, X, pl, bl, t16,
                       t64, U, V, gp, nblocks, niter, nplanes, plane0, (BcdpSync*)c->psync.p, c->h_perr, 2 * nplanes, ++c->pseq, wave_lds, ls);
    LAUNCH_CHECK();
    return LRF_OK;
}

int bcdp_launch(lrf_ctx* c, const BcdPlan& plan, const float* X, const PlaneDesc* pl, const BlockDesc* bl, int nblocks, int nplanes, int plane0,
                const FamBufs& f16, const FamBufs& f64, int8_t* U, int8_t* V, GsParams gp)
{
    const bool first = plan.persist_first; // item iteration 0 is the call's first iteration
    const int niter = first ? plan.K : plan.K - 1;
    if (!plan.persist || (first && plan.persist_np32 != 0)) return set_err(LRF_EINVAL, "internal: no instantiation of k_bcd_p for this plan");
    if (plan.luma_bytes && !first) return set_err(LRF_EINVAL, "internal: luma from the image bytes needs every iteration inside k_bcd_p");
    if (!c->h_perr) {
        HIP_TRY(hipHostMalloc((void**)&c->h_perr, sizeof(int), hipHostMallocDefault));
        *c->h_perr = 0;
    }
    // a failure nobody has looked at yet (the results of the calls it names were never checked): refuse to go on silently
    int rc = ctx_check(c);
    if (rc) return rc;
    const size_t sbytes = sizeof(BcdpSync) + (2 * (size_t)nplanes + (size_t)nblocks) * sizeof(int); // (+ a debug count per block)
    const void* before = c->psync.p;
    if ((rc = ensure(c, c->psync, sbytes))) return rc;
    if (c->psync.p != before || c->psync_dirty) { // a launch leaves the state zeroed (its last wave); a new buffer or a failed launch does not
        HIP_TRY(hipMemsetAsync(c->psync.p, 0, c->psync.cap, c->stream));
        c->psync_dirty = false;
    }
    const long total_waves = (long)niter * nblocks;
    long wgs = (total_waves + LRF_BCDW_WAVES - 1) / LRF_BCDW_WAVES;
    if (wgs > 512) wgs = 512; // two workgroups per CU resident; later ones would only find the queue empty
    // LDS per wave: the largest share a family of the call needs
    int wave_lds = (64 * 64 + 64 * 8) * 4 + LRF_BCDP_USTAGE; // ranks <= 8: X tile, u tile, U-span staging (18.5 KB: 8 waves per CU)
    if (plan.persist_f16 && LRF_BCDW16_WAVE_LDS > wave_lds) wave_lds = LRF_BCDW16_WAVE_LDS;
    const BcdpTabs t16{f16.vf, f16.bf, f16.pp, f16.qp, f16.wf}, t64{f64.vf, f64.bf, f64.pp, f64.qp, f64.wf};
    gp.exact_int = 1;
#define LRF_P(F16, NP, BIT)                                                                                                          \
    return bcdp_launch_t<F16, NP>(c, BIT, (int)wgs, NP ? (LRF_BCDW32_WAVE_LDS(NP) > wave_lds ? LRF_BCDW32_WAVE_LDS(NP) : wave_lds) : wave_lds, X, pl, bl, \
                                  nblocks, nplanes, plane0, t16, t64, U, V, gp, niter)
    if (first) {
        // (the only instantiation with the luma-from-bytes body: plan_luma_bytes asks for this branch; plane 0 of the table is
        // image 0's luma plane there)
        const LumaSrc ls = plan.luma_bytes && plane0 == 0 ? plan.luma : LumaSrc{nullptr, 0, 0, 0, 0};
        if (plan.luma_bytes && ls.nluma == 0) return set_err(LRF_EINVAL, "internal: luma from the image bytes without its source");
        if (!plan.persist_f16) return bcdp_launch_t<false, 0, true>(c, 10, (int)wgs, wave_lds, X, pl, bl, nblocks, nplanes, plane0, t16, t64, U, V, gp, niter, ls);
        if (plan.luma_bytes) return set_err(LRF_EINVAL, "internal: no luma-from-bytes body in this instantiation of k_bcd_p");
        return bcdp_launch_t<true, 0, true>(c, 11, (int)wgs, wave_lds, X, pl, bl, nblocks, nplanes, plane0, t16, t64, U, V, gp, niter);
    }
    if (!plan.persist_f16) LRF_P(false, 0, 0);
    switch (plan.persist_np32) {
    case 0: LRF_P(true, 0, 1);
    case 9: LRF_P(true, 9, 2);
    case 10: LRF_P(true, 10, 3);
    case 11: LRF_P(true, 11, 4);
    case 12: LRF_P(true, 12, 5);
    case 13: LRF_P(true, 13, 6);
    case 14: LRF_P(true, 14, 7);
    case 15: LRF_P(true, 15, 8);
    default: LRF_P(true, 16, 9);
    }
#undef LRF_P
}
