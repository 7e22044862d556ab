// lrf_encode8.hip — the 64-column path of liblrf_hip.so (8x8 patches; the default branch of qmf_encode / qmf_decode): its
// kernels and their launch sequences — patch matrices, exact Gram matrix, SVD initialisation, the BCD iterations by rank
// family, decode — and the C ABI entry points built on them (include/lrf_hip.h).
#include "lrf_host.h"
#include "lrf_gram_kernels.hip"
#include "lrf_kernels.hip"
#include "lrf_bcdw_kernel.hip"
#include "lrf_bcdw16_kernel.hip"
#include "lrf_sweep_sse_kernel.hip"
#include "lrf_decode_ragged_kernel.hip"
#include "lrf_sse_ragged_kernel.hip"
#include "lrf_decode_tensor_kernel.hip"
#include "lrf_decode_crops_kernel.hip"
#include "lrf_decode_scaled_kernel.hip"
#include "lrf_decode_resized_kernel.hip"
#include "lrf_planes_ragged_kernel.hip"

// gram_exp: the fixed-point grid exponent of the exact Gram matrix (max|x| < 2^gram_exp) when the caller knows it — 8 for the
// planes of qmf_encode — or LRF_GRAM_EXP_FROM_DATA: one more pass over X finds it per matrix
static int run_init(lrf_ctx* c, const float* X, const Tables& t, const BcdPlan& plan, const int8_t* sign_dev, int gram_exp)
{
    if (!(c->attr_done & (1u << 0))) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_init<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitLds<8>)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_init<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitLds<16>)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_init<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitLds<32>)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_init<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitLds<64>)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_init<16, 8, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitLds<16>)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_init<32, 8, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitLds<32>)));
        HIP_TRY(hipFuncSetAttribute((const void*)k_init<64, 8, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitLds<64>)));
        c->attr_done |= 1u << 0;
    }
    const int nplanes = (int)t.planes.size();
    {
        Prof p(c, LRF_K_GRAM);
        if (gram_exp == LRF_GRAM_EXP_FROM_DATA) {
            hipLaunchKernelGGL(k_gram_exponent, dim3(nplanes), dim3(256), 0, c->stream, X, (const PlaneDesc*)c->planes.p, (int*)c->gexp.p);
            LAUNCH_CHECK();
        }
        // (t.ngram_rest: all chunks, or — behind k_planes16_gram, which has written the luma planes' partials itself — the chroma ones)
        if (t.ngram_rest != (int)t.gchunks.size() && gram_exp != LRF_PLANES_GRAM_EXP)
            return set_err(LRF_EINVAL, "internal: fused Gram partials exist only for the planes of qmf_encode");
        if (t.ngram_rest > 0) {
            if (gram_exp == LRF_PLANES_GRAM_EXP)
                hipLaunchKernelGGL(k_gram64<true>, dim3((unsigned)t.ngram_rest), dim3(256), 0, c->stream, X, (const PlaneDesc*)c->planes.p,
                                   (const GramChunk*)c->gchunks.p, (const int*)c->gexp.p, gram_exp, (ulonglong2*)c->gpart.p);
            else
                hipLaunchKernelGGL(k_gram64<false>, dim3((unsigned)t.ngram_rest), dim3(256), 0, c->stream, X, (const PlaneDesc*)c->planes.p,
                                   (const GramChunk*)c->gchunks.p, (const int*)c->gexp.p, gram_exp, (ulonglong2*)c->gpart.p);
            LAUNCH_CHECK();
        }
    }
    Prof p(c, LRF_K_INIT);
    const std::vector<FamRun>& runs = plan.runs;
    const bool mixed = plan.mixed;
    // A call whose iterations run in the persistent kernel keeps one stream — except here (FAM_STREAMS_INIT): the initialisation
    // kernels of its families are per-matrix latency chains that leave most of a CU idle (k_init<16> 190 us for 256 luma planes,
    // k_init<8> 180 us for 512 chroma planes, one round of workgroups each), and LDS admits one workgroup of the first beside two
    // of the second: forked for this stage only, the later runs (chroma: more, smaller workgroups) enqueued first, joined at once.
    // (The order of the enqueues does not show in the step time — measured both ways at five rank triples — because the
    // streams' queues place their workgroups side by side either way.)  Since round 5's LDS layout (InitLds) a ZR = 32 workgroup
    // has two ZR = 16 ones beside it as well ((26,13,13): the stage 484 -> ~340 us).
    const bool init_only_fork = plan.streams == FAM_STREAMS_INIT;
    int rcf = fam_fork_streams(c, plan.streams, runs.size());
    if (rcf) return rcf;
    long ninit = 0;
    for (const FamRun& r : runs) ninit += r.nbase;
    const bool dense = ninit > 256; // more initialisation workgroups than CUs (k_init's DENSE)
    for (size_t rj = 0; rj < runs.size(); rj++) {
        const size_t ri = init_only_fork ? runs.size() - 1 - rj : rj;
        const FamRun& r = runs[ri];
        hipStream_t rs = run_stream(c, ri);
        const FamBufs fb = run_bufs(c, r, mixed);
        if (r.nbase == 0) continue; // (a sweep call: every plane of this run takes its columns from a plane of another run)
#define LRF_LAUNCH_INIT(ZR, ...)                                                                                     \
    hipLaunchKernelGGL((k_init<ZR, ##__VA_ARGS__>), dim3(r.nbase), dim3(ZR > 8 ? 512 : 256), sizeof(InitLds<ZR>), rs, (const ulonglong2*)c->gpart.p, \
                       (const int*)c->gexp.p, gram_exp, (const PlaneDesc*)c->planes.p, sign_dev, fb.vf, fb.wf, c->init_sweeps, r.pitch, r.plane0)
        if (r.rmax <= 8) LRF_LAUNCH_INIT(8);
        else if (dense) {
            if (r.rmax <= 16) LRF_LAUNCH_INIT(16);
            else if (r.rmax <= 32) LRF_LAUNCH_INIT(32);
            else LRF_LAUNCH_INIT(64);
        } else { // (no more matrices than CUs: the eight-wave workgroups without spills, k_init<.., 8, false>)
            if (r.rmax <= 16) LRF_LAUNCH_INIT(16, 8, false);
            else if (r.rmax <= 32) LRF_LAUNCH_INIT(32, 8, false);
            else LRF_LAUNCH_INIT(64, 8, false);
        }
#undef LRF_LAUNCH_INIT
        LAUNCH_CHECK();
    }
    if (init_only_fork) {
        int rcj = fam_join_streams(c, runs.size());
        if (rcj) return rcj;
    }
    bool shares = false;
    for (const FamRun& r : runs) shares = shares || r.nbase != r.nplanes;
    if (shares) { // a sweep call (its plan keeps one stream): the other ranks' planes take their columns from the base planes
        if (c->fam_forked) return set_err(LRF_EINVAL, "internal: a call that shares initialisations between planes must not fork its families");
        hipLaunchKernelGGL(k_init_share, dim3(nplanes), dim3(256), 0, c->stream, (const PlaneDesc*)c->planes.p, (float*)c->vf.p, (float*)c->wf.p,
                           (float*)c->vf16.p, (float*)c->wf16.p, plan.split ? 1 : 0, mixed ? 1 : 0, plan.rp);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

static GsParams make_gs(int lo, int hi)
{
    GsParams gp;
    gp.lo = (float)lo;
    gp.hi = (float)hi;
    const long mx = bounds_mx(lo, hi);
    gp.flimit = (float)(mx + 2);
    gp.fthr = 0.5f - 8e-7f * (float)(mx + 2); // see gs_row: q~ is within 3 ulp (< 2e-7 |q|) of fl(num/den)
    gp.exact_int = 0; // set per run by run_bcd (FamRun::exact_int)
    return gp;
}

// the iterations of the plan (plan.first_mode: 1 = old U from X @ W0 after run_init, 2 = old U from the caller's fp32 U0)
static int run_bcd(lrf_ctx* c, const float* X, const BcdPlan& plan, const float* U0, int8_t* U, int8_t* V)
{
    const PlaneDesc* pl = (const PlaneDesc*)c->planes.p;
    const BlockDesc* bl = (const BlockDesc*)c->blocks.p;
    const int K = plan.K;
    const GsParams gp = make_gs(plan.lo, plan.hi);
    if (plan.rmax > LRF_BIG_TO_ANY_RANK) return set_err(LRF_ENOTSUP, "internal: ranks above %d iterate on the any-shape kernels", LRF_BIG_TO_ANY_RANK);
    const std::vector<FamRun>& runs = plan.runs;
    const bool mixed = plan.mixed;
    if (!(c->attr_done & (1u << 1))) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_bcd_w<0>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_BCDW_LDS));
        HIP_TRY(hipFuncSetAttribute((const void*)k_bcd_w<1>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_BCDW_LDS));
        HIP_TRY(hipFuncSetAttribute((const void*)k_bcd_w<2>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_BCDW_LDS));
        HIP_TRY(hipFuncSetAttribute((const void*)k_bcd_w16<0>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_BCDW16_LDS));
        HIP_TRY(hipFuncSetAttribute((const void*)k_bcd_w16<1>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_BCDW16_LDS));
        c->attr_done |= 1u << 1;
    }
    // the b tables of the initial V
    for (size_t ri = 0; ri < runs.size(); ri++) {
        const FamRun& r = runs[ri];
        hipStream_t rs = run_stream(c, ri);
        const FamBufs fb = run_bufs(c, r, mixed);
        if (r.pitch == 16) {
            hipLaunchKernelGGL(k_bprep, dim3(r.nplanes), dim3(256), 0, rs, pl, (const float*)fb.vf, fb.bf, r.plane0);
            LAUNCH_CHECK();
        } else {
            int rcb = bcd32_bprep(rs, pl, fb.vf, fb.bf, r.nplanes, r.plane0);
            if (rcb) return rcb;
        }
    }
    for (int it = 0; it < K; it++) {
        if (plan.persist && it == (plan.persist_first ? 0 : 1)) { // the remaining iterations in one launch (lrf_bcd_persist.hip)
            const FamRun& r0 = runs.front();
            long nb = 0, np = 0;
            for (const FamRun& r : runs) { nb += r.nblocks; np += r.nplanes; }
            // the table sets of the two rank pitches (run_bufs): a call without ranks above 16 has only the pitch-16 one
            FamBufs f16{nullptr, nullptr, nullptr, nullptr, nullptr}, f64 = f16;
            for (const FamRun& r : runs) (r.pitch == 16 ? f16 : f64) = run_bufs(c, r, mixed);
            int rcp = bcdp_launch(c, plan, X, pl, bl + r0.block0, (int)nb, (int)np, r0.plane0, f16, f64, U, V, gp);
            if (rcp) return rcp;
            break;
        }
        {
            Prof p(c, LRF_K_BCD);
            const int mode = (it == 0) ? plan.first_mode : 0;
            for (size_t ri = 0; ri < runs.size(); ri++) {
                const FamRun& r = runs[ri];
                hipStream_t rs = run_stream(c, ri);
                const FamBufs fb = run_bufs(c, r, mixed);
                const BlockDesc* blr = bl + r.block0;
                const int nbr = r.nblocks;
                GsParams gpr = gp;
                gpr.exact_int = r.exact_int ? 1 : 0;
                const BcdChoice ch = (it == 0) ? r.first : r.later;
#define LRF_LAUNCH_W(MODE)                                                                                           \
    hipLaunchKernelGGL((k_bcd_w<MODE>), dim3((nbr + LRF_BCDW_WAVES - 1) / LRF_BCDW_WAVES), dim3(64 * LRF_BCDW_WAVES), LRF_BCDW_LDS, rs, X, pl, blr, \
                       (const float*)fb.vf, (const float*)fb.wf, (const float*)fb.bf, U0, U, fb.pp, fb.qp, gpr, nbr)
#define LRF_LAUNCH_WG(MODE, RMAX)                                                                                    \
    hipLaunchKernelGGL((k_bcd<MODE, RMAX>), dim3(nbr), dim3(256), 0, rs, X, pl, blr, (const float*)fb.vf, (const float*)fb.wf, \
                       (const float*)fb.bf, U0, U, fb.pp, fb.qp, gpr)
#define LRF_LAUNCH_W16(MODE)                                                                                         \
    hipLaunchKernelGGL((k_bcd_w16<MODE>), dim3((nbr + LRF_BCDW16_WAVES - 1) / LRF_BCDW16_WAVES), dim3(64 * LRF_BCDW16_WAVES), LRF_BCDW16_LDS, \
                       rs, X, pl, blr, (const float*)fb.vf, (const float*)fb.wf, (const float*)fb.bf, U, fb.pp, fb.qp, gpr, nbr)
#define LRF_BY_MODE(LAUNCH, ...) if (mode == 1) LAUNCH(1, ##__VA_ARGS__); else if (mode == 2) LAUNCH(2, ##__VA_ARGS__); else LAUNCH(0, ##__VA_ARGS__)
                switch (ch.k) {
                case BCD_K_W: LRF_BY_MODE(LRF_LAUNCH_W); break;
                case BCD_K_WG8: LRF_BY_MODE(LRF_LAUNCH_WG, 8); break;
                case BCD_K_WG16: LRF_BY_MODE(LRF_LAUNCH_WG, 16); break;
                case BCD_K_W16: if (mode == 1) LRF_LAUNCH_W16(1); else LRF_LAUNCH_W16(0); break;
                default: { // ranks 17..32 (lrf_bcd32.hip)
                    const BcdLaunch a{X, pl, blr, nbr, fb.vf, fb.wf, fb.bf, U0, U, fb.pp, fb.qp, gpr, mode};
                    int rcu = bcd32_update_u(c, rs, a, ch);
                    if (rcu) return rcu;
                    continue;
                }
                }
#undef LRF_BY_MODE
#undef LRF_LAUNCH_W
#undef LRF_LAUNCH_WG
#undef LRF_LAUNCH_W16
                LAUNCH_CHECK();
            }
        }
        {
            Prof p(c, LRF_K_VUPDATE);
            const int last = it == K - 1 ? 1 : 0;
            for (size_t ri = 0; ri < runs.size(); ri++) {
                const FamRun& r = runs[ri];
                hipStream_t rs = run_stream(c, ri);
                const FamBufs fb = run_bufs(c, r, mixed);
                if (r.fam == 2) {
                    int rcv = bcd32_update_v(c, rs, pl, fb.pp, fb.qp, fb.vf, fb.bf, V, gp.lo, gp.hi, last, r.nplanes, r.plane0);
                    if (rcv) return rcv;
                    continue;
                } else if (r.fam == 0)
                    hipLaunchKernelGGL(k_vupdate<8>, dim3(r.nplanes), dim3(256), 0, rs, pl, (const float*)fb.pp, (const float*)fb.qp,
                                       fb.vf, fb.bf, V, gp, last, r.plane0);
                else
                    hipLaunchKernelGGL(k_vupdate<16>, dim3(r.nplanes), dim3(256), 0, rs, pl, (const float*)fb.pp, (const float*)fb.qp,
                                       fb.vf, fb.bf, V, gp, last, r.plane0);
                LAUNCH_CHECK();
            }
        }
    }
    return fam_join_streams(c, runs.size());
}

// a call that initialises and iterates at once: run_init may leave the families forked for run_bcd to join
static int init_then_bcd(lrf_ctx* c, const float* X, const Tables& t, const BcdPlan& plan, const int8_t* sign, int gram_exp, int8_t* U, int8_t* V)
{
    int rc = run_init(c, X, t, plan, sign, gram_exp);
    if (rc) {
        (void)fam_join_streams(c, 3);
        return rc;
    }
    return run_bcd(c, X, plan, nullptr, U, V);
}
// the same for the entries of other units (lrf_channels.hip: the ragged gray encode)
int init_then_bcd64(lrf_ctx* c, const float* X, const Tables& t, const BcdPlan& plan, const int8_t* sign, int gram_exp, int8_t* U, int8_t* V)
{
    return init_then_bcd(c, X, t, plan, sign, gram_exp, U, V);
}

// ---- C ABI ------------------------------------------------------------------------------------
extern "C" {

int lrf_qmf_planes_from_rgb_u8(lrf_ctx* c, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, float* X)
{
    if (!c || !rgb || !X) return set_err(LRF_EINVAL, "NULL argument");
    if (B < 1 || B > 65535) return set_err(LRF_EINVAL, "B=%ld out of range [1,65535]", (long)B);
    ImageGeom g;
    int rc = make_geom(H, W, &g);
    if (rc) return rc;
    LRF_ON_DEVICE(c);
    Prof p(c, LRF_K_PLANES);
    if ((long)H * W * 3 >= (1L << 31)) return set_err(LRF_ENOTSUP, "image too large for 32-bit pixel indexing");
    static const bool no_tiled = dev_flag("LRF_PLANES_NO_TILED");
    if (H % 16 == 0 && W % 16 == 0 && (reinterpret_cast<uintptr_t>(rgb) & 7) == 0 && !no_tiled)
        hipLaunchKernelGGL(k_planes16, dim3((unsigned)((H / 16) * ((g.p[0].nw + 31) / 32)), (unsigned)B), dim3(256), 0, c->stream, rgb, (int)H,
                           (int)W, g, X);
    else if (!no_tiled) {
        // any other size: the same tiling over the padded planes (k_planes_strip); blocks dealt so that the strips of an image
        // stay on one XCD (block index mod 8 is the XCD when the grid's x extent is a multiple of 8)
        static const bool no_xcd = dev_flag("LRF_PLANES_NO_XCD");
        const int ncols = g.p[0].nw > 2 * g.p[1].nw ? g.p[0].nw : 2 * g.p[1].nw;
        const int per_strip = (ncols + 31) / 32;
        const int nstrips = (g.p[0].nh + 1) / 2 > g.p[1].nh ? (g.p[0].nh + 1) / 2 : g.p[1].nh;
        const int nblk = nstrips * per_strip;
        const int chunk = no_xcd ? 0 : (nblk + 7) / 8;
        const dim3 grid((unsigned)(chunk ? 8 * chunk : nblk), (unsigned)B);
#define LRF_LAUNCH_STRIP(KH, KW) \
    hipLaunchKernelGGL((k_planes_strip<KH, KW>), grid, dim3(256), 0, c->stream, rgb, (int)H, (int)W, g, X, per_strip, nblk, chunk)
        if (H & 1) {
            if (W & 1) LRF_LAUNCH_STRIP(3, 3);
            else LRF_LAUNCH_STRIP(3, 2);
        } else {
            if (W & 1) LRF_LAUNCH_STRIP(2, 3);
            else LRF_LAUNCH_STRIP(2, 2);
        }
#undef LRF_LAUNCH_STRIP
    } else
        hipLaunchKernelGGL(k_planes, dim3((unsigned)(g.p[1].pr0 + g.p[1].nh), (unsigned)B), dim3(256), 0, c->stream, rgb, (int)H,
                           (int)W, g, X);
    LAUNCH_CHECK();
    return LRF_OK;
}

static void uniform_tables(Tables& t, int64_t B, int64_t M, int R, bool with_sign)
{
    for (int64_t b = 0; b < B; b++)
        add_plane(t, b * M * 64, b * M * R, b * 64 * R, b * M * R, b * 64 * R, (int)M, R, with_sign ? (int)(b * R) : -1);
}

// Ranks 33..64 of the 64-column path iterate on the any-shape kernels, which spread the ordered Gauss-Seidel chain over all
// waves (a first rank-64 workgroup kernel with the chain on one wave of four was 2x slower there: (40,20) 20.8 against 11.4 ms
// per 64 images, (64,32) 45.6 against 20.6).  The initialisation stays with k_init, which mirrors the oracle operation for
// operation: k_emit_init writes its factors out as fp32 and the any-shape iteration takes over.

// one class of B equal-shaped 64-column matrices whose initial factors sit contiguously at U0c / V0c
static int any_bcd_from_init(lrf_ctx* c, const float* X, long x_batch, int B, int M, int R, int K, int lo, int hi, const float* U0c,
                             const float* V0c, int8_t* U, long u_batch, int8_t* V, long v_batch)
{
    int rc = any_workspace(c, B, M, 64, R);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->any_uf.p, U0c, (size_t)B * M * R * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->any_vf.p, V0c, (size_t)B * 64 * R * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return any_run_bcd_ex(c, X, x_batch, B, M, 64, R, K, lo, hi, U, u_batch, V, v_batch);
}

// k_init on the uploaded table, then its factors as fp32 into c->any_e2 (U0 at [0], V0 behind it): offsets from the table
static int init_to_fp32(lrf_ctx* c, const float* X, const Tables& t, const BcdPlan& plan, const int8_t* sign, size_t u0_floats, size_t v0_floats, float** U0,
                        float** V0, int gram_exp)
{
    int rc = run_init(c, X, t, plan, sign, gram_exp);
    if (rc) return rc;
    if ((rc = ensure(c, c->any_e2, (u0_floats + v0_floats) * sizeof(float)))) return rc;
    *U0 = (float*)c->any_e2.p;
    *V0 = *U0 + u0_floats;
    hipLaunchKernelGGL(k_emit_init, dim3((unsigned)t.blocks.size()), dim3(256), 0, c->stream, X, (const PlaneDesc*)c->planes.p,
                       (const BlockDesc*)c->blocks.p, (const float*)c->vf.p, (const float*)c->wf.p, *U0, *V0, plan.rp);
    LAUNCH_CHECK();
    return LRF_OK;
}

} // extern "C"

// The 64-column route of lrf_qmf_decompose_f32 (own initialisation, R <= LRF_MAX_RANK) and of lrf_qmf_bcd_f32 (the caller's
// factors, R <= LRF_BIG_TO_ANY_RANK): also what lrf_qmf_encode_gray_u8 (lrf_channels.hip) runs behind its planes kernel, so
// that a gray batch takes the same plan and the same kernels as the same X handed in as floats.
int decompose64(lrf_ctx* c, const float* X, int64_t B, int64_t M, int R, int K, int lo, int hi, const int8_t* sign, int8_t* U, int8_t* V)
{
    int rc = check_params(M, LRF_PATCH_ELEMS, R, K, lo, hi);
    if (rc) return rc;
    if (B < 1) return set_err(LRF_EINVAL, "B must be >= 1");
    LRF_ON_DEVICE(c);
    Tables t;
    uniform_tables(t, B, M, R, sign != nullptr);
    const BcdPlan plan = plan_bcd(t.planes, K, lo, hi, PLAN_FIRST_W0, plan_settings(c));
    if ((rc = upload_tables(c, t, plan))) return rc;
    if (R > LRF_BIG_TO_ANY_RANK) {
        float *U0, *V0;
        if ((rc = init_to_fp32(c, X, t, plan, sign, (size_t)B * M * R, (size_t)B * 64 * R, &U0, &V0, LRF_GRAM_EXP_FROM_DATA))) return rc;
        return any_bcd_from_init(c, X, M * 64, (int)B, (int)M, R, K, lo, hi, U0, V0, U, M * R, V, 64L * R);
    }
    return init_then_bcd(c, X, t, plan, sign, LRF_GRAM_EXP_FROM_DATA, U, V);
}

int bcd64(lrf_ctx* c, const float* X, int64_t B, int64_t M, int R, int K, int lo, int hi, const float* U0, const float* V0, int8_t* U,
          int8_t* V)
{
    int rc = check_params(M, LRF_PATCH_ELEMS, R, K, lo, hi);
    if (rc) return rc;
    if (B < 1) return set_err(LRF_EINVAL, "B must be >= 1");
    LRF_ON_DEVICE(c);
    Tables t;
    uniform_tables(t, B, M, R, false);
    const BcdPlan plan = plan_bcd(t.planes, K, lo, hi, PLAN_FIRST_U0, plan_settings(c));
    if ((rc = upload_tables(c, t, plan))) return rc;
    hipLaunchKernelGGL(k_load_v0, dim3((unsigned)t.planes.size()), dim3(256), 0, c->stream, (const PlaneDesc*)c->planes.p, V0,
                       (float*)c->vf.p, plan.rp);
    LAUNCH_CHECK();
    return run_bcd(c, X, plan, U0, U, V);
}

extern "C" {

int lrf_qmf_decompose_f32(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, int K, int lo, int hi,
                          const int8_t* sign, int8_t* U, int8_t* V)
{
    if (!c || !X || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    static const bool force_any = dev_flag("LRF_FORCE_ANY");
    if (N != LRF_PATCH_ELEMS || R > LRF_MAX_RANK || force_any) return any_decompose(c, X, B, M, N, R, K, lo, hi, sign, U, V);
    return decompose64(c, X, B, M, R, K, lo, hi, sign, U, V);
}

int lrf_qmf_bcd_f32(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, int K, int lo, int hi,
                    const float* U0, const float* V0, int8_t* U, int8_t* V)
{
    if (!c || !X || !U || !V || !U0 || !V0) return set_err(LRF_EINVAL, "NULL argument");
    if (N != LRF_PATCH_ELEMS || R > LRF_BIG_TO_ANY_RANK) return any_bcd(c, X, B, M, N, R, K, lo, hi, U0, V0, U, V);
    return bcd64(c, X, B, M, R, K, lo, hi, U0, V0, U, V);
}

int lrf_qmf_svd_init_f32(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, const int8_t* sign,
                         float* U0, float* V0)
{
    if (!c || !X || !U0 || !V0) return set_err(LRF_EINVAL, "NULL argument");
    if (N != LRF_PATCH_ELEMS || R > LRF_MAX_RANK) return any_svd_init(c, X, B, M, N, R, sign, U0, V0);
    int rc = check_params(M, N, R, 1, -16, 15);
    if (rc) return rc;
    if (B < 1) return set_err(LRF_EINVAL, "B must be >= 1");
    LRF_ON_DEVICE(c);
    Tables t;
    uniform_tables(t, B, M, R, sign != nullptr);
    const BcdPlan plan = plan_bcd(t.planes, 0, 0, 0, PLAN_INIT_ONLY, plan_settings(c));
    if ((rc = upload_tables(c, t, plan))) return rc;
    if ((rc = run_init(c, X, t, plan, sign, LRF_GRAM_EXP_FROM_DATA))) return rc;
    hipLaunchKernelGGL(k_emit_init, dim3((unsigned)t.blocks.size()), dim3(256), 0, c->stream, X, (const PlaneDesc*)c->planes.p,
                       (const BlockDesc*)c->blocks.p, (const float*)c->vf.p, (const float*)c->wf.p, U0, V0, plan.rp);
    LAUNCH_CHECK();
    return LRF_OK;
}

} // extern "C"

int encode_rgb_prepare(lrf_ctx* c, int64_t B, int64_t H, int64_t W, const int R[3], int K, int lo, int hi, bool with_sign,
                       bool fuse_gram /* planes_gram_eligible(rgb, H, W): the luma planes' Gram partials come from k_planes16_gram */, EncodePlan& ep,
                       bool upload)
{
    if (B < 1 || B > 65535) return set_err(LRF_EINVAL, "B=%ld out of range [1,65535]", (long)B);
    int rc = make_geom(H, W, &ep.g);
    if (rc) return rc;
    const ImageGeom& g = ep.g;
    for (int ch = 0; ch < 3; ch++)
        if ((rc = check_params(g.p[ch].M, 64, R[ch], K, lo, hi))) return rc;
    if ((rc = ensure(c, c->x, (size_t)B * g.img_floats * sizeof(float)))) return rc;
    // plane table: all Y planes first (four times the work of a chroma plane), then Cb, then Cr
    const long s_img = R[0] + R[1] + R[2];
    const long soff[3] = {0, R[0], R[0] + R[1]};
    for (int ch = 0; ch < 3; ch++) {
        ep.uoff[ch] = ep.u_img; ep.voff[ch] = ep.v_img;
        ep.u_img += (long)g.p[ch].M * R[ch];
        ep.v_img += 64L * R[ch];
    }
    // fp32 initial factors, if they are wanted (ranks above LRF_BIG_TO_ANY_RANK): per plane class contiguous [B][M][R] / [B][64][R]
    for (int ch = 0; ch < 3; ch++) {
        ep.u0c[ch + 1] = ep.u0c[ch] + B * (long)g.p[ch].M * R[ch];
        ep.v0c[ch + 1] = ep.v0c[ch] + B * 64L * R[ch];
    }
    for (int ch = 0; ch < 3; ch++)
        for (int64_t b = 0; b < B; b++) {
            add_plane(ep.t, b * g.img_floats + g.p[ch].xoff, b * ep.u_img + ep.uoff[ch], b * ep.v_img + ep.voff[ch],
                      ep.u0c[ch] + b * (long)g.p[ch].M * R[ch], ep.v0c[ch] + b * 64L * R[ch], g.p[ch].M, R[ch],
                      with_sign ? (int)(b * s_img + soff[ch]) : -1);
            if (fuse_gram && ch == 0) ep.t.planes.back().gram_fused = 1;
        }
    ep.bcd = plan_bcd(ep.t.planes, K, lo, hi, PLAN_FIRST_W0, plan_settings(c));
    return upload ? upload_tables(c, ep.t, ep.bcd) : LRF_OK;
}

extern "C" {

int lrf_qmf_encode_rgb_u8(lrf_ctx* c, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, const int R[3], int K, int lo,
                          int hi, const int8_t* sign, int8_t* U, int8_t* V)
{
    if (!c || !rgb || !R || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    LRF_ON_DEVICE(c);
    EncodePlan ep;
    const bool fuse = planes_gram_eligible(rgb, B, H, W);
    int rc = encode_rgb_prepare(c, B, H, W, R, K, lo, hi, sign != nullptr, fuse, ep, false);
    if (rc) return rc;
    const ImageGeom& g = ep.g;
    Tables& t = ep.t;
    const long u_img = ep.u_img, v_img = ep.v_img;
    const long *uoff = ep.uoff, *voff = ep.voff, *u0c = ep.u0c, *v0c = ep.v0c;
    // luma from the image bytes (plan_luma_bytes, lrf_plan.h): the luma blocks of k_bcd_p read `rgb`, and the fused planes kernel
    // leaves the luma rows of X unwritten (a pipe, which hands the bytes back at planes_done, keeps the X path)
    ep.bcd.luma_bytes = plan_luma_bytes(ep.bcd, t.planes, (int)B, H, W, reinterpret_cast<uintptr_t>(rgb), c->planes_done != nullptr, plan_settings(c));
    if (ep.bcd.luma_bytes) ep.bcd.luma = LumaSrc{rgb, (int)(H * W), (int)W, (int)(W / 8), (int)B};
    c->last_luma_source = ep.bcd.luma_bytes ? 1 : 0;
    // which X of the call k_bcd_p keeps in the Infinity Cache and which it streams past it (plan_x_residency marks the blocks:
    // the tables go up behind it; under a pipe nothing is marked, and these are the tables its prepare call left resident)
    const XResidency xr = plan_x_residency(ep.bcd, t, (int)B, ep.bcd.luma_bytes, c->planes_done != nullptr, plan_settings(c));
    c->last_x_kept_planes = xr.kept_planes;
    c->last_x_kept_bytes = xr.kept_bytes;
    if ((rc = upload_tables(c, t, ep.bcd))) return rc;
    float* X = (float*)c->x.p;
    if ((rc = fuse ? planes_gram_from_rgb(c, rgb, H, W, g, t, X, !ep.bcd.luma_bytes) : lrf_qmf_planes_from_rgb_u8(c, rgb, B, H, W, X))) return rc;
    if (c->planes_done) HIP_TRY(hipEventRecord(c->planes_done, c->stream)); // the RGB bytes are not read again
    if (ep.bcd.rmax > LRF_BIG_TO_ANY_RANK) {
        float *U0, *V0;
        if ((rc = init_to_fp32(c, X, t, ep.bcd, sign, (size_t)u0c[3], (size_t)v0c[3], &U0, &V0, LRF_PLANES_GRAM_EXP))) return rc;
        for (int ch = 0; ch < 3; ch++)
            if ((rc = any_bcd_from_init(c, X + g.p[ch].xoff, g.img_floats, (int)B, g.p[ch].M, R[ch], K, lo, hi, U0 + u0c[ch],
                                        V0 + v0c[ch], U + uoff[ch], u_img, V + voff[ch], v_img)))
                return rc;
        return LRF_OK;
    }
    return init_then_bcd(c, X, t, ep.bcd, sign, LRF_PLANES_GRAM_EXP, U, V);
}

// One batch at Q rank triples in one call (BASELINE config 3: an R-D sweep of 24 images x qualities 1..32; the reference's loop
// experiments/comparison/eval.py:83-110 calls qmf_encode once per image and quality).  What does not depend on the rank is done
// once per image — patch matrices, exact Gram matrices — and the SVD initialisation once per (image, channel) at the largest
// rank asked for that channel: the lower ranks take its leading columns (k_init_share).  The BCD of ALL (quality, image) pairs
// runs as one call of Q x B "virtual images" that share X: large per-family launches, the persistent kernel from 3584 blocks.
// Output: for q = 0..Q-1 the factors of the B images at triple q back to back, each in lrf_qmf_encode_rgb_u8's layout
// (U: offset sum_{q' < q} B u_img(q'), image stride u_img(q) = sum_c M_c R[q][c]; V likewise with 64 R[q][c]).
// sign: optional [B][Rmax_Y + Rmax_Cb + Rmax_Cr] int8 (component signs of the largest ranks; every triple uses its leading ones).
int lrf_qmf_encode_sweep_rgb_u8(lrf_ctx* c, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, int Q, const int* R /*[Q][3]*/, int K, int lo,
                                int hi, const int8_t* sign, int8_t* U, int8_t* V)
{
    if (!c || !rgb || !R || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    if (B < 1 || B > 65535) return set_err(LRF_EINVAL, "B=%ld out of range [1,65535]", (long)B);
    if (Q < 1 || Q > 4096) return set_err(LRF_EINVAL, "Q=%d out of range [1,4096]", Q);
    LRF_ON_DEVICE(c);
    ImageGeom g;
    int rc = make_geom(H, W, &g);
    if (rc) return rc;
    int rmaxc[3] = {0, 0, 0}, qbase[3] = {0, 0, 0}, rmax_t = 0;
    for (int q = 0; q < Q; q++)
        for (int ch = 0; ch < 3; ch++) {
            const int r = R[3 * q + ch];
            if ((rc = check_params(g.p[ch].M, 64, r, K, lo, hi))) return rc;
            if (r > LRF_BIG_TO_ANY_RANK) return set_err(LRF_ENOTSUP, "sweep call: rank %d > %d (ranks above it iterate on the any-shape kernels: one call per triple)", r, LRF_BIG_TO_ANY_RANK);
            if (r > rmaxc[ch]) { rmaxc[ch] = r; qbase[ch] = q; }
            rmax_t = r > rmax_t ? r : rmax_t;
        }
    if ((rc = ensure(c, c->x, (size_t)B * g.img_floats * sizeof(float)))) return rc;
    // output offsets of the triples
    std::vector<long> uq((size_t)Q + 1, 0), vq((size_t)Q + 1, 0), u_img((size_t)Q), v_img((size_t)Q);
    for (int q = 0; q < Q; q++) {
        u_img[q] = v_img[q] = 0;
        for (int ch = 0; ch < 3; ch++) { u_img[q] += (long)g.p[ch].M * R[3 * q + ch]; v_img[q] += 64L * R[3 * q + ch]; }
        uq[q + 1] = uq[q] + B * u_img[q];
        vq[q + 1] = vq[q] + B * v_img[q];
    }
    // The plane table: Q x B x 3 planes on B x 3 matrices.  Order: by kernel family (so that plan_bcd finds at most three runs),
    // inside a family the planes that compute an initialisation first (run_init launches k_init for a run's leading planes), then
    // luma before chroma; a call too small to split its families keeps one run: all initialising planes first.
    long nblk_img = 0;
    for (int ch = 0; ch < 3; ch++) nblk_img += (g.p[ch].M + LRF_KC - 1) / LRF_KC;
    const PlanSettings settings = plan_settings(c);
    const bool split = plan_splits((long)Q * B * nblk_img, rmax_t, settings);
    const long s_img = rmaxc[0] + rmaxc[1] + rmaxc[2];
    const long soff[3] = {0, rmaxc[0], (long)rmaxc[0] + rmaxc[1]};
    struct Spec { int q, ch; long b; };
    std::vector<Spec> order;
    order.reserve((size_t)Q * B * 3);
    for (int fam = 0; fam < (split ? 3 : 1); fam++)
        for (int base = 1; base >= 0; base--)
            for (int ch = 0; ch < 3; ch++)
                for (int q = 0; q < Q; q++) {
                    if (split && fam_of_rank(R[3 * q + ch]) != fam) continue;
                    if ((q == qbase[ch]) != (base == 1)) continue;
                    for (long b = 0; b < B; b++) order.push_back(Spec{q, ch, b});
                }
    Tables t;
    std::vector<int> base_index((size_t)B * 3, -1);
    for (const Spec& sp : order) {
        const int r = R[3 * sp.q + sp.ch];
        long uo = uq[sp.q] + sp.b * u_img[sp.q], vo = vq[sp.q] + sp.b * v_img[sp.q];
        for (int c2 = 0; c2 < sp.ch; c2++) { uo += (long)g.p[c2].M * R[3 * sp.q + c2]; vo += 64L * R[3 * sp.q + c2]; }
        if (sp.q == qbase[sp.ch]) base_index[(size_t)sp.b * 3 + sp.ch] = (int)t.planes.size();
        add_plane(t, sp.b * g.img_floats + g.p[sp.ch].xoff, uo, vo, 0, 0, g.p[sp.ch].M, r, sign ? (int)(sp.b * s_img + soff[sp.ch]) : -1);
    }
    const bool fuse = planes_gram_eligible(rgb, B, H, W);
    for (size_t pi = 0; pi < t.planes.size(); pi++) {
        const Spec& sp = order[pi];
        t.planes[pi].init_src = base_index[(size_t)sp.b * 3 + sp.ch];
        if (fuse && sp.ch == 0 && t.planes[pi].init_src == (int)pi) t.planes[pi].gram_fused = 1; // one luma plane per image
    }
    const BcdPlan plan = plan_bcd(t.planes, K, lo, hi, PLAN_FIRST_W0, settings, true);
    if ((rc = upload_tables(c, t, plan))) return rc;
    float* X = (float*)c->x.p;
    if ((rc = fuse ? planes_gram_from_rgb(c, rgb, H, W, g, t, X) : lrf_qmf_planes_from_rgb_u8(c, rgb, B, H, W, X))) return rc;
    if (c->planes_done) HIP_TRY(hipEventRecord(c->planes_done, c->stream));
    return init_then_bcd(c, X, t, plan, sign, LRF_PLANES_GRAM_EXP, U, V);
}

} // extern "C"

// A table that stays resident in `buf` under the bytes of its key: `tab`, and behind it `tail` — a function of the key that is
// not part of it.  Calls that repeat the key skip the synchronising upload.  The key is cleared before the upload and assigned
// only after it succeeded: a failed upload leaves no key that vouches for the buffer.
int keep_resident(lrf_ctx* c, DevBuf& buf, std::vector<char>& key, const void* tab, size_t tb, const void* tail, size_t tail_bytes)
{
    if (key.size() == tb && memcmp(key.data(), tab, tb) == 0 && buf.p) return LRF_OK;
    key.clear();
    int rc;
    if (tail_bytes) {
        std::vector<char> both(tb + tail_bytes);
        memcpy(both.data(), tab, tb);
        memcpy(both.data() + tb, tail, tail_bytes);
        rc = upload(c, buf, both.data(), both.size());
    } else
        rc = upload(c, buf, tab, tb);
    if (rc) return rc;
    key.assign((const char*)tab, (const char*)tab + tb);
    return LRF_OK;
}

// the planes stage of a ragged call: its table on the device (resident while calls repeat the list), then the launches of the plan
static int run_planes_ragged(lrf_ctx* c, const std::vector<EncRaggedDesc>& descs, const std::vector<RaggedBlock>& blocks,
                             const std::vector<EncRaggedLaunch>& launches, const uint8_t* rgb, float* X)
{
    // the planes table: descriptors, then workgroups (a function of the descriptors: they alone are the key)
    const size_t db = descs.size() * sizeof(EncRaggedDesc), bb = blocks.size() * sizeof(RaggedBlock);
    int rc = keep_resident(c, c->enc_ragged_tab, c->enc_ragged_key, descs.data(), db, blocks.data(), bb);
    if (rc) return rc;
    const EncRaggedDesc* d_desc = (const EncRaggedDesc*)c->enc_ragged_tab.p;
    const RaggedBlock* d_blk = (const RaggedBlock*)((const char*)c->enc_ragged_tab.p + db);
    {
        Prof p(c, LRF_K_PLANES);
        for (const EncRaggedLaunch& l : launches) {
            const RaggedBlock* bl = d_blk + l.block0;
#define LRF_RAGGED_STRIP(KH, KW) \
    hipLaunchKernelGGL((k_planes_strip_ragged<KH, KW>), dim3((unsigned)(8 * l.xcd_chunk)), dim3(256), 0, c->stream, rgb, X, d_desc, bl, (int)l.nblocks, l.xcd_chunk)
            switch (l.body) {
            case ENC_TILE16: hipLaunchKernelGGL(k_planes16_ragged, dim3((unsigned)l.nblocks), dim3(256), 0, c->stream, rgb, X, d_desc, bl); break;
            case ENC_STRIP22: LRF_RAGGED_STRIP(2, 2); break;
            case ENC_STRIP23: LRF_RAGGED_STRIP(2, 3); break;
            case ENC_STRIP32: LRF_RAGGED_STRIP(3, 2); break;
            default: LRF_RAGGED_STRIP(3, 3); break;
            }
#undef LRF_RAGGED_STRIP
            LAUNCH_CHECK();
        }
    }
    return LRF_OK;
}

// A refusal of check_window_call or check_windows (lrf_plan.h) in the words of the ten entries that decode crops
int refuse_window(const WindowRefusal& r, const WindowCall& k)
{
    const long j = (long)r.crop;
    switch (r.check) {
    case WIN_N_IMAGES: return set_err(LRF_EINVAL, "n_images=%ld out of range [1,65535]", (long)k.n_images);
    case WIN_N_CROPS: return set_err(LRF_EINVAL, "n_crops=%ld out of range [1,2^20]", (long)k.n_crops);
    case WIN_SIZE:
        if (k.resized) return set_err(LRF_EINVAL, "output size %ldx%ld out of range [1,16384]", (long)k.h, (long)k.w);
        return set_err(LRF_EINVAL, "crop size %ldx%ld out of range", (long)k.h, (long)k.w);
    case WIN_CAPACITY:
        if (k.channels == 1)
            return set_err(LRF_EINVAL, "%ld crops of %ldx%ld leave the output buffer of %ld elements", (long)k.n_crops, (long)k.h, (long)k.w, (long)k.out_len);
        return set_err(LRF_EINVAL, "%ld crops of 3x%ldx%ld leave the output buffer of %ld bytes", (long)k.n_crops, (long)k.h, (long)k.w, (long)k.out_len);
    case WIN_IMAGE: return set_err(LRF_EINVAL, "crop %ld: image %d out of range [0,%ld)", j, r.image, (long)k.n_images);
    case WIN_SCALE:
        if (k.scales == LRF_WIN_SCALES_GRAY) return set_err(LRF_EINVAL, "crop %ld: scale %d: 1, 2, 4 or 8 expected", j, r.scale);
        return set_err(LRF_EINVAL, "crop %ld: scale %d: 2, 4 or 8 expected", j, r.scale);
    case WIN_SIDES: return set_err(LRF_EINVAL, "crop %ld: box of %ldx%ld: both sides must be >= 1", j, (long)r.h, (long)r.w);
    default:
        if (k.scales)
            return set_err(LRF_EINVAL, "crop %ld: %ldx%ld at (%d,%d) leaves image %d of %ldx%ld at scale 1/%d", j, (long)r.h, (long)r.w, r.y0, r.x0, r.image,
                           (long)r.H, (long)r.W, r.scale);
        return set_err(LRF_EINVAL, "crop %ld: %ldx%ld at (%d,%d) leaves image %d of %ldx%ld", j, (long)r.h, (long)r.w, r.y0, r.x0, r.image, (long)r.H, (long)r.W);
    }
}
int check_crop_call(bool null_argument, const WindowCall& k)
{
    if (null_argument) return set_err(LRF_EINVAL, "NULL argument");
    const WindowRefusal r = check_window_call(k);
    return r.check == WIN_OK ? LRF_OK : refuse_window(r, k);
}

extern "C" {

// A list of images that differ in size and ranks in one encode (planes kernels: lrf_planes_ragged_kernel.hip; the tables:
// plan_encode_ragged).  Behind the planes stage the call is its plane table: Gram pass, initialisation and iterations read
// PlaneDesc / BlockDesc as in every other call, chosen by the same plan_bcd.  Everything the kernels index with is checked here,
// before anything is launched or written.
int lrf_qmf_encode_ragged_rgb_u8(lrf_ctx* c, int64_t n, const lrf_ragged_encode_image* images, const uint8_t* rgb, int64_t rgb_len, int K, int lo,
                                 int hi, const int8_t* sign, int64_t sign_len, int8_t* U, int64_t u_len, int8_t* V, int64_t v_len)
{
    if (!c || !images || !rgb || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    if (rgb_len < 1 || u_len < 1 || v_len < 1 || (sign && sign_len < 1)) return set_err(LRF_EINVAL, "a buffer length below 1");
    if (sign && sign_len > INT32_MAX) return set_err(LRF_ENOTSUP, "sign_len=%ld: sign offsets are 32-bit", (long)sign_len);
    std::vector<EncRaggedImage> ims((size_t)n);
    struct Range { long off, len; };
    std::vector<Range> ur((size_t)n), vr((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const lrf_ragged_encode_image& im = images[i];
        if (im.H < 1 || im.W < 1 || im.H > INT32_MAX || im.W > INT32_MAX) return set_err(LRF_EINVAL, "image %ld: size %ldx%ld out of range", (long)i, (long)im.H, (long)im.W);
        ImageGeom g;
        int rc = make_geom(im.H, im.W, &g);
        if (rc) return rc;
        for (int ch = 0; ch < 3; ch++)
            if ((rc = check_params(g.p[ch].M, 64, im.R[ch], K, lo, hi))) return rc;
        for (int ch = 0; ch < 3; ch++)
            if (im.R[ch] > LRF_BIG_TO_ANY_RANK)
                return set_err(LRF_ENOTSUP, "image %ld: rank %d > %d (ranks above it iterate on the any-shape kernels: lrf_qmf_encode_rgb_u8 per image)", (long)i, im.R[ch], LRF_BIG_TO_ANY_RANK);
        if (im.rgb_off < 0 || im.u_off < 0 || im.v_off < 0 || im.sign_off < -1) return set_err(LRF_EINVAL, "image %ld: negative offset", (long)i);
        if (im.H * im.W * 3 >= (1L << 31)) return set_err(LRF_ENOTSUP, "image %ld: too large for 32-bit pixel indexing", (long)i);
        // (every term is checked against the length before it is added to an offset: no sum can wrap)
        const long bytes = 3 * im.H * im.W;
        long u_img = 0, v_img = 0, s_img = 0;
        for (int ch = 0; ch < 3; ch++) {
            u_img += (long)g.p[ch].M * im.R[ch];
            v_img += 64L * im.R[ch];
            s_img += im.R[ch];
        }
        if (bytes > rgb_len || im.rgb_off > rgb_len - bytes) return set_err(LRF_EINVAL, "image %ld: its pixels leave the buffer of %ld bytes", (long)i, (long)rgb_len);
        if (u_img > u_len || im.u_off > u_len - u_img) return set_err(LRF_EINVAL, "image %ld: its U factors leave the buffer of %ld elements", (long)i, (long)u_len);
        if (v_img > v_len || im.v_off > v_len - v_img) return set_err(LRF_EINVAL, "image %ld: its V factors leave the buffer of %ld elements", (long)i, (long)v_len);
        const bool own_sign = sign && im.sign_off >= 0;
        if (own_sign && (s_img > sign_len || im.sign_off > sign_len - s_img)) return set_err(LRF_EINVAL, "image %ld: its signs leave the buffer of %ld elements", (long)i, (long)sign_len);
        EncRaggedImage& e = ims[(size_t)i];
        e.H = im.H; e.W = im.W;
        for (int ch = 0; ch < 3; ch++) e.R[ch] = im.R[ch];
        e.rgb_off = im.rgb_off; e.u_off = im.u_off; e.v_off = im.v_off;
        e.sign_off = own_sign ? im.sign_off : -1;
        e.aligned8 = ((reinterpret_cast<uintptr_t>(rgb) + (uintptr_t)im.rgb_off) & 7) == 0;
        ur[(size_t)i] = Range{im.u_off, u_img};
        vr[(size_t)i] = Range{im.v_off, v_img};
    }
    for (std::vector<Range>* r : {&ur, &vr}) { // no two images may share output bytes
        std::sort(r->begin(), r->end(), [](const Range& a, const Range& b) { return a.off < b.off; });
        for (size_t i = 1; i < r->size(); i++)
            if ((*r)[i].off - (*r)[i - 1].off < (*r)[i - 1].len) return set_err(LRF_EINVAL, "the %s ranges of two images overlap (at element %ld)", r == &ur ? "U" : "V", (*r)[i].off);
    }
    const PlanSettings settings = plan_settings(c);
    EncRaggedPlan plan = plan_encode_ragged(ims, settings);
    if (plan.too_many) return set_err(LRF_ENOTSUP, "%ld blocks in one call: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    int rc = ensure(c, c->x, (size_t)plan.x_floats * sizeof(float));
    if (rc) return rc;
    const BcdPlan bcd = plan_bcd(plan.t.planes, K, lo, hi, PLAN_FIRST_W0, settings);
    if ((rc = upload_tables(c, plan.t, bcd))) return rc;
    float* X = (float*)c->x.p;
    if ((rc = run_planes_ragged(c, plan.descs, plan.blocks, plan.launches, rgb, X))) return rc;
    if (c->planes_done) HIP_TRY(hipEventRecord(c->planes_done, c->stream)); // the RGB bytes are not read again
    return init_then_bcd(c, X, plan.t, bcd, sign, LRF_PLANES_GRAM_EXP, U, V);
}

// The two entries above married: n images that differ in size, each at a list of candidate rank triples of its own, m candidates
// in all (the tables: plan_encode_ragged_sweep).  The planes stage runs once per image, the Gram pass and the initialisation
// once per (image, channel) at the image's largest rank for that channel; the other candidates take its leading columns
// (k_init_share), and the BCD of all m candidates runs as one table that shares X.  Everything the kernels index with is checked
// here, before anything is launched or written.
int lrf_qmf_encode_ragged_sweep_rgb_u8(lrf_ctx* c, int64_t n, const lrf_ragged_sweep_image* images, int64_t m, const lrf_ragged_sweep_candidate* cands,
                                       const uint8_t* rgb, int64_t rgb_len, int K, int lo, int hi, const int8_t* sign, int64_t sign_len, int8_t* U,
                                       int64_t u_len, int8_t* V, int64_t v_len)
{
    if (!c || !images || !cands || !rgb || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    if (m < n || m > (1 << 20)) return set_err(LRF_EINVAL, "m=%ld out of range [n,2^20] (every image needs a candidate)", (long)m);
    if (rgb_len < 1 || u_len < 1 || v_len < 1 || (sign && sign_len < 1)) return set_err(LRF_EINVAL, "a buffer length below 1");
    if (sign && sign_len > INT32_MAX) return set_err(LRF_ENOTSUP, "sign_len=%ld: sign offsets are 32-bit", (long)sign_len);
    std::vector<EncSweepImage> ims((size_t)n);
    std::vector<ImageGeom> geoms((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const lrf_ragged_sweep_image& im = images[i];
        if (im.H < 1 || im.W < 1 || im.H > INT32_MAX || im.W > INT32_MAX) return set_err(LRF_EINVAL, "image %ld: size %ldx%ld out of range", (long)i, (long)im.H, (long)im.W);
        int rc = make_geom(im.H, im.W, &geoms[(size_t)i]);
        if (rc) return rc;
        if (im.rgb_off < 0 || im.sign_off < -1) return set_err(LRF_EINVAL, "image %ld: negative offset", (long)i);
        if (im.H * im.W * 3 >= (1L << 31)) return set_err(LRF_ENOTSUP, "image %ld: too large for 32-bit pixel indexing", (long)i);
        const long bytes = 3 * im.H * im.W;
        if (bytes > rgb_len || im.rgb_off > rgb_len - bytes) return set_err(LRF_EINVAL, "image %ld: its pixels leave the buffer of %ld bytes", (long)i, (long)rgb_len);
        EncSweepImage& e = ims[(size_t)i];
        e.H = im.H; e.W = im.W;
        e.rgb_off = im.rgb_off;
        e.sign_off = sign && im.sign_off >= 0 ? im.sign_off : -1;
        e.aligned8 = ((reinterpret_cast<uintptr_t>(rgb) + (uintptr_t)im.rgb_off) & 7) == 0;
    }
    std::vector<EncSweepCand> cs((size_t)m);
    std::vector<long> s_img((size_t)n * 3, 0); // the largest rank per (image, channel)
    struct Range { long off, len; };
    std::vector<Range> ur((size_t)m), vr((size_t)m);
    for (int64_t j = 0; j < m; j++) {
        const lrf_ragged_sweep_candidate& cd = cands[j];
        if (cd.image < 0 || cd.image >= n) return set_err(LRF_EINVAL, "candidate %ld: image %d out of range [0,%ld)", (long)j, cd.image, (long)n);
        const ImageGeom& g = geoms[(size_t)cd.image];
        int rc;
        for (int ch = 0; ch < 3; ch++)
            if ((rc = check_params(g.p[ch].M, 64, cd.R[ch], K, lo, hi))) return rc;
        for (int ch = 0; ch < 3; ch++)
            if (cd.R[ch] > LRF_BIG_TO_ANY_RANK)
                return set_err(LRF_ENOTSUP, "candidate %ld: rank %d > %d (ranks above it iterate on the any-shape kernels: lrf_qmf_encode_rgb_u8 per image)", (long)j, cd.R[ch], LRF_BIG_TO_ANY_RANK);
        if (cd.u_off < 0 || cd.v_off < 0) return set_err(LRF_EINVAL, "candidate %ld: negative offset", (long)j);
        // (every term is checked against the length before it is added to an offset: no sum can wrap)
        long u_img = 0, v_img = 0;
        for (int ch = 0; ch < 3; ch++) {
            u_img += (long)g.p[ch].M * cd.R[ch];
            v_img += 64L * cd.R[ch];
            long& s = s_img[(size_t)cd.image * 3 + ch];
            s = cd.R[ch] > s ? cd.R[ch] : s;
        }
        if (u_img > u_len || cd.u_off > u_len - u_img) return set_err(LRF_EINVAL, "candidate %ld: its U factors leave the buffer of %ld elements", (long)j, (long)u_len);
        if (v_img > v_len || cd.v_off > v_len - v_img) return set_err(LRF_EINVAL, "candidate %ld: its V factors leave the buffer of %ld elements", (long)j, (long)v_len);
        EncSweepCand& e = cs[(size_t)j];
        e.image = cd.image;
        for (int ch = 0; ch < 3; ch++) e.R[ch] = cd.R[ch];
        e.u_off = cd.u_off; e.v_off = cd.v_off;
        ur[(size_t)j] = Range{cd.u_off, u_img};
        vr[(size_t)j] = Range{cd.v_off, v_img};
    }
    for (int64_t i = 0; i < n; i++) {
        const long s = s_img[(size_t)i * 3] + s_img[(size_t)i * 3 + 1] + s_img[(size_t)i * 3 + 2];
        if (s_img[(size_t)i * 3] == 0) return set_err(LRF_EINVAL, "image %ld has no candidate", (long)i);
        if (ims[(size_t)i].sign_off >= 0 && (s > sign_len || ims[(size_t)i].sign_off > sign_len - s))
            return set_err(LRF_EINVAL, "image %ld: its %ld signs leave the buffer of %ld elements", (long)i, s, (long)sign_len);
    }
    for (std::vector<Range>* r : {&ur, &vr}) { // no two candidates may share output bytes
        std::sort(r->begin(), r->end(), [](const Range& a, const Range& b) { return a.off < b.off; });
        for (size_t i = 1; i < r->size(); i++)
            if ((*r)[i].off - (*r)[i - 1].off < (*r)[i - 1].len) return set_err(LRF_EINVAL, "the %s ranges of two candidates overlap (at element %ld)", r == &ur ? "U" : "V", (*r)[i].off);
    }
    const PlanSettings settings = plan_settings(c);
    EncRaggedSweepPlan plan = plan_encode_ragged_sweep(ims, cs, settings);
    if (plan.too_many) return set_err(LRF_ENOTSUP, "%ld blocks in one call: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    int rc = ensure(c, c->x, (size_t)plan.x_floats * sizeof(float));
    if (rc) return rc;
    const BcdPlan bcd = plan_bcd(plan.t.planes, K, lo, hi, PLAN_FIRST_W0, settings, true);
    if ((rc = upload_tables(c, plan.t, bcd))) return rc;
    float* X = (float*)c->x.p;
    if ((rc = run_planes_ragged(c, plan.descs, plan.blocks, plan.launches, rgb, X))) return rc;
    if (c->planes_done) HIP_TRY(hipEventRecord(c->planes_done, c->stream)); // the RGB bytes are not read again
    return init_then_bcd(c, X, plan.t, bcd, sign, LRF_PLANES_GRAM_EXP, U, V);
}

// ---- what the decode and SSE entries share (which body serves an image: decode_plan, lrf_plan.h) ---------------------------------
static bool decode_no_tiled()
{
    static const bool no_tiled = dev_flag("LRF_DECODE_NO_TILED");
    return no_tiled;
}
// A run-time rank-bound class 0 .. LRF_DEC_CLASSES - 1 as a template argument: LAUNCH(CLS) with CLS a constant; the bounds
// (chroma, luma) of a class for the kernels that take the pair
#define LRF_FOR_DEC_CLASS(cls, LAUNCH)  \
    switch (cls) {                      \
    case 0: LAUNCH(0); break;           \
    case 1: LAUNCH(1); break;           \
    case 2: LAUNCH(2); break;           \
    case 3: LAUNCH(3); break;           \
    default: LAUNCH(4); break;          \
    }
constexpr int dec_class_rc(int cls) { return cls >= 3 ? 16 : (cls >= 1 ? 8 : 4); }
constexpr int dec_class_rl(int cls) { return cls == 4 ? 32 : (cls >= 2 ? 16 : 8); }

// The images of a list entry, described (describe_images) or refused in the entry's words: noun "image" or "item", buf what
// rgb holds for the entry, "output" or "source".  Geometry refusals keep make_geom's wording.
static int refuse_image(const DescribeRefusal& r, const char* noun, const char* buf)
{
    const long i = (long)r.image;
    ImageGeom g;
    switch (r.check) {
    case DESC_SIZE: return set_err(LRF_EINVAL, "%s %ld: size %ldx%ld out of range", noun, i, (long)r.a, (long)r.b);
    case DESC_GEOM: return make_geom(r.a, r.b, &g);
    case DESC_RANK: return set_err(LRF_EINVAL, "%s %ld: rank %d out of range", noun, i, (int)r.a);
    case DESC_NEGATIVE: return set_err(LRF_EINVAL, "%s %ld: negative offset", noun, i);
    case DESC_U: return set_err(LRF_EINVAL, "%s %ld: its U factors leave the buffer of %ld elements", noun, i, (long)r.a);
    case DESC_V: return set_err(LRF_EINVAL, "%s %ld: its V factors leave the buffer of %ld elements", noun, i, (long)r.a);
    default: return set_err(LRF_EINVAL, "%s %ld: its %s leaves the buffer of %ld bytes", noun, i, buf, (long)r.a);
    }
}
static int describe(int64_t n, const lrf_ragged_image* images, int64_t u_len, int64_t v_len, DescribeOptions o, const char* noun, const char* buf,
                    std::vector<RaggedDesc>& descs, std::vector<RaggedWork>* work = nullptr)
{
    o.no_tiled = decode_no_tiled();
    const DescribeRefusal r = describe_images(n, images, u_len, v_len, o, descs, work);
    return r.check == DESC_OK ? LRF_OK : refuse_image(r, noun, buf);
}
// the options of an entry whose rgb holds the images at full size: rgb_off and the extents are checked
static DescribeOptions full_size_rgb(int64_t rgb_len)
{
    DescribeOptions o;
    o.check_rgb = true;
    o.rgb_len = rgb_len;
    return o;
}
// groups of four pixels per thread of k_decode8 / k_sse8: as many as leave the call ~2048 workgroups (small calls keep one group per thread)
static long decode8_reps(long images, long n4) { return decode8_reps_of(images * ((n4 + 255) / 256)); }

int lrf_qmf_decode_rgb_u8(lrf_ctx* c, const int8_t* U, const int8_t* V, int64_t B, int64_t H, int64_t W, const int R[3],
                          uint8_t* rgb)
{
    if (!c || !U || !V || !R || !rgb) return set_err(LRF_EINVAL, "NULL argument");
    if (B < 1 || B > 65535) return set_err(LRF_EINVAL, "B=%ld out of range [1,65535]", (long)B);
    ImageGeom g;
    int rc = make_geom(H, W, &g);
    if (rc) return rc;
    for (int ch = 0; ch < 3; ch++)
        if (R[ch] < 1 || R[ch] > 64) return set_err(LRF_EINVAL, "rank %d out of range", R[ch]);
    LRF_ON_DEVICE(c);
    long u_img = 0, v_img = 0;
    for (int ch = 0; ch < 3; ch++) {
        u_img += (long)g.p[ch].M * R[ch];
        v_img += 64L * R[ch];
    }
    long n4 = (long)H * ((W + 3) / 4);
    Prof p(c, LRF_K_DECODE);
    const DecodePlan plan = decode_plan(g, H, W, R, (reinterpret_cast<uintptr_t>(rgb) & 7) == 0, decode_no_tiled());
    if (plan.kind == DEC_TILE16 || plan.kind == DEC_STRIP) {
        const int per_strip = (g.p[0].nw + 31) / 32;
        const dim3 grid16((unsigned)((H / 16) * per_strip), (unsigned)B), grids((unsigned)(((g.p[0].nh + 1) / 2) * per_strip), (unsigned)B);
#define LRF_DECODE_TILED(CLS)                                                                                                     \
    do {                                                                                                                         \
        if (plan.kind == DEC_TILE16)                                                                                             \
            hipLaunchKernelGGL((k_decode16<dec_class_rc(CLS), dec_class_rl(CLS)>), grid16, dim3(256), 0, c->stream, U, V, (int)H, (int)W, g, R[0], R[1], R[2], u_img, v_img, rgb); \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_decode_strip<dec_class_rc(CLS), dec_class_rl(CLS)>), grids, dim3(256), 0, c->stream, U, V, (int)H, (int)W, g, R[0], R[1], R[2], u_img, v_img, rgb, per_strip); \
    } while (0)
        LRF_FOR_DEC_CLASS(plan.cls, LRF_DECODE_TILED)
#undef LRF_DECODE_TILED
    }
    else if (plan.kind == DEC_R8) {
        const long reps = decode8_reps(B, n4);
        hipLaunchKernelGGL(k_decode8, dim3((unsigned)((n4 + 256 * reps - 1) / (256 * reps)), (unsigned)B), dim3(256), 0, c->stream, U, V, (int)H, (int)W,
                           g, R[0], R[1], R[2], u_img, v_img, rgb, (int)reps);
    }
    else
        hipLaunchKernelGGL(k_decode, dim3((unsigned)((n4 + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, U, V, (int)H, (int)W,
                           g, R[0], R[1], R[2], u_img, v_img, rgb);
    LAUNCH_CHECK();
    return LRF_OK;
}

// the launches of a ragged decode (plan_decode_ragged) over tables already on their way to the device
static int launch_decode_ragged(lrf_ctx* c, const RaggedPlan& plan, const int8_t* U, const int8_t* V, uint8_t* rgb, const RaggedDesc* d_desc,
                                const RaggedBlock* d_blk)
{
    for (const RaggedLaunch& l : plan.launches) {
        const dim3 grid((unsigned)l.nblocks);
        const RaggedBlock* bl = d_blk + l.block0;
        if (l.kind == DEC_TILE16)
            hipLaunchKernelGGL((k_decode_ragged_tiled<false, -1>), grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl);
        else if (l.kind == DEC_STRIP) {
#define LRF_RAGGED_STRIP(CLS) hipLaunchKernelGGL((k_decode_ragged_tiled<true, CLS>), grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl)
            LRF_FOR_DEC_CLASS(l.cls, LRF_RAGGED_STRIP)
#undef LRF_RAGGED_STRIP
        } else if (l.kind == DEC_R8)
            hipLaunchKernelGGL(k_decode8_ragged, grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl, l.reps);
        else
            hipLaunchKernelGGL(k_decode_ragged_any, grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

// A list of images that differ in size and ranks in one call (kernels: lrf_decode_ragged_kernel.hip; the launches:
// plan_decode_ragged).  Everything the kernels index with is checked here, before any launch.
int lrf_qmf_decode_ragged_rgb_u8(lrf_ctx* c, int64_t n, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                 int64_t v_len, uint8_t* rgb, int64_t rgb_len)
{
    if (!c || !images || !U || !V || !rgb) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    std::vector<RaggedDesc> descs;
    std::vector<RaggedWork> work;
    DescribeOptions o = full_size_rgb(rgb_len);
    o.aligned8 = false; // (k_decode16's 8-byte stores: per image, by where its output starts)
    o.rgb_base = reinterpret_cast<uintptr_t>(rgb);
    int rc = describe(n, images, u_len, v_len, o, "image", "output", descs, &work);
    if (rc) return rc;
    const RaggedPlan plan = plan_decode_ragged(work);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld work items in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    // the table: descriptors, then blocks (a function of the descriptors: they alone are the key)
    const size_t db = descs.size() * sizeof(RaggedDesc);
    if ((rc = keep_resident(c, c->ragged_tab, c->ragged_key, descs.data(), db, plan.blocks.data(), plan.blocks.size() * sizeof(RaggedBlock)))) return rc;
    const RaggedDesc* d_desc = (const RaggedDesc*)c->ragged_tab.p;
    const RaggedBlock* d_blk = (const RaggedBlock*)((const char*)c->ragged_tab.p + db);
    Prof p(c, LRF_K_DECODE);
    return launch_decode_ragged(c, plan, U, V, rgb, d_desc, d_blk);
}

// The crop table of one call on its way to the device: stream-ordered, no wait for the stream.  The pinned staging slots take
// turns; a slot is written again only after the event recorded behind its last copy says that copy has run (a wait for that
// one copy at most, LRF_CROP_SLOTS calls back).  The device table is one buffer: the copy of a call is ordered behind the
// kernels of the call before it on the same stream.
int stage_crop_bytes(lrf_ctx* c, const void* table, size_t bytes)
{
    int rc = ensure(c, c->crop_tab, bytes);
    if (rc) return rc;
    lrf_ctx::CropSlot& s = c->crop_slot[c->crop_next];
    c->crop_next = (c->crop_next + 1) % LRF_CROP_SLOTS;
    if (!s.copied) HIP_TRY(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    else if (s.in_flight) HIP_TRY(hipEventSynchronize(s.copied));
    s.in_flight = false;
    if (bytes > s.cap) {
        if (s.h) HIP_TRY(hipHostFree(s.h));
        s.h = nullptr;
        s.cap = 0;
        HIP_TRY(hipHostMalloc(&s.h, bytes + bytes / 2, hipHostMallocDefault));
        s.cap = bytes + bytes / 2;
    }
    memcpy(s.h, table, bytes);
    HIP_TRY(hipMemcpyAsync(c->crop_tab.p, s.h, bytes, hipMemcpyHostToDevice, c->stream));
    s.in_flight = true;
    HIP_TRY(hipEventRecord(s.copied, c->stream));
    return LRF_OK;
}
static int stage_crop_table(lrf_ctx* c, const std::vector<CropEntry>& table) { return stage_crop_bytes(c, table.data(), table.size() * sizeof(CropEntry)); }
// the image descriptors of the entries that decode windows (full-size, scaled, resized): one table, resident between their calls
static int resident_crop_descs(lrf_ctx* c, const std::vector<RaggedDesc>& descs)
{
    return keep_resident(c, c->crop_desc, c->crop_desc_key, descs.data(), descs.size() * sizeof(RaggedDesc));
}

// n_crops windows of one size (h, w) out of a list of images that differ in size and ranks (kernels:
// lrf_decode_crops_kernel.hip; the launches: plan_decode_crops).  Everything the kernels index with is checked here, before
// any launch.  The image descriptors stay resident between calls (their bytes are the key); the crop list does not.
// DecodeOut (lrf_host.h): where the three entries that decode windows write — the bytes of the _rgb_u8 entries or the tensor of the _tensor
// entries (lrf_decode_tensor_host.inc), `len` counted in its elements.  One body per entry serves both: the checks, the launch
// plan and the staging do not depend on it, only which instantiation a launch names.
static int decode_crops_to(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                           int64_t n_crops, const lrf_crop* crops, int64_t h, int64_t w, const DecodeOut& o)
{
    void* const rgb = o.p;
    const WindowCall k = {n_images, n_crops, h, w, false, 0, 3, o.len};
    int rc = check_crop_call(!c || !images || !U || !V || !crops || !rgb, k);
    if (rc) return rc;
    std::vector<RaggedDesc> descs;
    std::vector<RaggedWork> work;
    // (the output is the crops', and the windowed tiled body stores at any alignment: the defaults)
    if ((rc = describe(n_images, images, u_len, v_len, DescribeOptions{}, "image", "output", descs, &work))) return rc;
    std::vector<CropEntry> list;
    if ((rc = checked_windows(k, descs, crops, list))) return rc;
    const CropPlan plan = plan_decode_crops(work, list, (int)h, (int)w);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld workgroups in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    if ((rc = resident_crop_descs(c, descs))) return rc;
    const RaggedDesc* d_desc = (const RaggedDesc*)c->crop_desc.p;
    Prof p(c, LRF_K_DECODE);
    if ((rc = stage_crop_table(c, plan.table))) return rc;
    const CropEntry* d_crop = (const CropEntry*)c->crop_tab.p;
    for (const CropLaunch& l : plan.launches) {
        const dim3 grid((unsigned)(l.ncrops * l.wgs));
        const CropEntry* ce = d_crop + l.crop0;
        if (o.dtype >= 0)
            with_tensor_type(o, [&](auto* out) {
                using T = std::remove_pointer_t<decltype(out)>;
                if (l.kind == DEC_STRIP) {
#define LRF_CROPS_TILED(CLS) \
    hipLaunchKernelGGL((k_decode_crops_tiled_t<CLS, T>), grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, ce, (int)h, (int)w, (int)l.wgs)
                    LRF_FOR_DEC_CLASS(l.cls, LRF_CROPS_TILED)
#undef LRF_CROPS_TILED
                } else if (l.kind == DEC_R8)
                    hipLaunchKernelGGL(k_decode8_crops_t<T>, grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, ce, (int)h, (int)w, (int)l.wgs);
                else
                    hipLaunchKernelGGL(k_decode_crops_any_t<T>, grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, ce, (int)h, (int)w, (int)l.wgs);
            });
        else if (l.kind == DEC_STRIP) {
#define LRF_CROPS_TILED(CLS) \
    hipLaunchKernelGGL((k_decode_crops_tiled<CLS>), grid, dim3(256), 0, c->stream, U, V, (uint8_t*)rgb, d_desc, ce, (int)h, (int)w, (int)l.wgs)
            LRF_FOR_DEC_CLASS(l.cls, LRF_CROPS_TILED)
#undef LRF_CROPS_TILED
        } else if (l.kind == DEC_R8)
            hipLaunchKernelGGL(k_decode8_crops, grid, dim3(256), 0, c->stream, U, V, (uint8_t*)rgb, d_desc, ce, (int)h, (int)w, (int)l.wgs);
        else
            hipLaunchKernelGGL(k_decode_crops_any, grid, dim3(256), 0, c->stream, U, V, (uint8_t*)rgb, d_desc, ce, (int)h, (int)w, (int)l.wgs);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}
int lrf_qmf_decode_crops_rgb_u8(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                int64_t v_len, int64_t n_crops, const lrf_crop* crops, int64_t h, int64_t w, uint8_t* rgb, int64_t rgb_len)
{
    return decode_crops_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, h, w, bytes_out(rgb, rgb_len));
}

// The squared error of Q x B decodes against the B source images, without the decoded images (kernels and the choice of the
// work item: lrf_sweep_sse_kernel.hip).  The triples are sorted by the decode body that serves them — for a geometry the tiled
// 16-aligned body covers and ranks <= (32,16,16) that is ONE launch over all (triple, image, tile) items — and described by a table on
// the device, which stays resident while calls repeat the same (B, H, W, triples).
int lrf_qmf_sweep_sse_rgb_u8(lrf_ctx* c, const uint8_t* rgb, const int8_t* U, const int8_t* V, int64_t B, int64_t H, int64_t W, int Q, const int* R,
                             uint64_t* sse)
{
    if (!c || !rgb || !U || !V || !R || !sse) return set_err(LRF_EINVAL, "NULL argument");
    if (B < 1 || B > 65535) return set_err(LRF_EINVAL, "B=%ld out of range [1,65535]", (long)B);
    if (Q < 1 || Q > 4096) return set_err(LRF_EINVAL, "Q=%d out of range [1,4096]", Q);
    ImageGeom g;
    int rc = make_geom(H, W, &g);
    if (rc) return rc;
    for (int i = 0; i < 3 * Q; i++)
        if (R[i] < 1 || R[i] > 64) return set_err(LRF_EINVAL, "rank %d out of range", R[i]);
    LRF_ON_DEVICE(c);
    // the table: the items of the tiled body first, then k_sse8's, then k_sse_any's (source rows of 16-aligned images are read in
    // 8-byte pieces whatever the pointer: loads need no alignment, so DEC_TILE16 does not ask for it here)
    std::vector<SseItem> items[3];
    int tiled_kind = DEC_STRIP;
    long uo = 0, vo = 0;
    for (int q = 0; q < Q; q++) {
        const int* r = R + 3 * q;
        SseItem it{};
        it.u_base = uo;
        it.v_base = vo;
        for (int ch = 0; ch < 3; ch++) { it.u_img += (long)g.p[ch].M * r[ch]; it.v_img += 64L * r[ch]; }
        it.R0 = r[0]; it.R1 = r[1]; it.R2 = r[2];
        it.q = q;
        const DecodePlan plan = decode_plan(g, H, W, r, true, decode_no_tiled());
        it.cls = plan.cls;
        if (plan.kind == DEC_TILE16) tiled_kind = DEC_TILE16; // (a property of the geometry: the same for every tiled triple)
        items[plan.kind <= DEC_STRIP ? 0 : plan.kind - 1].push_back(it);
        uo += B * it.u_img;
        vo += B * it.v_img;
    }
    const long n4 = (long)H * ((W + 3) / 4);
    const int per_strip = (g.p[0].nw + 31) / 32;
    const long tiles = tiled_kind == DEC_TILE16 ? (H / 16) * per_strip : (long)((g.p[0].nh + 1) / 2) * per_strip;
    const long reps = decode8_reps(B * (long)items[1].size(), n4);
    const long groups[3] = {tiles, (n4 + 256 * reps - 1) / (256 * reps), (n4 + 255) / 256};
    if (tiled_kind == DEC_STRIP) // a launch per class: the classes stand together
        std::stable_sort(items[0].begin(), items[0].end(), [](const SseItem& a, const SseItem& b) { return a.cls < b.cls; });
    std::vector<SseItem> tab;
    for (int k = 0; k < 3; k++) {
        if (groups[k] * (long)items[k].size() >= (1L << 31)) return set_err(LRF_EINVAL, "%ld work items in one launch: split the sweep", groups[k] * (long)items[k].size());
        tab.insert(tab.end(), items[k].begin(), items[k].end());
    }
    if ((rc = keep_resident(c, c->sse_tab, c->sse_key, tab.data(), tab.size() * sizeof(SseItem)))) return rc;
    const SseItem* d_tab = (const SseItem*)c->sse_tab.p;
    unsigned long long* d_sse = reinterpret_cast<unsigned long long*>(sse);
    Prof p(c, LRF_K_METRICS); // the scoring stage: timed with lrf_image_metrics_u8
    HIP_TRY(hipMemsetAsync(sse, 0, (size_t)Q * B * sizeof(uint64_t), c->stream));
    if (tiled_kind == DEC_TILE16 && !items[0].empty()) {
        const int nq = (int)items[0].size();
        hipLaunchKernelGGL((k_sse_tiled<false, -1>), dim3((unsigned)(tiles * nq), (unsigned)B), dim3(256), 0, c->stream, rgb, U, V, (int)H, (int)W, g, d_tab, nq,
                           per_strip, (int)B, d_sse);
        LAUNCH_CHECK();
    } else {
        for (size_t i0 = 0; i0 < items[0].size();) { // the strip body: one launch per class present
            size_t i1 = i0;
            while (i1 < items[0].size() && items[0][i1].cls == items[0][i0].cls) i1++;
            const int nq = (int)(i1 - i0);
            const dim3 grid((unsigned)(tiles * nq), (unsigned)B);
#define LRF_SSE_STRIP(CLS) hipLaunchKernelGGL((k_sse_tiled<true, CLS>), grid, dim3(256), 0, c->stream, rgb, U, V, (int)H, (int)W, g, d_tab + i0, nq, per_strip, (int)B, d_sse)
            LRF_FOR_DEC_CLASS(items[0][i0].cls, LRF_SSE_STRIP)
#undef LRF_SSE_STRIP
            LAUNCH_CHECK();
            i0 = i1;
        }
    }
    if (int nq = (int)items[1].size()) {
        hipLaunchKernelGGL(k_sse8, dim3((unsigned)(groups[1] * nq), (unsigned)B), dim3(256), 0, c->stream, rgb, U, V, (int)H, (int)W, g,
                           d_tab + items[0].size(), nq, (int)reps, (int)B, d_sse);
        LAUNCH_CHECK();
    }
    if (int nq = (int)items[2].size()) {
        hipLaunchKernelGGL(k_sse_any, dim3((unsigned)(groups[2] * nq), (unsigned)B), dim3(256), 0, c->stream, rgb, U, V, (int)H, (int)W, g,
                           d_tab + items[0].size() + items[1].size(), nq, (int)B, d_sse);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}


// The squared error of n (factors, source) items that differ in size and ranks, without the decoded images (kernels:
// lrf_sse_ragged_kernel.hip; classification: decode_plan; the launches: plan_decode_ragged).  Validation is
// lrf_qmf_decode_ragged_rgb_u8's with rgb read-only: the source ranges of items may overlap.  Candidate lists change from call
// to call, so the table (descriptors, then blocks) is not kept: it travels stream-ordered through the pinned slots of the crop
// table, and the call does not wait for the stream.
int lrf_qmf_sse_ragged_rgb_u8(lrf_ctx* c, int64_t n, const lrf_ragged_image* items, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                              const uint8_t* rgb, int64_t rgb_len, uint64_t* sse)
{
    if (!c || !items || !U || !V || !rgb || !sse) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    std::vector<RaggedDesc> descs;
    std::vector<RaggedWork> work;
    // (the sink's loads need no alignment: a 16-aligned item keeps the 16-aligned body wherever its source starts)
    int rc = describe(n, items, u_len, v_len, full_size_rgb(rgb_len), "item", "source", descs, &work);
    if (rc) return rc;
    const RaggedPlan plan = plan_decode_ragged(work);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld work items in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    const size_t db = descs.size() * sizeof(RaggedDesc), bb = plan.blocks.size() * sizeof(RaggedBlock);
    std::vector<char> tab(db + bb);
    memcpy(tab.data(), descs.data(), db);
    memcpy(tab.data() + db, plan.blocks.data(), bb);
    Prof p(c, LRF_K_DECODE);
    if ((rc = stage_crop_bytes(c, tab.data(), tab.size()))) return rc;
    const RaggedDesc* d_desc = (const RaggedDesc*)c->crop_tab.p;
    const RaggedBlock* d_blk = (const RaggedBlock*)((const char*)c->crop_tab.p + db);
    unsigned long long* d_sse = reinterpret_cast<unsigned long long*>(sse);
    HIP_TRY(hipMemsetAsync(sse, 0, (size_t)n * sizeof(uint64_t), c->stream));
    for (const RaggedLaunch& l : plan.launches) {
        const dim3 grid((unsigned)l.nblocks);
        const RaggedBlock* bl = d_blk + l.block0;
        if (l.kind == DEC_TILE16)
            hipLaunchKernelGGL((k_sse_ragged_tiled<false, -1>), grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl, d_sse);
        else if (l.kind == DEC_STRIP) {
#define LRF_SSE_RAGGED_STRIP(CLS) hipLaunchKernelGGL((k_sse_ragged_tiled<true, CLS>), grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl, d_sse)
            LRF_FOR_DEC_CLASS(l.cls, LRF_SSE_RAGGED_STRIP)
#undef LRF_SSE_RAGGED_STRIP
        } else if (l.kind == DEC_R8)
            hipLaunchKernelGGL(k_sse8_ragged, grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl, l.reps, d_sse);
        else
            hipLaunchKernelGGL(k_sse_ragged_any, grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, bl, d_sse);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}


// The squared error and the SSIM of n (factors, source) items from the factors, in bounded memory (plan_metrics_chunks): per
// chunk of consecutive items the ragged decode into lrf_ctx::ssim_scratch, then the ragged metrics (lrf_metrics.hip) with the
// sources as a and the scratch as b.  Validation is lrf_qmf_sse_ragged_rgb_u8's plus the 7x7 window; every chunk's tables are
// built and checked once before the first launch (and dropped: a sweep's block tables run to tens of megabytes), then built
// again chunk by chunk on their way to the device.  The tables travel through the pinned slots of the crop table.
int lrf_qmf_ssim_ragged_rgb_u8(lrf_ctx* c, int64_t n, const lrf_ragged_image* items, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                               const uint8_t* rgb, int64_t rgb_len, int64_t scratch_bytes, uint64_t* sse, double* ssim)
{
    if (!c || !items || !U || !V || !rgb || !sse || !ssim) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    if (scratch_bytes < 0) return set_err(LRF_EINVAL, "scratch_bytes=%ld is negative", (long)scratch_bytes);
    std::vector<RaggedDesc> descs;
    int rc = describe(n, items, u_len, v_len, full_size_rgb(rgb_len), "item", "source", descs);
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++)
        if (items[i].H < 7 || items[i].W < 7)
            return set_err(LRF_EINVAL, "item %ld: win_size exceeds image extent (%ldx%ld, window 7x7)", (long)i, (long)items[i].H, (long)items[i].W);
    const MetricsChunks ch = plan_metrics_chunks(n, items, scratch_bytes ? scratch_bytes : LRF_SSIM_SCRATCH_DEFAULT);
    LRF_ON_DEVICE(c);
    if ((size_t)ch.max_bytes > c->ssim_scratch.cap) { // exactly what the largest chunk holds: the cap bounds the buffer
        DevBuf& b = c->ssim_scratch;
        if (b.p) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipFree(b.p));
            b.p = nullptr;
            b.cap = 0;
        }
        const hipError_t e = hipMalloc(&b.p, (size_t)ch.max_bytes);
        if (e != hipSuccess) return set_err(LRF_ENOMEM, "hipMalloc(%ld) failed: %s", (long)ch.max_bytes, hipGetErrorString(e));
        b.cap = (size_t)ch.max_bytes;
    }
    uint8_t* scratch = (uint8_t*)c->ssim_scratch.p;
    std::vector<RaggedWork> work;
    std::vector<lrf_ragged_image> its;
    std::vector<lrf_image_pair> pairs;
    RaggedPlan dplan;
    MetricsRaggedPlan mplan;
    // the tables of one chunk: its items decoded back to back (16-byte steps) into the scratch, scored against their sources
    auto build = [&](const MetricsChunk& k) -> int {
        its.assign(items + k.item0, items + k.item0 + k.nitems);
        pairs.resize((size_t)k.nitems);
        for (int64_t j = 0; j < k.nitems; j++) {
            pairs[(size_t)j] = lrf_image_pair{its[(size_t)j].H, its[(size_t)j].W, its[(size_t)j].rgb_off, ch.off[(size_t)(k.item0 + j)]};
            its[(size_t)j].rgb_off = ch.off[(size_t)(k.item0 + j)];
        }
        DescribeOptions o = full_size_rgb(k.bytes);
        o.aligned8 = false;
        o.rgb_base = reinterpret_cast<uintptr_t>(scratch);
        int rc_ = describe(k.nitems, its.data(), u_len, v_len, o, "item", "decoded image", descs, &work);
        if (rc_) return rc_;
        dplan = plan_decode_ragged(work);
        if (dplan.too_many) return set_err(LRF_EINVAL, "%ld work items in one launch: split the list", dplan.too_many);
        const MetricsCall mk = {3, rgb_len, k.bytes, reinterpret_cast<uintptr_t>(rgb), reinterpret_cast<uintptr_t>(scratch), true};
        mplan = plan_metrics_ragged(k.nitems, pairs.data(), mk);
        return mplan.refusal.check == MTR_OK ? LRF_OK : refuse_metrics(mplan.refusal);
    };
    size_t ws = 0;
    for (const MetricsChunk& k : ch.chunks) {
        if ((rc = build(k))) return rc;
        ws = std::max(ws, metrics_ragged_workspace(mplan));
    }
    if ((rc = ensure(c, c->metrics, ws))) return rc;
    Prof p(c, LRF_K_METRICS);
    std::vector<char> tab;
    for (const MetricsChunk& k : ch.chunks) {
        if (ch.chunks.size() > 1 && (rc = build(k))) return rc; // (one chunk: the tables of the checking pass stand)
        const size_t db = descs.size() * sizeof(RaggedDesc), bb = dplan.blocks.size() * sizeof(RaggedBlock);
        tab.resize(db + bb);
        memcpy(tab.data(), descs.data(), db);
        memcpy(tab.data() + db, dplan.blocks.data(), bb);
        if ((rc = stage_crop_bytes(c, tab.data(), tab.size()))) return rc;
        if ((rc = launch_decode_ragged(c, dplan, U, V, scratch, (const RaggedDesc*)c->crop_tab.p, (const RaggedBlock*)((const char*)c->crop_tab.p + db)))) return rc;
        if ((rc = metrics_ragged_launch(c, mplan, 3, rgb, scratch, sse + k.item0, ssim + k.item0))) return rc;
    }
    return LRF_OK;
}

#if defined(LRF_STAMPS) || defined(LRF_INIT_STAMPS) || defined(LRF_BLK_STAMPS) || defined(LRF_REG_STAMPS)
int lrf_debug_read_stamps(lrf_ctx* c, unsigned long long* out_host, int n)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * (size_t)n));
    return LRF_OK;
}
#endif

#ifdef LRF_GRAM_STAMPS
int lrf_debug_read_gram_stamps(lrf_ctx* c, unsigned long long* out_host, int n)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_gram_stamps), sizeof(unsigned long long) * (size_t)n));
    return LRF_OK;
}
#endif

} // extern "C"

#include "lrf_decode_scaled_host.inc"
#include "lrf_decode_resized_host.inc"
#include "lrf_decode_tensor_host.inc"
