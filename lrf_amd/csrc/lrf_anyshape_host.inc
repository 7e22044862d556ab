// lrf_anyshape_host.inc — launch sequencing of the any-shape QMF path (kernels: lrf_anyshape_kernels.hip).
// Included by lrf_any.hip before its extern "C" block.

// LRF_ANY_MAX_SIDE (include/lrf_hip.h): min(M, N) handled by k_any_eig (eight columns per thread)
// LRF_ANY_MAX_RANK: k_any_gs keeps 64 rows of R | 1 floats in 160 KB of LDS

static int any_check(int64_t B, int64_t M, int64_t N, int R, int lo, int hi)
{
    if (B < 1 || B > 65535) return set_err(LRF_EINVAL, "B=%ld out of range [1,65535]", (long)B);
    if (M < 1 || N < 1) return set_err(LRF_EINVAL, "matrix %ldx%ld is empty", (long)M, (long)N);
    if (M > (1 << 24) || N > (1 << 24)) return set_err(LRF_ENOTSUP, "matrix side above 2^24");
    if (R < 1) return set_err(LRF_EINVAL, "rank must be >= 1 (got %d)", R);
    if (R > LRF_ANY_MAX_RANK) return set_err(LRF_ENOTSUP, "rank %d > %d not implemented", R, LRF_ANY_MAX_RANK);
    if (lo > hi || lo < -128 || hi > 127) return set_err(LRF_EINVAL, "bounds (%d,%d) outside int8", lo, hi);
    return LRF_OK;
}

// C [B][I][R] = A' Bm with the reference's order (k_any_prod + k_any_fold); native: ATen's small-product kernel.  Which kernel,
// its grid and loop counts: plan_any_prod (lrf_plan.cpp)
static int any_prod(lrf_ctx* c, const float* A, long a_batch, long sai, long sak, const float* Bm, long b_batch, float* C, int B,
                    int I, int D, int R, bool native)
{
    static const bool prod_small = dev_flag("LRF_ANY_PROD_SMALL");
    const AnyProdPlan p = plan_any_prod(I, D, R, B, sai, sak, native, prod_small);
    const int nblk = p.nblk;
    float* P = C;
    if (nblk > 1) {
        int rc = ensure(c, c->any_p, (size_t)B * nblk * I * R * sizeof(float));
        if (rc) return rc;
        P = (float*)c->any_p.p;
    }
    if (p.refused) return set_err(LRF_ENOTSUP, "contraction of length %d with rank %d exceeds the launch grid", D, R);
    const dim3 grid(p.gx, p.gy, p.gz), block((unsigned)p.threads);
    switch (p.k) {
    case ANY_PROD_THIN_LONG:
        hipLaunchKernelGGL(k_any_prod_thin_long, grid, block, 0, c->stream, A, a_batch, sai, sak, Bm, b_batch, P, I, D, R, nblk);
        break;
    case ANY_PROD_THIN_SHORT4:
        hipLaunchKernelGGL(k_any_prod_thin_short<4>, grid, block, 0, c->stream, A, a_batch, sai, sak, Bm, b_batch, P, I, D, R, p.tpw);
        break;
    case ANY_PROD_THIN_SHORT8:
        hipLaunchKernelGGL(k_any_prod_thin_short<8>, grid, block, 0, c->stream, A, a_batch, sai, sak, Bm, b_batch, P, I, D, R, p.tpw);
        break;
    case ANY_PROD_THIN_SHORT16:
        hipLaunchKernelGGL(k_any_prod_thin_short<16>, grid, block, 0, c->stream, A, a_batch, sai, sak, Bm, b_batch, P, I, D, R, p.tpw);
        break;
    case ANY_PROD_BIG:
        hipLaunchKernelGGL(k_any_prod_big, grid, block, 0, c->stream, A, a_batch, sai, sak, Bm, b_batch, P, I, D, R, nblk);
        break;
    case ANY_PROD_TILED:
        hipLaunchKernelGGL(k_any_prod, grid, block, 0, c->stream, A, a_batch, sai, sak, Bm, b_batch, P, I, D, R, nblk, p.native ? 1 : 0, p.tiles);
        break;
    }
    LAUNCH_CHECK();
    if (p.fold) {
        hipLaunchKernelGGL(k_any_fold, dim3(p.fold_gx, (unsigned)B), dim3(256), 0, c->stream, (const float*)P, C, (long)I * R, nblk);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

// CoordinateDescent.update_u (lrf/factorization/qmf.py:93-126) for the factor F [B][rows][R]; `trans`: x.mT (update_v, :128-139).
// The native flags of the two products and the Gauss-Seidel variant: plan_any_update (lrf_plan.cpp)
static int any_update(lrf_ctx* c, const float* X, long x_batch, int B, int M, int N, int R, bool trans, float* F, const float* Fix,
                      float lo, float hi, float l1 = 0.f, float l2 = 0.f, float eps = LRF_EPS, bool int_rows = false)
{
    const int rows = trans ? N : M, depth = trans ? M : N;
    float* a = (float*)c->any_a.p;
    float* bm = (float*)c->any_b.p;
    int rc;
    // a = x @ v  (or x.mT @ u)
    if ((rc = any_prod(c, X, x_batch, trans ? 1 : N, trans ? N : 1, Fix, (long)depth * R, a, B, rows, depth, R,
                       (long)depth * rows * R < LRF_ANY_NATIVE_BELOW)))
        return rc;
    // b = v.mT @ v
    if ((rc = any_prod(c, Fix, (long)depth * R, 1, R, Fix, (long)depth * R, bm, B, R, depth, R, (long)depth * R * R < LRF_ANY_NATIVE_BELOW)))
        return rc;
    static const bool gs_f32 = dev_flag("LRF_ANY_GS_F32");
    const AnyGsPlan g = plan_any_gs(rows, R, B, int_rows, gs_f32);
    const dim3 ggrid(g.gx, g.gy);
    switch (g.k) {
    case ANY_GS_I8: // F holds integers of the int8 range: byte rows in LDS
        hipLaunchKernelGGL((k_any_gs<int8_t, true>), ggrid, dim3(64), g.lds, c->stream, (const float*)a, (const float*)bm, F, rows, R, g.native_gs,
                           lo, hi, l1, l2, eps);
        break;
    case ANY_GS_F32_LDS:
        hipLaunchKernelGGL((k_any_gs<float, true>), ggrid, dim3(64), g.lds, c->stream, (const float*)a, (const float*)bm, F, rows, R, g.native_gs,
                           lo, hi, l1, l2, eps);
        break;
    case ANY_GS_F32_NOLDS:
        hipLaunchKernelGGL((k_any_gs<float, false>), ggrid, dim3(64), g.lds, c->stream, (const float*)a, (const float*)bm, F, rows, R, g.native_gs,
                           lo, hi, l1, l2, eps);
        break;
    }
    LAUNCH_CHECK();
    return LRF_OK;
}

int any_workspace(lrf_ctx* c, int B, int M, int N, int R)
{
    const size_t mx = (size_t)(M > N ? M : N);
    int rc;
    if ((rc = ensure(c, c->any_uf, (size_t)B * M * R * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->any_vf, (size_t)B * N * R * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->any_a, (size_t)B * mx * R * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->any_b, (size_t)B * R * R * sizeof(float)))) return rc;
    if (!(c->attr_done & (1u << 8))) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_any_gs<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_ANY_GS_MAX_LDS));
        HIP_TRY(hipFuncSetAttribute((const void*)k_any_gs<float, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LRF_ANY_GS_MAX_LDS));
        HIP_TRY(hipFuncSetAttribute((const void*)k_any_gs<int8_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
        c->attr_done |= 1u << 8;
    }
    return LRF_OK;
}

// K iterations from the fp32 factors in any_uf / any_vf, then the int8 cast (qmf.py:260).  x_batch: floats between the
// matrices of X; u_batch / v_batch: int8 elements between the outputs of consecutive matrices.
int any_run_bcd_ex(lrf_ctx* c, const float* X, long x_batch, int B, int M, int N, int R, int K, int lo, int hi, int8_t* U,
                          long u_batch, int8_t* V, long v_batch)
{
    float* Uf = (float*)c->any_uf.p;
    float* Vf = (float*)c->any_vf.p;
    int rc;
    for (int it = 0; it < K; it++) {
        Prof p(c, LRF_K_BCD);
        // after the first sweep a factor holds the rounded, clamped integers of the int8 range (any_check)
        if ((rc = any_update(c, X, x_batch, B, M, N, R, false, Uf, Vf, (float)lo, (float)hi, 0.f, 0.f, LRF_EPS, it > 0))) return rc;
        if ((rc = any_update(c, X, x_batch, B, M, N, R, true, Vf, Uf, (float)lo, (float)hi, 0.f, 0.f, LRF_EPS, it > 0))) return rc;
    }
    const long nu = (long)M * R, nv = (long)N * R;
    hipLaunchKernelGGL(k_any_to_i8, dim3((unsigned)((nu + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, (const float*)Uf, U, nu, u_batch);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_any_to_i8, dim3((unsigned)((nv + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, (const float*)Vf, V, nv, v_batch);
    LAUNCH_CHECK();
    return LRF_OK;
}

static int any_run_bcd(lrf_ctx* c, const float* X, int B, int M, int N, int R, int K, int lo, int hi, int8_t* U, int8_t* V)
{
    return any_run_bcd_ex(c, X, (long)M * N, B, M, N, R, K, lo, hi, U, (long)M * R, V, (long)N * R);
}

// QMF.decompose in its general form (lrf/factorization/qmf.py:74-214; include/lrf_hip.h lrf_qmf_decompose_ex_f32): fp32
// factors in any_uf / any_vf on entry (the initialisation) and on return.  Wd [B][2] device, initial pair on entry.
// affine_always: the pair is not [0; 1] on entry (SVDInit(num_levels=...), qmf.py:56-68): the u / v updates see
// safe_divide(x - w0, w1) also when w itself is not updated.  The same holds for [0; 1] itself when eps > 1: safe_divide takes
// CoordinateDescent's eps (qmf.py:105) and |w1| = 1 < eps divides x by eps.
static int any_run_bcd_general(lrf_ctx* c, const float* X, int B, int M, int N, int R, int K, float lo, float hi, float l1_u, float l2_u,
                               float l1_v, float l2_v, int factors, float* Wd, float eps = LRF_EPS, bool affine_always = false)
{
    affine_always = affine_always || eps > 1.f;
    float* Uf = (float*)c->any_uf.p;
    float* Vf = (float*)c->any_vf.p;
    const long per = (long)M * N;
    const int ntiles = (M + 63) / 64;
    int rc;
    const float* Xuse = X;
    if ((factors & 4) || affine_always) { // the u / v updates see safe_divide(x - w0, w1): materialised per iteration (the pair changes every time)
        if ((rc = ensure(c, c->any_e2, (size_t)B * per * sizeof(float) + 8 + (size_t)B * ntiles * 4 * sizeof(double)))) return rc;
    }
    float* Xp = (float*)c->any_e2.p;
    double* part = (factors & 4) ? reinterpret_cast<double*>(reinterpret_cast<char*>(c->any_e2.p) + (((size_t)B * per * sizeof(float) + 7) & ~(size_t)7)) : nullptr;
    for (int it = 0; it < K; it++) {
        Prof p(c, LRF_K_BCD);
        if ((factors & 4) || (affine_always && it == 0)) { // (a pair that is never updated: once)
            hipLaunchKernelGGL(k_any_affine, dim3((unsigned)((per + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, X, (const float*)Wd, Xp, per,
                               eps);
            LAUNCH_CHECK();
            Xuse = Xp;
        }
        if ((factors & 1) && (rc = any_update(c, Xuse, per, B, M, N, R, false, Uf, Vf, lo, hi, l1_u, l2_u, eps))) return rc;
        if ((factors & 2) && (rc = any_update(c, Xuse, per, B, M, N, R, true, Vf, Uf, lo, hi, l1_v, l2_v, eps))) return rc;
        if (factors & 4) {
            hipLaunchKernelGGL(k_any_wstats, dim3((unsigned)ntiles, (unsigned)B), dim3(256), 0, c->stream, X, (const float*)Uf, (const float*)Vf, M, N,
                               R, part);
            LAUNCH_CHECK();
            hipLaunchKernelGGL(k_any_wsolve, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, c->stream, (const double*)part, ntiles, (double)M * (double)N,
                               Wd, B);
            LAUNCH_CHECK();
        }
    }
    return LRF_OK;
}

template <int NCT>
static int any_launch_eig(lrf_ctx* c, int nb, double* G, int n, int R, const int8_t* sign, float* E1, float* E2, double* Z, double* D,
                          unsigned attr_bit, int rcap)
{
    const size_t lds = (size_t)(6 * (size_t)n + R + 24) * sizeof(double);
    if (!(c->attr_done & (1u << attr_bit))) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_any_eig<NCT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((6 * (size_t)LRF_ANY_MAX_SIDE + LRF_ANY_MAX_RANK + 24) * sizeof(double))));
        c->attr_done |= 1u << attr_bit;
    }
    const double* td = nullptr;
    if constexpr (NCT == 1) {
        static const bool no_reg = dev_flag("LRF_ANY_TRIDIAG_GLOBAL");
        if (n > 64 && n <= 192 && !no_reg) { // the matrix fits the registers of one workgroup
            int rc;
            if ((rc = ensure(c, c->any_td, (size_t)nb * 3 * n * sizeof(double)))) return rc;
            if (n <= 128)
                hipLaunchKernelGGL(k_any_tridiag_reg<2>, dim3((unsigned)nb), dim3(512), 0, c->stream, G, n, (double*)c->any_td.p);
            else
                hipLaunchKernelGGL(k_any_tridiag_reg<3>, dim3((unsigned)nb), dim3(768), 0, c->stream, G, n, (double*)c->any_td.p);
            LAUNCH_CHECK();
            td = (const double*)c->any_td.p;
        }
    }
    static const bool unblocked = dev_flag("LRF_ANY_TRIDIAG_UNBLOCKED");
    static const bool full_square = dev_flag("LRF_ANY_TRIDIAG_SQUARE");
    if (n > 192 && !unblocked) {
        int rc;
        if ((rc = ensure(c, c->any_td, (size_t)nb * 3 * n * sizeof(double)))) return rc;
        if constexpr (NCT <= 2) {
            if (!full_square) { // the triangle-only form (k_any_tridiag_sym): panels of 8 steps; eight waves for n <= 256, four above
                constexpr int NB = 8, NCH = 4 * NCT, NW = NCT == 1 ? 8 : 4;
                const size_t ns = (((size_t)n + 1) & ~(size_t)1) + 16;
                const size_t lds_sym = (2 * (size_t)NB * ns + ns + (size_t)NCH * ns + NW * ns + NW * 16 * 65 + 64 * NW + 8 * NB + 24) * sizeof(double);
                if (!(c->attr_done & (1u << (attr_bit + 16)))) {
                    HIP_TRY(hipFuncSetAttribute((const void*)k_any_tridiag_sym<NCT, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                    c->attr_done |= 1u << (attr_bit + 16);
                }
                hipLaunchKernelGGL((k_any_tridiag_sym<NCT, NW>), dim3((unsigned)nb), dim3(64 * NW), lds_sym, c->stream, G, n, (double*)c->any_td.p);
                LAUNCH_CHECK();
                td = (const double*)c->any_td.p;
            }
        }
        if (!td) { // panels of 16 / 16 / 8 / 4 steps over the full square (k_any_tridiag_blk): sides above 512
            constexpr int NB = NCT == 1 ? 16 : 32 / NCT;
            if (!(c->attr_done & (1u << (attr_bit + 8)))) {
                HIP_TRY(hipFuncSetAttribute((const void*)k_any_tridiag_blk<NCT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)((2 * (size_t)NB * 256 * NCT + 64 + 8 * NB + 24) * sizeof(double))));
                c->attr_done |= 1u << (attr_bit + 8);
            }
            const size_t lds_blk = (2 * (size_t)NB * ((n + 1) & ~1) + 64 + 8 * NB + 24) * sizeof(double);
            hipLaunchKernelGGL(k_any_tridiag_blk<NCT>, dim3((unsigned)nb), dim3(256), lds_blk, c->stream, G, n, (double*)c->any_td.p);
            LAUNCH_CHECK();
            td = (const double*)c->any_td.p;
        }
    }
    hipLaunchKernelGGL(k_any_eig<NCT>, dim3((unsigned)nb), dim3(256), lds, c->stream, G, n, R, sign, E1, E2, Z, D, c->init_sweeps, rcap, td);
    return LRF_OK;
}

// Top-R pairs of B Gram matrices [N][N] (N <= 256) of matrices with M rows -> Vn = e sqrt(sigma), Wn = e / sqrt(sigma),
// then Uf = X Wn: the eigen-solver and the product of this path serving the [M,192] matrices of svd_encode and of the RGB
// colour-space branch (they replaced a single-buffered solver and a thread-per-element product: svd_encode of 256 images
// 15.5 -> 8.3 ms, DESIGN.md section 1).
static int any_eig_from_gram(lrf_ctx* c, double* G, int B, int M, int N, int R, const int8_t* sign, float* Vn, float* Wn)
{
    const int Rc = R < N ? R : N;
    int rc;
    if ((rc = ensure(c, c->any_g, (size_t)B * 3 * N * Rc * sizeof(double)))) return rc;
    double* Z = (double*)c->any_g.p;
    double* Dw = Z + (size_t)B * N * Rc;
    if ((rc = any_launch_eig<1>(c, B, G, N, R, sign, Vn, Wn, Z, Dw, 9, M < N ? M : N))) return rc;
    LAUNCH_CHECK();
    return LRF_OK;
}
static int any_factors_from_gram(lrf_ctx* c, const float* X, double* G, int B, int M, int N, int R, const int8_t* sign, float* Vn,
                                 float* Wn, float* Uf)
{
    int rc = any_eig_from_gram(c, G, B, M, N, R, sign, Vn, Wn);
    if (rc) return rc;
    return any_prod(c, X, (long)M * N, N, 1, Wn, (long)N * R, Uf, B, M, N, R, false);
}

// SVDInit.forward (qmf.py:42-71): any_uf = U sqrt(s), any_vf = V sqrt(s); sign: device [B][R] or NULL
static int any_run_init(lrf_ctx* c, const float* X, int B, int M, int N, int R, const int8_t* sign)
{
    Prof p(c, LRF_K_INIT);
    const bool tall = N <= M;
    const int n = tall ? N : M, D = tall ? M : N;
    if (n > LRF_ANY_MAX_SIDE) return set_err(LRF_ENOTSUP, "min(M, N) = %d > %d not implemented", n, LRF_ANY_MAX_SIDE);
    const int Rc = R < n ? R : n;
    float* Uf = (float*)c->any_uf.p;
    float* Vf = (float*)c->any_vf.p;
    float* E1 = tall ? Vf : Uf;
    int rc;
    if ((rc = ensure(c, c->any_e2, (size_t)B * n * R * sizeof(float)))) return rc;
    float* E2 = (float*)c->any_e2.p;
    const size_t per = sizeof(double) * ((size_t)n * n + (size_t)3 * n * Rc);
    const long chunk = plan_any_init_chunk(n, Rc, B);
    if ((rc = ensure(c, c->any_g, (size_t)chunk * per))) return rc;
    double* G = (double*)c->any_g.p;
    double* Z = G + (size_t)chunk * n * n;
    double* Dw = Z + (size_t)chunk * n * Rc;
    const unsigned nt = (unsigned)((n + 31) / 32);
    for (long b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (int)((B - b0 < chunk) ? B - b0 : chunk);
        static const bool gram_valu = dev_flag("LRF_ANY_GRAM_VALU");
        if (gram_valu)
            hipLaunchKernelGGL(k_any_gram, dim3(nt, nt, (unsigned)nb), dim3(256), 0, c->stream, X + b0 * (long)M * N, (long)M * N,
                               (long)(tall ? N : 1), (long)(tall ? 1 : N), n, D, G);
        else
            hipLaunchKernelGGL(k_any_gram_mfma, dim3((nt + 1) / 2, (nt + 1) / 2, (unsigned)nb), dim3(256), 0, c->stream,
                               X + b0 * (long)M * N, (long)M * N, (long)(tall ? N : 1), (long)(tall ? 1 : N), n, D, G);
        LAUNCH_CHECK();
        const int8_t* sg = (sign && tall) ? sign + b0 * R : nullptr;
        float* e1 = E1 + b0 * (long)n * R;
        float* e2 = E2 + b0 * (long)n * R;
        if (n <= 256) rc = any_launch_eig<1>(c, nb, G, n, R, sg, e1, e2, Z, Dw, 9, n);
        else if (n <= 512) rc = any_launch_eig<2>(c, nb, G, n, R, sg, e1, e2, Z, Dw, 10, n);
        else if (n <= 1024) rc = any_launch_eig<4>(c, nb, G, n, R, sg, e1, e2, Z, Dw, 11, n);
        else rc = any_launch_eig<8>(c, nb, G, n, R, sg, e1, e2, Z, Dw, 12, n);
        if (rc) return rc;
        LAUNCH_CHECK();
    }
    // the long factor: u0 = X (e / sqrt(sigma))  or  v0 = X^T (e / sqrt(sigma)), k-ordered fma chains
    if (tall) return any_prod(c, X, (long)M * N, N, 1, E2, (long)n * R, Uf, B, M, N, R, false);
    if ((rc = any_prod(c, X, (long)M * N, 1, N, E2, (long)n * R, Vf, B, N, M, R, false))) return rc;
    hipLaunchKernelGGL(k_any_signfix, dim3((unsigned)B), dim3(256), (size_t)R * sizeof(float), c->stream, Uf, Vf, M, N, R, sign);
    LAUNCH_CHECK();
    return LRF_OK;
}

int any_decompose(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, int K, int lo, int hi, const int8_t* sign,
                         int8_t* U, int8_t* V)
{
    int rc = any_check(B, M, N, R, lo, hi);
    if (rc) return rc;
    if (K < 1) return set_err(LRF_ENOTSUP, "num_iters=%d: use lrf_qmf_svd_init_f32 for K=0", K);
    LRF_ON_DEVICE(c);
    if ((rc = any_workspace(c, (int)B, (int)M, (int)N, R))) return rc;
    if ((rc = any_run_init(c, X, (int)B, (int)M, (int)N, R, sign))) return rc;
    return any_run_bcd(c, X, (int)B, (int)M, (int)N, R, K, lo, hi, U, V);
}

int any_bcd(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, int K, int lo, int hi, const float* U0,
                   const float* V0, int8_t* U, int8_t* V)
{
    int rc = any_check(B, M, N, R, lo, hi);
    if (rc) return rc;
    if (K < 1) return set_err(LRF_ENOTSUP, "num_iters=%d: nothing to iterate", K);
    LRF_ON_DEVICE(c);
    if ((rc = any_workspace(c, (int)B, (int)M, (int)N, R))) return rc;
    HIP_TRY(hipMemcpyAsync(c->any_uf.p, U0, (size_t)B * M * R * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->any_vf.p, V0, (size_t)B * N * R * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return any_run_bcd(c, X, (int)B, (int)M, (int)N, R, K, lo, hi, U, V);
}

int any_svd_init(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, const int8_t* sign, float* U0, float* V0)
{
    int rc = any_check(B, M, N, R, -16, 15);
    if (rc) return rc;
    LRF_ON_DEVICE(c);
    if ((rc = any_workspace(c, (int)B, (int)M, (int)N, R))) return rc;
    if ((rc = any_run_init(c, X, (int)B, (int)M, (int)N, R, sign))) return rc;
    HIP_TRY(hipMemcpyAsync(U0, c->any_uf.p, (size_t)B * M * R * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(V0, c->any_vf.p, (size_t)B * N * R * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return LRF_OK;
}

// geometry of plane c for patches p x q (p = 0: no patches): lrf/compression/qmf.py:230-262, :264-286
struct AnyGeom {
    int h, w, hp, wp, top, left, nw;
    long M, N;
};
// hc, wc: the chroma plane size; <= 0 = the default scale_factor (0.5, 0.5): floor(H / 2) x floor(W / 2) (qmf.py:230)
static int any_geom(int64_t H, int64_t W, int p, int q, int ch, AnyGeom* g, int64_t hc = 0, int64_t wc = 0)
{
    if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return set_err(LRF_EINVAL, "image size %ldx%ld", (long)H, (long)W);
    if (ch < 0 || ch > 2) return set_err(LRF_EINVAL, "plane %d", ch);
    if ((p == 0) != (q == 0) || p < 0 || q < 0 || p > 1024 || q > 1024) return set_err(LRF_EINVAL, "patch size (%d,%d)", p, q);
    if (hc > (1 << 20) || wc > (1 << 20)) return set_err(LRF_EINVAL, "chroma plane %ldx%ld", (long)hc, (long)wc);
    const long h = ch ? (hc > 0 ? (long)hc : (long)floor((double)H * 0.5)) : H, w = ch ? (wc > 0 ? (long)wc : (long)floor((double)W * 0.5)) : W;
    if (h < 1 || w < 1) return set_err(LRF_EINVAL, "image %ldx%ld too small", (long)H, (long)W);
    g->h = (int)h;
    g->w = (int)w;
    if (p == 0) {
        g->hp = (int)h; g->wp = (int)w; g->top = g->left = 0; g->nw = 0;
        g->M = h; g->N = w;
        return LRF_OK;
    }
    const long hp = h + (p - h % p) % p, wp = w + (q - w % q) % q;
    const long pt = (hp - h) / 2, pb = (hp - h) - pt, pl = (wp - w) / 2, pr = (wp - w) - pl;
    if (pt >= h || pb >= h || pl >= w || pr >= w) return set_err(LRF_EINVAL, "reflect padding larger than the plane (%ldx%ld)", h, w);
    g->hp = (int)hp; g->wp = (int)wp; g->top = (int)pt; g->left = (int)pl; g->nw = (int)(wp / q);
    g->M = (hp / p) * (wp / q);
    g->N = (long)p * q;
    return LRF_OK;
}
