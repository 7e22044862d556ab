// lrf_gray_encode_host.inc — the host side of the gray encode lists (lrf_qmf_encode_gray_ragged_u8,
// lrf_qmf_encode_gray_ragged_sweep_u8, lrf_qmf_sse_gray_ragged_u8; kernels: lrf_gray_encode_kernel.hip; the list check and the
// tables: describe_gray_encode, plan_encode_gray_ragged_sweep in lrf_plan.cpp).  Included by lrf_channels.hip.
// Everything the kernels index with is checked here, before any launch or write.  Behind the planes stage a call is its plane
// table: Gram pass, initialisation and iterations read PlaneDesc / BlockDesc as in every other call, chosen by the same plan_bcd,
// with the settings of lrf_qmf_encode_gray_u8 -> decompose64 (the Gram exponent from the data), so that an image's bytes are
// that call's at B = 1.

// describe_gray_encode with its refusal worded
static int gray_encode_describe(int64_t n, const lrf_gray_sweep_image* images, int64_t m, const lrf_gray_sweep_candidate* cands, const GrayEncCall& k,
                                std::vector<EncGrayImage>& ims, std::vector<EncGrayCand>& cs)
{
    const GrayEncRefusal r = describe_gray_encode(n, images, m, cands, k, ims, cs);
    const char* noun = r.candidate ? "candidate" : "image";
    const long i = (long)r.index;
    switch (r.check) {
    case GENC_OK: return LRF_OK;
    case GENC_N: return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", i);
    case GENC_M: return set_err(LRF_EINVAL, "m=%ld out of range [n,2^20] (every image needs a candidate)", i);
    case GENC_SIZE: return set_err(LRF_EINVAL, "image %ld: size %ldx%ld: sides in [1,2^20] expected", i, (long)r.a, (long)r.b);
    case GENC_GEOM: return set_err(LRF_EINVAL, "image %ld: reflect padding larger than the image (%ldx%ld, patches 8x8)", i, (long)r.a, (long)r.b);
    case GENC_PIXELS: return set_err(LRF_ENOTSUP, "image %ld: %ldx%ld is too large for 32-bit pixel indexing", i, (long)r.a, (long)r.b);
    case GENC_NEGATIVE: return set_err(LRF_EINVAL, "%s %ld: negative offset", noun, i);
    case GENC_GRAY: return set_err(LRF_EINVAL, "image %ld: its pixels leave the buffer of %ld bytes", i, (long)r.a);
    case GENC_K:
    case GENC_BOUNDS: return check_params(1, LRF_PATCH_ELEMS, 1, k.K, k.lo, k.hi); // (its words and codes)
    case GENC_IMAGE: return set_err(LRF_EINVAL, "candidate %ld: image %ld out of range [0,%ld)", i, (long)r.a, (long)n);
    case GENC_RANK_LOW: return set_err(LRF_EINVAL, "candidate %ld: rank must be >= 1 (got %ld)", i, (long)r.a);
    case GENC_RANK_BIG:
        return set_err(LRF_ENOTSUP, "candidate %ld: rank %ld > %d (ranks above it iterate on the any-shape kernels: lrf_qmf_encode_gray_u8 per image)", i,
                       (long)r.a, LRF_BIG_TO_ANY_RANK);
    case GENC_U: return set_err(LRF_EINVAL, "candidate %ld: its U factor leaves the buffer of %ld elements", i, (long)r.a);
    case GENC_V: return set_err(LRF_EINVAL, "candidate %ld: its V factor leaves the buffer of %ld elements", i, (long)r.a);
    case GENC_NO_CAND: return set_err(LRF_EINVAL, "image %ld has no candidate", i);
    case GENC_SIGN: return set_err(LRF_EINVAL, "image %ld: its signs leave the buffer of %ld elements (sign offsets are 32-bit)", i, (long)r.a);
    default: return set_err(LRF_EINVAL, "the %s ranges of two candidates overlap (at element %ld)", r.check == GENC_OVERLAP_U ? "U" : "V", (long)r.a);
    }
}

// the planes stage of a gray list: its table on the device (resident while calls repeat the list), then the launches of the plan
static int run_gray_planes_ragged(lrf_ctx* c, const EncGraySweepPlan& plan, const uint8_t* gray, float* X)
{
    // descriptors, then workgroups (a function of the descriptors: they alone are the key)
    const size_t db = plan.descs.size() * sizeof(EncGrayDesc), bb = plan.blocks.size() * sizeof(RaggedBlock);
    int rc = keep_resident(c, c->enc_gray_tab, c->enc_gray_key, plan.descs.data(), db, plan.blocks.data(), bb);
    if (rc) return rc;
    const EncGrayDesc* d_desc = (const EncGrayDesc*)c->enc_gray_tab.p;
    const RaggedBlock* d_blk = (const RaggedBlock*)((const char*)c->enc_gray_tab.p + db);
    Prof p(c, LRF_K_PLANES);
    for (const EncGrayLaunch& l : plan.launches) {
        if (l.body == ENC_GRAY16)
            hipLaunchKernelGGL(k_gray_planes16_ragged, dim3((unsigned)l.nblocks), dim3(256), 0, c->stream, gray, X, d_desc, d_blk + l.block0);
        else
            hipLaunchKernelGGL(k_gray_planes_ragged, dim3((unsigned)l.nblocks), dim3(256), 0, c->stream, gray, X, d_desc, d_blk + l.block0);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

extern "C" {

int lrf_qmf_encode_gray_ragged_sweep_u8(lrf_ctx* c, int64_t n, const lrf_gray_sweep_image* images, int64_t m, const lrf_gray_sweep_candidate* cands,
                                        const uint8_t* gray, int64_t gray_len, int K, int lo, int hi, const int8_t* sign, int64_t sign_len, int8_t* U,
                                        int64_t u_len, int8_t* V, int64_t v_len)
{
    if (!c || !images || !cands || !gray || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    if (gray_len < 1 || u_len < 1 || v_len < 1 || (sign && sign_len < 1)) return set_err(LRF_EINVAL, "a buffer length below 1");
    const GrayEncCall k = {gray_len, sign ? sign_len : 0, u_len, v_len, reinterpret_cast<uintptr_t>(gray), K, lo, hi};
    std::vector<EncGrayImage> ims;
    std::vector<EncGrayCand> cs;
    int rc = gray_encode_describe(n, images, m, cands, k, ims, cs);
    if (rc) return rc;
    const PlanSettings settings = plan_settings(c);
    EncGraySweepPlan plan = plan_encode_gray_ragged_sweep(ims, cs, settings);
    if (plan.too_many) return set_err(LRF_ENOTSUP, "%ld blocks in one call: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    if ((rc = ensure(c, c->x, (size_t)plan.x_floats * sizeof(float)))) return rc;
    const BcdPlan bcd = plan_bcd(plan.t.planes, K, lo, hi, PLAN_FIRST_W0, settings, m > n);
    if ((rc = upload_tables(c, plan.t, bcd))) return rc;
    float* X = (float*)c->x.p;
    if ((rc = run_gray_planes_ragged(c, plan, gray, X))) return rc;
    if (c->planes_done) HIP_TRY(hipEventRecord(c->planes_done, c->stream)); // the image bytes are not read again
    return init_then_bcd64(c, X, plan.t, bcd, sign, LRF_GRAM_EXP_FROM_DATA, U, V);
}

int lrf_qmf_encode_gray_ragged_u8(lrf_ctx* c, int64_t n, const lrf_gray_encode_image* images, const uint8_t* gray, int64_t gray_len, int K, int lo,
                                  int hi, const int8_t* sign, int64_t sign_len, int8_t* U, int64_t u_len, int8_t* V, int64_t v_len)
{
    if (!c || !images || !gray || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    // the sweep with one candidate per image, in image order
    std::vector<lrf_gray_sweep_image> ims((size_t)n);
    std::vector<lrf_gray_sweep_candidate> cds((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const lrf_gray_encode_image& im = images[i];
        ims[(size_t)i] = lrf_gray_sweep_image{im.H, im.W, im.gray_off, im.sign_off};
        cds[(size_t)i] = lrf_gray_sweep_candidate{(int32_t)i, im.R, im.u_off, im.v_off};
    }
    return lrf_qmf_encode_gray_ragged_sweep_u8(c, n, ims.data(), n, cds.data(), gray, gray_len, K, lo, hi, sign, sign_len, U, u_len, V, v_len);
}

int lrf_qmf_sse_gray_ragged_u8(lrf_ctx* c, int64_t n, const lrf_gray_image* items, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                               const uint8_t* gray, int64_t gray_len, uint64_t* sse)
{
    if (!c || !items || !U || !V || !gray || !sse) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    if (gray_len < 0) return set_err(LRF_EINVAL, "gray_len=%ld is negative", (long)gray_len);
    std::vector<GrayDesc> descs;
    // (scale 1 with gray_len as the output's length: out_off and the item's [H][W] are checked against the buffer the SOURCE is read from)
    const GrayRefusal r = describe_gray_images(n, items, u_len, v_len, 1, gray_len, descs);
    if (r.check == GDESC_OUT) return set_err(LRF_EINVAL, "item %ld: its source leaves the buffer of %ld bytes", (long)r.image, (long)r.a);
    int rc = r.check == GDESC_OK ? LRF_OK : gray_describe(n, items, u_len, v_len, 1, gray_len, descs);
    if (rc) return rc;
    std::vector<GrayItem> its((size_t)n);
    for (int64_t i = 0; i < n; i++)
        its[(size_t)i] = GrayItem{(int)i, 1, 0, 0, (int)items[i].H, (int)items[i].W, 0, (int)i, (long)items[i].out_off, (long)items[i].W};
    const GrayPlan plan = plan_gray_windows(descs, its);
    if (plan.too_many) return set_err(LRF_ENOTSUP, "%ld workgroups in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    if ((rc = keep_resident(c, c->gray_desc, c->gray_desc_key, descs.data(), descs.size() * sizeof(GrayDesc)))) return rc;
    const GrayDesc* d_desc = (const GrayDesc*)c->gray_desc.p;
    Prof p(c, LRF_K_DECODE);
    if ((rc = stage_crop_bytes(c, plan.table.data(), plan.table.size() * sizeof(GrayItem)))) return rc;
    const GrayItem* d_item = (const GrayItem*)c->crop_tab.p;
    HIP_TRY(hipMemsetAsync(sse, 0, (size_t)n * sizeof(uint64_t), c->stream));
    for (const GrayLaunch& l : plan.launches) { // (whole images at level 1: one launch)
        hipLaunchKernelGGL(k_gray_sse, dim3((unsigned)(l.nitems * l.wgs)), dim3(256), 0, c->stream, U, V, gray, d_desc, d_item + l.item0, (int)l.wgs,
                           (unsigned long long*)sse);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

} // extern "C"
