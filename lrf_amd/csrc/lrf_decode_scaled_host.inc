// lrf_decode_scaled_host.inc — the host side of the decode at 1/2, 1/4, 1/8 scale (lrf_qmf_decode_scaled_rgb_u8,
// lrf_qmf_decode_scaled_crops_rgb_u8; kernels: lrf_decode_scaled_kernel.hip; the launches: plan_decode_scaled).  Included by
// lrf_encode8.hip: the entries share decode_plan, the descriptor table and the staging slots of the decode of windows.

int lrf_scaled_dims(int64_t H, int64_t W, int scale, int64_t* Hs, int64_t* Ws)
{
    if (!Hs || !Ws) return set_err(LRF_EINVAL, "NULL argument");
    if (!scaled_f_ok(scale)) return set_err(LRF_EINVAL, "scale %d: 2, 4 or 8 expected", scale);
    if (H < 1 || W < 1 || H > INT32_MAX || W > INT32_MAX) return set_err(LRF_EINVAL, "size %ldx%ld out of range", (long)H, (long)W);
    *Hs = scaled_dim(H, scale);
    *Ws = scaled_dim(W, scale);
    return LRF_OK;
}

// The images of a call: validated exactly as lrf_qmf_decode_crops_rgb_u8 validates them, and described by the same bytes (the two
// entries share the resident descriptor table: a loader that mixes full-scale and scaled windows of one list uploads it once).
static int scaled_images(int64_t n_images, const lrf_ragged_image* images, int64_t u_len, int64_t v_len, std::vector<RaggedDesc>& descs,
                         std::vector<ScaledImage>& simg)
{
    descs.resize((size_t)n_images);
    simg.resize((size_t)n_images);
    memset((void*)descs.data(), 0, descs.size() * sizeof(RaggedDesc)); // (the bytes are the table's key: padding included)
    for (int64_t i = 0; i < n_images; i++) {
        const lrf_ragged_image& im = images[i];
        RaggedDesc& d = descs[(size_t)i];
        if (im.H < 1 || im.W < 1 || im.H > INT32_MAX || im.W > INT32_MAX) return set_err(LRF_EINVAL, "image %ld: size %ldx%ld out of range", (long)i, (long)im.H, (long)im.W);
        int rc = make_geom(im.H, im.W, &d.g);
        if (rc) return rc;
        for (int ch = 0; ch < 3; ch++)
            if (im.R[ch] < 1 || im.R[ch] > 64) return set_err(LRF_EINVAL, "image %ld: rank %d out of range", (long)i, im.R[ch]);
        if (im.u_off < 0 || im.v_off < 0) return set_err(LRF_EINVAL, "image %ld: negative offset", (long)i);
        long u_img = 0, v_img = 0;
        for (int ch = 0; ch < 3; ch++) {
            u_img += (long)d.g.p[ch].M * im.R[ch];
            v_img += 64L * im.R[ch];
        }
        // (every term is checked against the length before it is added to an offset: no sum can wrap)
        if (u_img > u_len || im.u_off > u_len - u_img) return set_err(LRF_EINVAL, "image %ld: its U factors leave the buffer of %ld elements", (long)i, (long)u_len);
        if (v_img > v_len || im.v_off > v_len - v_img) return set_err(LRF_EINVAL, "image %ld: its V factors leave the buffer of %ld elements", (long)i, (long)v_len);
        const DecodePlan plan = decode_plan(d.g, im.H, im.W, im.R, true);
        d.u_off = im.u_off; d.v_off = im.v_off;
        d.H = (int)im.H; d.W = (int)im.W;
        d.R0 = im.R[0]; d.R1 = im.R[1]; d.R2 = im.R[2];
        d.kind = plan.kind; d.cls = plan.cls;
        d.per_strip = (d.g.p[0].nw + 31) / 32;
        simg[(size_t)i] = ScaledImage{plan.kind == DEC_TILE16, plan.cls, {im.R[0], im.R[1], im.R[2]}};
    }
    return LRF_OK;
}

// items: validated.  The descriptors stay resident under their bytes; the sorted items and the pool jobs travel together
// through the pinned slots of the decode of windows, stream-ordered.
static int run_scaled(lrf_ctx* c, const std::vector<RaggedDesc>& descs, const std::vector<ScaledImage>& simg, const std::vector<ScaledItem>& items,
                      const int8_t* U, const int8_t* V, uint8_t* rgb)
{
    const ScaledPlan plan = plan_decode_scaled(simg, items);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld workgroups in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    const size_t db = descs.size() * sizeof(RaggedDesc);
    if (c->crop_desc_key.size() != db || memcmp(c->crop_desc_key.data(), descs.data(), db) != 0 || !c->crop_desc.p) {
        c->crop_desc_key.clear();
        int rc = upload(c, c->crop_desc, descs.data(), db);
        if (rc) return rc;
        c->crop_desc_key.assign((const char*)descs.data(), (const char*)descs.data() + db);
    }
    const RaggedDesc* d_desc = (const RaggedDesc*)c->crop_desc.p;
    Prof p(c, LRF_K_DECODE);
    const size_t ib = plan.table.size() * sizeof(ScaledItem), jb = plan.jobs.size() * sizeof(ScaledPoolJob);
    std::vector<char> tab(ib + jb);
    memcpy(tab.data(), plan.table.data(), ib);
    if (jb) memcpy(tab.data() + ib, plan.jobs.data(), jb);
    int rc = stage_crop_bytes(c, tab.data(), tab.size());
    if (rc) return rc;
    const ScaledItem* d_item = (const ScaledItem*)c->crop_tab.p;
    const ScaledPoolJob* d_job = (const ScaledPoolJob*)((const char*)c->crop_tab.p + ib);
    if (!plan.jobs.empty()) {
        rc = ensure(c, c->scaled_pool, (size_t)plan.pool_elems * sizeof(int16_t));
        if (rc) return rc;
        hipLaunchKernelGGL(k_pool_v, dim3((unsigned)plan.jobs.size()), dim3(256), 0, c->stream, V, (int16_t*)c->scaled_pool.p, d_desc, d_job);
        LAUNCH_CHECK();
    }
    const int16_t* pool = (const int16_t*)c->scaled_pool.p;
    for (const ScaledLaunch& l : plan.launches) {
        const dim3 grid((unsigned)(l.nitems * l.wgs));
        const ScaledItem* it = d_item + l.item0;
        if (!l.tiled)
            hipLaunchKernelGGL(k_decode_scaled_any, grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, it, (int)l.wgs);
        else {
#define LRF_SCALED_TILED(F, CLS) hipLaunchKernelGGL((k_decode_scaled_tiled<F, CLS>), grid, dim3(256), 0, c->stream, U, pool, rgb, d_desc, it, (int)l.wgs)
#define LRF_SCALED_CLASSES(F)                   \
    switch (l.cls) {                            \
    case 0: LRF_SCALED_TILED(F, 0); break;      \
    case 1: LRF_SCALED_TILED(F, 1); break;      \
    case 2: LRF_SCALED_TILED(F, 2); break;      \
    case 3: LRF_SCALED_TILED(F, 3); break;      \
    default: LRF_SCALED_TILED(F, 4); break;     \
    }
            if (l.f == 2) { LRF_SCALED_CLASSES(2) }
            else if (l.f == 4) { LRF_SCALED_CLASSES(4) }
            else { LRF_SCALED_CLASSES(8) }
#undef LRF_SCALED_CLASSES
#undef LRF_SCALED_TILED
        }
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

int lrf_qmf_decode_scaled_rgb_u8(lrf_ctx* c, int64_t n, const lrf_ragged_image* images, int scale, const int8_t* U, int64_t u_len, const int8_t* V,
                                 int64_t v_len, uint8_t* rgb, int64_t rgb_len)
{
    if (!c || !images || !U || !V || !rgb) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    if (!scaled_f_ok(scale)) return set_err(LRF_EINVAL, "scale %d: 2, 4 or 8 expected", scale);
    std::vector<RaggedDesc> descs;
    std::vector<ScaledImage> simg;
    int rc = scaled_images(n, images, u_len, v_len, descs, simg);
    if (rc) return rc;
    std::vector<ScaledItem> items((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const lrf_ragged_image& im = images[i];
        const int64_t hs = scaled_dim(im.H, scale), ws = scaled_dim(im.W, scale);
        if (im.rgb_off < 0) return set_err(LRF_EINVAL, "image %ld: negative offset", (long)i);
        if (rgb_len < 3 || hs * ws > rgb_len / 3 || im.rgb_off > rgb_len - 3 * hs * ws)
            return set_err(LRF_EINVAL, "image %ld: its output of 3x%ldx%ld leaves the buffer of %ld bytes", (long)i, (long)hs, (long)ws, (long)rgb_len);
        items[(size_t)i] = ScaledItem{(int)i, scale, 0, 0, (int)hs, (int)ws, (int)i, 0, im.rgb_off, 0};
    }
    return run_scaled(c, descs, simg, items, U, V, rgb);
}

int lrf_qmf_decode_scaled_crops_rgb_u8(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                       int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops, int64_t h, int64_t w, uint8_t* rgb, int64_t rgb_len)
{
    if (!c || !images || !U || !V || !crops || !rgb) return set_err(LRF_EINVAL, "NULL argument");
    if (n_images < 1 || n_images > 65535) return set_err(LRF_EINVAL, "n_images=%ld out of range [1,65535]", (long)n_images);
    if (n_crops < 1 || n_crops > (1 << 20)) return set_err(LRF_EINVAL, "n_crops=%ld out of range [1,2^20]", (long)n_crops);
    if (h < 1 || w < 1 || h > INT32_MAX || w > INT32_MAX) return set_err(LRF_EINVAL, "crop size %ldx%ld out of range", (long)h, (long)w);
    std::vector<RaggedDesc> descs;
    std::vector<ScaledImage> simg;
    int rc = scaled_images(n_images, images, u_len, v_len, descs, simg);
    if (rc) return rc;
    // (h * w <= rgb_len / 3 first: then 3 h w cannot wrap)
    if (rgb_len < 3 || h > rgb_len / 3 / w || n_crops > rgb_len / (3 * h * w))
        return set_err(LRF_EINVAL, "%ld crops of 3x%ldx%ld leave the output buffer of %ld bytes", (long)n_crops, (long)h, (long)w, (long)rgb_len);
    std::vector<ScaledItem> items((size_t)n_crops);
    for (int64_t j = 0; j < n_crops; j++) {
        const lrf_scaled_crop& cr = crops[j];
        if (cr.image < 0 || cr.image >= n_images) return set_err(LRF_EINVAL, "crop %ld: image %d out of range [0,%ld)", (long)j, cr.image, (long)n_images);
        if (!scaled_f_ok(cr.scale)) return set_err(LRF_EINVAL, "crop %ld: scale %d: 2, 4 or 8 expected", (long)j, cr.scale);
        const lrf_ragged_image& im = images[cr.image];
        const int64_t hs = scaled_dim(im.H, cr.scale), ws = scaled_dim(im.W, cr.scale);
        if (cr.y0 < 0 || cr.x0 < 0 || h > hs || w > ws || cr.y0 > hs - h || cr.x0 > ws - w)
            return set_err(LRF_EINVAL, "crop %ld: %ldx%ld at (%d,%d) leaves image %d of %ldx%ld at scale 1/%d", (long)j, (long)h, (long)w, cr.y0, cr.x0, cr.image,
                           (long)hs, (long)ws, cr.scale);
        items[(size_t)j] = ScaledItem{cr.image, cr.scale, cr.y0, cr.x0, (int)h, (int)w, (int)j, 0, 3 * h * w * j, 0};
    }
    return run_scaled(c, descs, simg, items, U, V, rgb);
}
