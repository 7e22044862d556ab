// lrf_gray_loader_host.inc — the host side of the gray loader (lrf_qmf_decode_gray_ragged_u8, lrf_qmf_decode_gray_crops_u8,
// lrf_qmf_decode_gray_resized_crops_u8 and the _tensor forms; kernels: lrf_gray_loader_kernel.hip; the image list and the
// launches: describe_gray_images, plan_gray_windows, plan_gray_resized in lrf_plan.cpp).  Included by lrf_channels.hip.
// Everything the kernels index with is checked here, before any launch.  The image descriptors stay resident in a table of
// their own (lrf_ctx::gray_desc, keyed on their bytes); the item list of a call travels through the pinned staging slots of
// the colour crops (stage_crop_bytes: no stream wait).

// describe_gray_images with its refusal worded
static int gray_describe(int64_t n, const lrf_gray_image* images, int64_t u_len, int64_t v_len, int scale, int64_t out_len, std::vector<GrayDesc>& descs)
{
    const GrayRefusal r = describe_gray_images(n, images, u_len, v_len, scale, out_len, descs);
    const long i = (long)r.image;
    switch (r.check) {
    case GDESC_OK: return LRF_OK;
    case GDESC_SIZE: return set_err(LRF_EINVAL, "image %ld: size %ldx%ld: sides in [1,2^20] and fewer than 2^31 pixels expected", i, (long)r.a, (long)r.b);
    case GDESC_GEOM: return set_err(LRF_EINVAL, "image %ld: reflect padding larger than the image (%ldx%ld, patches 8x8)", i, (long)r.a, (long)r.b);
    case GDESC_RANK: return set_err(LRF_EINVAL, "image %ld: rank %ld out of range [1,%d]", i, (long)r.a, LRF_GRAY_DEC_MAX_RANK);
    case GDESC_NEGATIVE: return set_err(LRF_EINVAL, "image %ld: negative offset", i);
    case GDESC_U: return set_err(LRF_EINVAL, "image %ld: its U factor leaves the buffer of %ld elements", i, (long)r.a);
    case GDESC_V: return set_err(LRF_EINVAL, "image %ld: its V factor leaves the buffer of %ld elements", i, (long)r.a);
    default: return set_err(LRF_EINVAL, "image %ld: its output leaves the buffer of %ld bytes", i, (long)r.a);
    }
}

static bool gray_scale_ok(int f) { return f == 1 || f == 2 || f == 4 || f == 8; }

// the launches of a window plan (whole images and crops)
static int run_gray_windows(lrf_ctx* c, const std::vector<GrayDesc>& descs, const std::vector<GrayItem>& items, const int8_t* U, const int8_t* V,
                            const DecodeOut& o)
{
    const GrayPlan plan = plan_gray_windows(descs, items);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld workgroups in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    int rc = keep_resident(c, c->gray_desc, c->gray_desc_key, descs.data(), descs.size() * sizeof(GrayDesc));
    if (rc) return rc;
    const GrayDesc* d_desc = (const GrayDesc*)c->gray_desc.p;
    Prof p(c, LRF_K_DECODE);
    if ((rc = stage_crop_bytes(c, plan.table.data(), plan.table.size() * sizeof(GrayItem)))) return rc;
    const GrayItem* d_item = (const GrayItem*)c->crop_tab.p;
    for (const GrayLaunch& l : plan.launches) {
        const dim3 grid((unsigned)(l.nitems * l.wgs));
        const GrayItem* it = d_item + l.item0;
        if (o.dtype >= 0)
            with_tensor_type(o, [&](auto* out) {
                using T = std::remove_pointer_t<decltype(out)>;
                if (l.f == 1) hipLaunchKernelGGL(k_gray_window1_t<T>, grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, it, (int)l.wgs);
                else hipLaunchKernelGGL(k_gray_windowf_t<T>, grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, it, (int)l.wgs);
            });
        else if (l.f == 1)
            hipLaunchKernelGGL(k_gray_window1, grid, dim3(256), 0, c->stream, U, V, (uint8_t*)o.p, d_desc, it, (int)l.wgs);
        else
            hipLaunchKernelGGL(k_gray_windowf, grid, dim3(256), 0, c->stream, U, V, (uint8_t*)o.p, d_desc, it, (int)l.wgs);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

static int gray_crops_to(lrf_ctx* c, int64_t n_images, const lrf_gray_image* images, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                         int64_t n_crops, const lrf_scaled_crop* crops, int64_t h, int64_t w, const DecodeOut& o)
{
    if (!c || !images || !U || !V || !crops || !o.p) return set_err(LRF_EINVAL, "NULL argument");
    if (n_images < 1 || n_images > 65535) return set_err(LRF_EINVAL, "n_images=%ld out of range [1,65535]", (long)n_images);
    if (n_crops < 1 || n_crops > (1 << 20)) return set_err(LRF_EINVAL, "n_crops=%ld out of range [1,2^20]", (long)n_crops);
    if (h < 1 || w < 1 || h > INT32_MAX || w > INT32_MAX) return set_err(LRF_EINVAL, "crop size %ldx%ld out of range", (long)h, (long)w);
    std::vector<GrayDesc> descs;
    int rc = gray_describe(n_images, images, u_len, v_len, 0, 0, descs);
    if (rc) return rc;
    // (h <= len / w first: then h w cannot wrap)
    if (o.len < 1 || h > o.len / w || n_crops > o.len / (h * w))
        return set_err(LRF_EINVAL, "%ld crops of %ldx%ld leave the output buffer of %ld elements", (long)n_crops, (long)h, (long)w, (long)o.len);
    std::vector<GrayItem> items((size_t)n_crops);
    for (int64_t j = 0; j < n_crops; j++) {
        const lrf_scaled_crop& cr = crops[j];
        if (cr.image < 0 || cr.image >= n_images) return set_err(LRF_EINVAL, "crop %ld: image %d out of range [0,%ld)", (long)j, cr.image, (long)n_images);
        if (!gray_scale_ok(cr.scale)) return set_err(LRF_EINVAL, "crop %ld: scale %d: 1, 2, 4 or 8 expected", (long)j, cr.scale);
        const lrf_gray_image& im = images[cr.image];
        const int64_t Hs = scaled_dim(im.H, cr.scale), Ws = scaled_dim(im.W, cr.scale);
        if (cr.y0 < 0 || cr.x0 < 0 || h > Hs || w > Ws || cr.y0 > Hs - h || cr.x0 > Ws - w)
            return set_err(LRF_EINVAL, "crop %ld: %ldx%ld at (%d,%d) leaves image %d of %ldx%ld at scale 1/%d", (long)j, (long)h, (long)w, cr.y0, cr.x0,
                           cr.image, (long)Hs, (long)Ws, cr.scale);
        items[(size_t)j] = GrayItem{cr.image, cr.scale, cr.y0, cr.x0, (int)h, (int)w, 0, (int)j, (long)(j * h * w), (long)w};
    }
    return run_gray_windows(c, descs, items, U, V, o);
}

static int gray_resized_to(lrf_ctx* c, int64_t n_images, const lrf_gray_image* images, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                           int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow, const DecodeOut& o)
{
    if (!c || !images || !U || !V || !crops || !o.p) return set_err(LRF_EINVAL, "NULL argument");
    if (n_images < 1 || n_images > 65535) return set_err(LRF_EINVAL, "n_images=%ld out of range [1,65535]", (long)n_images);
    if (n_crops < 1 || n_crops > (1 << 20)) return set_err(LRF_EINVAL, "n_crops=%ld out of range [1,2^20]", (long)n_crops);
    if (oh < 1 || ow < 1 || oh > 16384 || ow > 16384) return set_err(LRF_EINVAL, "output size %ldx%ld out of range [1,16384]", (long)oh, (long)ow);
    std::vector<GrayDesc> descs;
    int rc = gray_describe(n_images, images, u_len, v_len, 0, 0, descs);
    if (rc) return rc;
    // (oh ow <= 2^28 and n_crops <= 2^20: oh ow n_crops cannot wrap)
    if (o.len < 1 || n_crops > o.len / (oh * ow))
        return set_err(LRF_EINVAL, "%ld crops of %ldx%ld leave the output buffer of %ld elements", (long)n_crops, (long)oh, (long)ow, (long)o.len);
    std::vector<GrayItem> boxes((size_t)n_crops);
    for (int64_t j = 0; j < n_crops; j++) {
        const lrf_resized_crop& cr = crops[j];
        if (cr.image < 0 || cr.image >= n_images) return set_err(LRF_EINVAL, "crop %ld: image %d out of range [0,%ld)", (long)j, cr.image, (long)n_images);
        const lrf_gray_image& im = images[cr.image];
        if (cr.h < 1 || cr.w < 1) return set_err(LRF_EINVAL, "crop %ld: box of %dx%d: both sides must be >= 1", (long)j, cr.h, cr.w);
        if (cr.y0 < 0 || cr.x0 < 0 || cr.h > im.H || cr.w > im.W || cr.y0 > im.H - cr.h || cr.x0 > im.W - cr.w)
            return set_err(LRF_EINVAL, "crop %ld: %dx%d at (%d,%d) leaves image %d of %ldx%ld", (long)j, cr.h, cr.w, cr.y0, cr.x0, cr.image, (long)im.H,
                           (long)im.W);
        boxes[(size_t)j] = GrayItem{cr.image, 1, cr.y0, cr.x0, cr.h, cr.w, cr.flip != 0, (int)j, 0, 0};
    }
    const GrayPlan plan = plan_gray_resized(boxes, (int)oh, (int)ow);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld workgroups in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    if ((rc = keep_resident(c, c->gray_desc, c->gray_desc_key, descs.data(), descs.size() * sizeof(GrayDesc)))) return rc;
    const GrayDesc* d_desc = (const GrayDesc*)c->gray_desc.p;
    Prof p(c, LRF_K_DECODE);
    if ((rc = stage_crop_bytes(c, plan.table.data(), plan.table.size() * sizeof(GrayItem)))) return rc;
    const GrayItem* d_item = (const GrayItem*)c->crop_tab.p;
    for (const GrayLaunch& l : plan.launches) {
        const dim3 grid((unsigned)(l.nitems * l.wgs));
        const GrayItem* it = d_item + l.item0;
        if (o.dtype >= 0)
            with_tensor_type(o, [&](auto* out) {
                using T = std::remove_pointer_t<decltype(out)>;
                if (l.direct) hipLaunchKernelGGL(k_gray_resized_direct_t<T>, grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, it, (int)oh, (int)ow, (int)l.wgs);
                else hipLaunchKernelGGL(k_gray_resized_t<T>, grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, it, (int)oh, (int)ow, (int)l.wgs);
            });
        else if (l.direct)
            hipLaunchKernelGGL(k_gray_resized_direct, grid, dim3(256), 0, c->stream, U, V, (uint8_t*)o.p, d_desc, it, (int)oh, (int)ow, (int)l.wgs);
        else
            hipLaunchKernelGGL(k_gray_resized, grid, dim3(256), 0, c->stream, U, V, (uint8_t*)o.p, d_desc, it, (int)oh, (int)ow, (int)l.wgs);
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

extern "C" {

int lrf_qmf_decode_gray_ragged_u8(lrf_ctx* c, int64_t n, const lrf_gray_image* images, int scale, const int8_t* U, int64_t u_len, const int8_t* V,
                                  int64_t v_len, uint8_t* out, int64_t out_len)
{
    if (!c || !images || !U || !V || !out) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > 65535) return set_err(LRF_EINVAL, "n=%ld out of range [1,65535]", (long)n);
    if (!gray_scale_ok(scale)) return set_err(LRF_EINVAL, "scale %d: 1, 2, 4 or 8 expected", scale);
    if (out_len < 0) return set_err(LRF_EINVAL, "out_len=%ld is negative", (long)out_len);
    std::vector<GrayDesc> descs;
    int rc = gray_describe(n, images, u_len, v_len, scale, out_len, descs);
    if (rc) return rc;
    std::vector<GrayItem> items((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int Hs = (int)scaled_dim(images[i].H, scale), Ws = (int)scaled_dim(images[i].W, scale);
        items[(size_t)i] = GrayItem{(int)i, scale, 0, 0, Hs, Ws, 0, (int)i, (long)images[i].out_off, (long)Ws}; // a whole image: the window (0, 0, Hs, Ws)
    }
    return run_gray_windows(c, descs, items, U, V, bytes_out(out, out_len));
}

int lrf_qmf_decode_gray_crops_u8(lrf_ctx* c, int64_t n_images, const lrf_gray_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                 int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops, int64_t h, int64_t w, uint8_t* out, int64_t out_len)
{
    return gray_crops_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, h, w, bytes_out(out, out_len));
}

int lrf_qmf_decode_gray_crops_tensor(lrf_ctx* c, int64_t n_images, const lrf_gray_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                     int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops, int64_t h, int64_t w, const lrf_tensor_format* fmt,
                                     void* out, int64_t out_bytes)
{
    DecodeOut o;
    if (int rc = tensor_out(fmt, out, out_bytes, &o)) return rc;
    return gray_crops_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, h, w, o);
}

int lrf_qmf_decode_gray_resized_crops_u8(lrf_ctx* c, int64_t n_images, const lrf_gray_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                         int64_t v_len, int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow, uint8_t* out,
                                         int64_t out_len)
{
    return gray_resized_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, oh, ow, bytes_out(out, out_len));
}

int lrf_qmf_decode_gray_resized_crops_tensor(lrf_ctx* c, int64_t n_images, const lrf_gray_image* images, const int8_t* U, int64_t u_len,
                                             const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow,
                                             const lrf_tensor_format* fmt, void* out, int64_t out_bytes)
{
    DecodeOut o;
    if (int rc = tensor_out(fmt, out, out_bytes, &o)) return rc;
    return gray_resized_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, oh, ow, o);
}

} // extern "C"
