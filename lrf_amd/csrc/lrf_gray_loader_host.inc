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
    const WindowCall k = {n_images, n_crops, h, w, false, LRF_WIN_SCALES_GRAY, 1, o.len};
    int rc = check_crop_call(!c || !images || !U || !V || !crops || !o.p, k);
    if (rc) return rc;
    std::vector<GrayDesc> descs;
    if ((rc = gray_describe(n_images, images, u_len, v_len, 0, 0, descs))) return rc;
    std::vector<GrayItem> items;
    if ((rc = checked_windows(k, descs, crops, items))) return rc;
    return run_gray_windows(c, descs, items, U, V, o);
}

static int gray_resized_to(lrf_ctx* c, int64_t n_images, const lrf_gray_image* images, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                           int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow, const DecodeOut& o)
{
    const WindowCall k = {n_images, n_crops, oh, ow, true, 0, 1, o.len};
    int rc = check_crop_call(!c || !images || !U || !V || !crops || !o.p, k);
    if (rc) return rc;
    std::vector<GrayDesc> descs;
    if ((rc = gray_describe(n_images, images, u_len, v_len, 0, 0, descs))) return rc;
    std::vector<GrayItem> boxes;
    if ((rc = checked_windows(k, descs, crops, boxes))) return rc;
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
