// lrf_decode_scaled_host.inc — the host side of the decode at 1/2, 1/4, 1/8 scale (lrf_qmf_decode_scaled_rgb_u8,
// lrf_qmf_decode_scaled_crops_rgb_u8; kernels: lrf_decode_scaled_kernel.hip; the launches: plan_decode_scaled).  Included by
// lrf_encode8.hip: the entries share its image check (describe), the descriptor table and the staging slots of the decode of windows.

int lrf_scaled_dims(int64_t H, int64_t W, int scale, int64_t* Hs, int64_t* Ws)
{
    if (!Hs || !Ws) return set_err(LRF_EINVAL, "NULL argument");
    if (!scaled_f_ok(scale)) return set_err(LRF_EINVAL, "scale %d: 2, 4 or 8 expected", scale);
    if (H < 1 || W < 1 || H > INT32_MAX || W > INT32_MAX) return set_err(LRF_EINVAL, "size %ldx%ld out of range", (long)H, (long)W);
    *Hs = scaled_dim(H, scale);
    *Ws = scaled_dim(W, scale);
    return LRF_OK;
}

// descs: the images, described exactly as lrf_qmf_decode_crops_rgb_u8 describes them (the entries share the resident descriptor
// table: a loader that mixes full-scale and scaled windows of one list uploads it once); items: validated.  The sorted items
// and the pool jobs travel together through the pinned slots of the decode of windows, stream-ordered.
static int run_scaled(lrf_ctx* c, const std::vector<RaggedDesc>& descs, const std::vector<ScaledItem>& items, const int8_t* U, const int8_t* V, const DecodeOut& o)
{
    uint8_t* const rgb = (uint8_t*)o.p;
    std::vector<ScaledImage> simg(descs.size());
    std::transform(descs.begin(), descs.end(), simg.begin(), scaled_image_of);
    const ScaledPlan plan = plan_decode_scaled(simg, items);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld workgroups in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    int rc = resident_crop_descs(c, descs);
    if (rc) return rc;
    const RaggedDesc* d_desc = (const RaggedDesc*)c->crop_desc.p;
    Prof p(c, LRF_K_DECODE);
    const size_t ib = plan.table.size() * sizeof(ScaledItem), jb = plan.jobs.size() * sizeof(ScaledPoolJob);
    std::vector<char> tab(ib + jb);
    memcpy(tab.data(), plan.table.data(), ib);
    if (jb) memcpy(tab.data() + ib, plan.jobs.data(), jb);
    if ((rc = stage_crop_bytes(c, tab.data(), tab.size()))) return rc;
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
        if (o.dtype >= 0)
            with_tensor_type(o, [&](auto* out) {
                using T = std::remove_pointer_t<decltype(out)>;
                if (!l.tiled)
                    hipLaunchKernelGGL(k_decode_scaled_any_t<T>, grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, it, (int)l.wgs);
                else {
#define LRF_SCALED_TILED(F, CLS) \
    hipLaunchKernelGGL((k_decode_scaled_tiled_t<F, CLS, T>), grid, dim3(256), 0, c->stream, U, pool, out, o.f, d_desc, it, (int)l.wgs)
#define LRF_SCALED_2(CLS) LRF_SCALED_TILED(2, CLS)
#define LRF_SCALED_4(CLS) LRF_SCALED_TILED(4, CLS)
#define LRF_SCALED_8(CLS) LRF_SCALED_TILED(8, CLS)
                    if (l.f == 2) { LRF_FOR_DEC_CLASS(l.cls, LRF_SCALED_2) }
                    else if (l.f == 4) { LRF_FOR_DEC_CLASS(l.cls, LRF_SCALED_4) }
                    else { LRF_FOR_DEC_CLASS(l.cls, LRF_SCALED_8) }
#undef LRF_SCALED_8
#undef LRF_SCALED_4
#undef LRF_SCALED_2
#undef LRF_SCALED_TILED
                }
            });
        else if (!l.tiled)
            hipLaunchKernelGGL(k_decode_scaled_any, grid, dim3(256), 0, c->stream, U, V, rgb, d_desc, it, (int)l.wgs);
        else {
#define LRF_SCALED_TILED(F, CLS) hipLaunchKernelGGL((k_decode_scaled_tiled<F, CLS>), grid, dim3(256), 0, c->stream, U, pool, rgb, d_desc, it, (int)l.wgs)
#define LRF_SCALED_2(CLS) LRF_SCALED_TILED(2, CLS)
#define LRF_SCALED_4(CLS) LRF_SCALED_TILED(4, CLS)
#define LRF_SCALED_8(CLS) LRF_SCALED_TILED(8, CLS)
            if (l.f == 2) { LRF_FOR_DEC_CLASS(l.cls, LRF_SCALED_2) }
            else if (l.f == 4) { LRF_FOR_DEC_CLASS(l.cls, LRF_SCALED_4) }
            else { LRF_FOR_DEC_CLASS(l.cls, LRF_SCALED_8) }
#undef LRF_SCALED_8
#undef LRF_SCALED_4
#undef LRF_SCALED_2
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
    int rc = describe(n, images, u_len, v_len, DescribeOptions{}, "image", "output", descs);
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
    return run_scaled(c, descs, items, U, V, bytes_out(rgb, rgb_len));
}

static int decode_scaled_crops_to(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                  int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops, int64_t h, int64_t w, const DecodeOut& o)
{
    const WindowCall k = {n_images, n_crops, h, w, false, LRF_WIN_SCALES_COLOUR, 3, o.len};
    int rc = check_crop_call(!c || !images || !U || !V || !crops || !o.p, k);
    if (rc) return rc;
    std::vector<RaggedDesc> descs;
    if ((rc = describe(n_images, images, u_len, v_len, DescribeOptions{}, "image", "output", descs))) return rc;
    std::vector<ScaledItem> items;
    if ((rc = checked_windows(k, descs, crops, items))) return rc;
    return run_scaled(c, descs, items, U, V, o);
}

int lrf_qmf_decode_scaled_crops_rgb_u8(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                       int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops, int64_t h, int64_t w, uint8_t* rgb, int64_t rgb_len)
{
    return decode_scaled_crops_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, h, w, bytes_out(rgb, rgb_len));
}
