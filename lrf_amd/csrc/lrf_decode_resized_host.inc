// lrf_decode_resized_host.inc — the host side of the resized crops (lrf_qmf_decode_resized_crops_rgb_u8; kernels:
// lrf_decode_resized_kernel.hip; the launches: plan_decode_resized).  Included by lrf_encode8.hip after
// lrf_decode_scaled_host.inc: the entry describes its images as the decode of windows does (describe) and shares its resident
// descriptor table and pinned staging slots.

static int decode_resized_to(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                             int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow, const DecodeOut& o)
{
    void* const rgb = o.p;
    const int64_t rgb_len = o.len;
    if (!c || !images || !U || !V || !crops || !rgb) return set_err(LRF_EINVAL, "NULL argument");
    if (n_images < 1 || n_images > 65535) return set_err(LRF_EINVAL, "n_images=%ld out of range [1,65535]", (long)n_images);
    if (n_crops < 1 || n_crops > (1 << 20)) return set_err(LRF_EINVAL, "n_crops=%ld out of range [1,2^20]", (long)n_crops);
    if (oh < 1 || ow < 1 || oh > 16384 || ow > 16384) return set_err(LRF_EINVAL, "output size %ldx%ld out of range [1,16384]", (long)oh, (long)ow);
    std::vector<RaggedDesc> descs;
    int rc = describe(n_images, images, u_len, v_len, DescribeOptions{}, "image", "output", descs);
    if (rc) return rc;
    // (oh ow <= 2^28 and n_crops <= 2^20: 3 oh ow n_crops cannot wrap)
    if (rgb_len < 3 || n_crops > rgb_len / (3 * oh * ow))
        return set_err(LRF_EINVAL, "%ld crops of 3x%ldx%ld leave the output buffer of %ld bytes", (long)n_crops, (long)oh, (long)ow, (long)rgb_len);
    std::vector<int> r8(descs.size());
    std::transform(descs.begin(), descs.end(), r8.begin(), [](const RaggedDesc& d) { return d.R0 <= 8 && d.R1 <= 8 && d.R2 <= 8; });
    std::vector<ResizedItem> list((size_t)n_crops);
    for (int64_t j = 0; j < n_crops; j++) {
        const lrf_resized_crop& cr = crops[j];
        if (cr.image < 0 || cr.image >= n_images) return set_err(LRF_EINVAL, "crop %ld: image %d out of range [0,%ld)", (long)j, cr.image, (long)n_images);
        const lrf_ragged_image& im = images[cr.image];
        if (cr.h < 1 || cr.w < 1) return set_err(LRF_EINVAL, "crop %ld: box of %dx%d: both sides must be >= 1", (long)j, cr.h, cr.w);
        if (cr.y0 < 0 || cr.x0 < 0 || cr.h > im.H || cr.w > im.W || cr.y0 > im.H - cr.h || cr.x0 > im.W - cr.w)
            return set_err(LRF_EINVAL, "crop %ld: %dx%d at (%d,%d) leaves image %d of %ldx%ld", (long)j, cr.h, cr.w, cr.y0, cr.x0, cr.image, (long)im.H,
                           (long)im.W);
        list[(size_t)j] = ResizedItem{cr.image, 1, cr.y0, cr.x0, cr.h, cr.w, cr.flip != 0, (int)j};
    }
    const ResizedPlan plan = plan_decode_resized(r8, list, (int)oh, (int)ow);
    if (plan.too_many) return set_err(LRF_EINVAL, "%ld workgroups in one launch: split the list", plan.too_many);
    LRF_ON_DEVICE(c);
    if ((rc = resident_crop_descs(c, descs))) return rc;
    const RaggedDesc* d_desc = (const RaggedDesc*)c->crop_desc.p;
    Prof p(c, LRF_K_DECODE);
    if ((rc = stage_crop_bytes(c, plan.table.data(), plan.table.size() * sizeof(ResizedItem)))) return rc;
    const ResizedItem* d_item = (const ResizedItem*)c->crop_tab.p;
    for (const ResizedLaunch& l : plan.launches) {
        const dim3 grid((unsigned)(l.nitems * l.wgs));
        const ResizedItem* it = d_item + l.item0;
#define LRF_RESIZED_ON(K, T)                                                                                                          \
    do {                                                                                                                              \
        if (l.direct) {                                                                                                               \
            if (l.f == 1) K(k_decode_resized_direct, true, T);                                                                        \
            else K(k_decode_resized_direct, false, T);                                                                                \
        } else if (l.f != 1)                                                                                                          \
            K(k_decode_resized, 2, T);                                                                                                \
        else if (l.r8)                                                                                                                \
            K(k_decode_resized, 0, T);                                                                                                \
        else                                                                                                                          \
            K(k_decode_resized, 1, T);                                                                                                \
    } while (0)
        if (o.dtype >= 0)
            with_tensor_type(o, [&](auto* out) {
                using T = std::remove_pointer_t<decltype(out)>;
#define LRF_RESIZED_T(K, A, T) hipLaunchKernelGGL((K##_t<A, T>), grid, dim3(256), 0, c->stream, U, V, out, o.f, d_desc, it, (int)oh, (int)ow, (int)l.wgs)
                LRF_RESIZED_ON(LRF_RESIZED_T, T);
#undef LRF_RESIZED_T
            });
        else {
#define LRF_RESIZED_U8(K, A, T) hipLaunchKernelGGL((K<A>), grid, dim3(256), 0, c->stream, U, V, (uint8_t*)rgb, d_desc, it, (int)oh, (int)ow, (int)l.wgs)
            LRF_RESIZED_ON(LRF_RESIZED_U8, );
#undef LRF_RESIZED_U8
        }
#undef LRF_RESIZED_ON
        LAUNCH_CHECK();
    }
    return LRF_OK;
}

int lrf_qmf_decode_resized_crops_rgb_u8(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                        int64_t v_len, int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow, uint8_t* rgb, int64_t rgb_len)
{
    return decode_resized_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, oh, ow, bytes_out(rgb, rgb_len));
}
