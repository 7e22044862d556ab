// lrf_decode_resized_host.inc — the host side of the resized crops (lrf_qmf_decode_resized_crops_rgb_u8; kernels:
// lrf_decode_resized_kernel.hip; the launches: plan_decode_resized).  Included by lrf_encode8.hip after
// lrf_decode_scaled_host.inc: the entry describes its images as the decode of windows does (describe) and shares its resident
// descriptor table and pinned staging slots.

static int decode_resized_to(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len,
                             int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow, const DecodeOut& o)
{
    void* const rgb = o.p;
    const WindowCall k = {n_images, n_crops, oh, ow, true, 0, 3, o.len};
    int rc = check_crop_call(!c || !images || !U || !V || !crops || !rgb, k);
    if (rc) return rc;
    std::vector<RaggedDesc> descs;
    if ((rc = describe(n_images, images, u_len, v_len, DescribeOptions{}, "image", "output", descs))) return rc;
    std::vector<ResizedItem> list;
    if ((rc = checked_windows(k, descs, crops, list))) return rc;
    std::vector<int> r8(descs.size());
    std::transform(descs.begin(), descs.end(), r8.begin(), [](const RaggedDesc& d) { return d.R0 <= 8 && d.R1 <= 8 && d.R2 <= 8; });
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
