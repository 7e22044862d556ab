// lrf_decode_tensor_host.inc — the host side of the entries that write a model's tensor (lrf_qmf_decode_crops_tensor,
// lrf_qmf_decode_scaled_crops_tensor, lrf_qmf_decode_resized_crops_tensor; the epilogue: lrf_decode_tensor_kernel.hip).  Included by
// lrf_encode8.hip last: an entry checks its format and hands the body of its _rgb_u8 counterpart (decode_crops_to,
// decode_scaled_crops_to, decode_resized_to) a DecodeOut that names the tensor, so every other check, the launch plan, the
// resident descriptors and the staging slots are that entry's own code.

// fmt, out, out_bytes -> the output in elements; everything is checked before the body sees it
int tensor_out(const lrf_tensor_format* fmt, void* out, int64_t out_bytes, DecodeOut* o)
{
    if (!fmt || !out) return set_err(LRF_EINVAL, "NULL argument");
    if (fmt->dtype != LRF_T_F32 && fmt->dtype != LRF_T_F16 && fmt->dtype != LRF_T_BF16)
        return set_err(LRF_EINVAL, "tensor format: dtype %d: LRF_T_F32, LRF_T_F16 or LRF_T_BF16 expected", fmt->dtype);
    if (fmt->layout != LRF_T_NCHW && fmt->layout != LRF_T_NHWC)
        return set_err(LRF_EINVAL, "tensor format: layout %d: LRF_T_NCHW or LRF_T_NHWC expected", fmt->layout);
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(fmt->scale[k]) || !std::isfinite(fmt->bias[k]))
            return set_err(LRF_EINVAL, "tensor format: scale and bias of channel %d must be finite", k);
    const int64_t es = fmt->dtype == LRF_T_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(out) % (uintptr_t)es) return set_err(LRF_EINVAL, "the output is not aligned to its %ld-byte elements", (long)es);
    if (out_bytes < 0) return set_err(LRF_EINVAL, "out_bytes=%ld is negative", (long)out_bytes);
    // (whole elements: n 3 h w elements fit iff n 3 h w <= floor(out_bytes / es), which the bodies check without wrapping)
    *o = DecodeOut{out, out_bytes / es, fmt->dtype,
                   TensorFmt{{fmt->scale[0], fmt->scale[1], fmt->scale[2]}, {fmt->bias[0], fmt->bias[1], fmt->bias[2]}, fmt->layout == LRF_T_NHWC}};
    return LRF_OK;
}

int lrf_qmf_decode_crops_tensor(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                int64_t v_len, int64_t n_crops, const lrf_crop* crops, int64_t h, int64_t w, const lrf_tensor_format* fmt, void* out,
                                int64_t out_bytes)
{
    DecodeOut o;
    if (int rc = tensor_out(fmt, out, out_bytes, &o)) return rc;
    return decode_crops_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, h, w, o);
}

int lrf_qmf_decode_scaled_crops_tensor(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                       int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops, int64_t h, int64_t w, const lrf_tensor_format* fmt,
                                       void* out, int64_t out_bytes)
{
    DecodeOut o;
    if (int rc = tensor_out(fmt, out, out_bytes, &o)) return rc;
    return decode_scaled_crops_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, h, w, o);
}

int lrf_qmf_decode_resized_crops_tensor(lrf_ctx* c, int64_t n_images, const lrf_ragged_image* images, const int8_t* U, int64_t u_len, const int8_t* V,
                                        int64_t v_len, int64_t n_crops, const lrf_resized_crop* crops, int64_t oh, int64_t ow,
                                        const lrf_tensor_format* fmt, void* out, int64_t out_bytes)
{
    DecodeOut o;
    if (int rc = tensor_out(fmt, out, out_bytes, &o)) return rc;
    return decode_resized_to(c, n_images, images, U, u_len, V, v_len, n_crops, crops, oh, ow, o);
}
