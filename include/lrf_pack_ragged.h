/*
 * lrf_pack_ragged.h — the part of liblrf_pack.so's C ABI that unpacks streams differing in size and ranks; included by lrf_pack.h.
 */
#ifndef LRF_PACK_RAGGED_H
#define LRF_PACK_RAGGED_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/*
 * What lrf_pack_unpack_qmf_factors does, for n streams that differ in size and ranks (the input of lrf_qmf_decode_ragged_rgb_u8): stream b has M[3 b + c] rows
 * and R[3 b + c] columns in plane c, and its factors go to U + u_off[b] and V + v_off[b] of two flat buffers of u_len / v_len
 * int8 elements, each laid out as that function writes one image.  All columns of all streams inflate on the host threads together.  Every length is
 * checked against the blob and against (M, R), every range against its buffer.  Returns 0; -1 bad argument (a range that leaves
 * its buffer included); -6 when a blob is not exactly the int8 / per-column layout.
 */
int lrf_pack_unpack_qmf_factors_ragged(const uint8_t* const* factor_blobs, const int64_t* blob_len, int64_t n, const int64_t* M /* [n][3] */,
                                       const int* R /* [n][3] */, const int64_t* u_off, const int64_t* v_off, int threads, int8_t* U,
                                       int64_t u_len, int8_t* V, int64_t v_len);
#ifdef __cplusplus
}
#endif
#endif
