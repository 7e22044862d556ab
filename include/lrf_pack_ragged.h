/*
 * lrf_pack_ragged.h — the part of liblrf_pack.so's C ABI that packs and unpacks streams differing in size and ranks; included by lrf_pack.h.
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

/*
 * What lrf_pack_qmf_streams does, for n images that differ in size and ranks (the output of lrf_qmf_encode_ragged_rgb_u8): image b has
 * M[3 b + c] rows and R[3 b + c] columns in plane c, its factors start at U + u_off[b] and V + v_off[b] of two flat host buffers
 * of u_len / v_len int8 elements, each laid out as lrf_qmf_encode_rgb_u8 writes one image, and its stream opens with the
 * metadata_len[b] bytes at metadata[b].  All columns of all images deflate (zlib level 9) on the host threads together; stream b
 * is byte for byte what lrf_pack_qmf_streams gives for that image alone.  out[b] is malloc'ed (lrf_pack_free), out_len[b] its
 * length.  Every length and range is checked as lrf_pack_unpack_qmf_factors_ragged checks them, before anything is read.
 * Returns 0; -6 for anything inconsistent (a NULL pointer, n < 1, M or R < 1, M x R beyond the buffer, a range that leaves
 * its buffer); -5 zlib failure; -4 out of memory.
 */
int lrf_pack_qmf_streams_ragged(const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len, int64_t n, const int64_t* M /* [n][3] */,
                                const int* R /* [n][3] */, const int64_t* u_off, const int64_t* v_off, const char* const* metadata,
                                const int64_t* metadata_len, int threads, uint8_t** out, int64_t* out_len);
#ifdef __cplusplus
}
#endif
#endif
