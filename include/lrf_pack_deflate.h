/*
 * lrf_pack_deflate.h — the part of liblrf_pack.so's C ABI that belongs to the Huffman-only deflate coder of factor columns
 * (lrf_amd/csrc/lrf_deflate_shared.h defines the format); included by lrf_pack.h.
 */
#ifndef LRF_PACK_DEFLATE_H
#define LRF_PACK_DEFLATE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the most a stream of `len` bytes can take (stored blocks): 2 + 5 * ceil(len / 65535) + len + 4; -1 for len < 1 */
int64_t lrf_pack_deflate_bound(int64_t len);

/*
 * The host restatement of the device coder (lrf_deflate_columns_i8 of liblrf_hip.so), serial, over the same shared header: the
 * zlib stream of the `rows` bytes src[0], src[stride], src[2 stride], ... written to dst.  Returns the stream's length; -1 for
 * a bad argument (NULL, rows outside [1, 2^30], stride < 1); -7 when the stream would not fit `cap` bytes.  No byte of dst
 * behind the returned length is written (nothing at all on an error).  The device call gives these bytes for the same column.
 */
int64_t lrf_pack_deflate_column_i8(const int8_t* src, int64_t rows, int64_t stride, uint8_t* dst, int64_t cap);

/*
 * The length lrf_pack_deflate_column_i8 would return for the same column (cap large enough), from the column's byte counts alone:
 * no stream is written.  The CPU-testable definition of what lrf_deflate_sizes_i8 of liblrf_hip.so counts on the device.
 * Returns -1 for a bad argument (NULL, rows outside [1, 2^30], stride < 1).
 */
int64_t lrf_pack_deflate_size_column_i8(const int8_t* src, int64_t rows, int64_t stride);

/*
 * What lrf_pack_qmf_streams_ragged does, from columns that are deflated already: image b of n has M[3 b + c] rows and
 * R[3 b + c] columns in plane c and its stream opens with the metadata_len[b] bytes at metadata[b]; its columns — those of
 * u_Y, v_Y, u_Cb, v_Cb, u_Cr, v_Cr in this order, the images in call order, `ncols` in all — are the col_len[k] bytes at
 * slots + col_off[k] of a host buffer of slots_len bytes.  Same JSON headers, same combine_bytes fold, same factor order as the
 * ragged packer: only the payload of a column is copied instead of deflated.  Before anything is read or written every offset
 * and length is checked against the buffer, ncols against the ranks, and the column ranges against each other (none may
 * overlap).  out[b] is malloc'ed (lrf_pack_free), out_len[b] its length.  threads <= 0: one per hardware thread, at most 64.
 * Returns 0; -6 for anything inconsistent (out and out_len are then untouched); -4 out of memory.
 */
int lrf_pack_qmf_streams_deflated(const uint8_t* slots, int64_t slots_len, int64_t n, const int64_t* M /* [n][3] */,
                                  const int* R /* [n][3] */, const int64_t* col_off, const int32_t* col_len, int64_t ncols,
                                  const char* const* metadata, const int64_t* metadata_len, int threads, uint8_t** out,
                                  int64_t* out_len);
#ifdef __cplusplus
}
#endif
#endif
