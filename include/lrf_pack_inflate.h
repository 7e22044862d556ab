/*
 * lrf_pack_inflate.h — the part of liblrf_pack.so's C ABI that belongs to the inflate of factor columns on the device
 * (lrf_amd/csrc/lrf_inflate_shared.h defines the decoder; lrf_inflate_columns_i8 of liblrf_hip.so runs it one lane per stream);
 * included by lrf_pack.h.
 */
#ifndef LRF_PACK_INFLATE_H
#define LRF_PACK_INFLATE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/*
 * The host restatement of the device decoder, serial, over the same shared header: the zlib stream of src_len bytes at src is
 * inflated into exactly `rows` elements dst[0], dst[stride], dst[2 stride], ...  Returns 0, or the LRFI_E_* status
 * (include/lrf_hip.h, positive) the device call reports for the same stream; -1 for a bad argument (NULL, src_len < 0, rows
 * outside [1, 2^30], stride < 1).  It allocates nothing.  Nothing outside those `rows` elements is written and no byte outside the
 * stream is read, whatever the stream holds; after an error the elements' content is unspecified.
 */
int lrf_pack_inflate_column_i8(const uint8_t* src, int64_t src_len, int8_t* dst, int64_t rows, int64_t stride);

/* The largest match distance of a stream that inflates to `rows` bytes (0: literals and stored blocks only), or minus the
 * status lrf_pack_inflate_column_i8 gives for it; -1 for a bad argument, -4 when the `rows` bytes of work space cannot be
 * allocated.  A test aid: proves that a stream really holds the matches a case is about. */
int64_t lrf_pack_inflate_max_distance(const uint8_t* src, int64_t src_len, int64_t rows);

/*
 * Where the columns' streams lie: walks the n factor blobs exactly as lrf_pack_unpack_qmf_factors_ragged does (same fold, same
 * JSON headers: num_fibers == R, mode "col", dtype "int8"; M and R as there, [n][3]) and inflates nothing.  Column k of the
 * call — the columns of u_Y, v_Y, u_Cb, v_Cb, u_Cr, v_Cr in this order, the blobs in call order, `ncols` = sum of 2 R in all —
 * is the col_len[k] bytes at factor_blobs[b] + col_off[k] of its own blob b.  Returns 0; -1 for a bad argument (NULL, n < 1,
 * M or R < 1, ncols not that sum); -6 when a blob is not exactly that layout or a column is longer than 2^31 - 1 bytes
 * (col_off and col_len are then unspecified).
 */
int lrf_pack_index_qmf_columns_ragged(const uint8_t* const* factor_blobs, const int64_t* blob_len, int64_t n, const int64_t* M /* [n][3] */,
                                      const int* R /* [n][3] */, int64_t* col_off, int32_t* col_len, int64_t ncols);
#ifdef __cplusplus
}
#endif
#endif
