// lrf_internal.h — structures shared by the kernels and the host side of liblrf_hip.so.
#ifndef LRF_INTERNAL_H
#define LRF_INTERNAL_H
#include <stdint.h>

#define LRF_FAM_OF_RANK(R) ((R) <= 8 ? 0 : ((R) <= 16 ? 1 : 2)) // kernel family of a rank: k_bcd_w / k_bcd_w16 / k_bcd_w32 (+ workgroup kernels)
#define LRF_RP 16    // rank padded to one 16-wide MFMA tile (== LRF_MAX_RANK)
#define LRF_KC 384   // rows per X^T U reduction block (the reference's MKL K-blocking)

// Table layout ("gt") of b = v.mT @ v at rank pitch 16, LRF_GT_LD floats per column r, so that one column's operands are
// contiguous:  gt[r*LD + n], n < R-1 : b[j_n][r] for the j != r in increasing order (the `bb` vector of qmf.py:114);
//   gt[r*LD + 16] = 1/den[r],  gt[r*LD + 17] = den[r] = (b[r][r] + 0) + eps
#define LRF_GT_LD 20
#define LRF_GT_RDEN 16
#define LRF_GT_DEN 17
#define LRF_GT_STRIDE (LRF_RP * LRF_GT_LD)
// ranks above 16: rank pitch 64 (lrf_bigrank_kernels.hip)
#define LRF_RPB 64                      // padded rank
#define LRF_GTB_LD 68                   // gt table pitch: <= 63 `bb` entries, [64] = 1/den (unused here), [65] = den
#define LRF_GTB_DEN 65
#define LRF_GTB_STRIDE (LRF_RPB * LRF_GTB_LD)
// the exact Gram pass (lrf_gram_kernels.hip)
#define LRF_GRAM_ROWS 1536            // rows per chunk: 24 blocks of 64
#define LRF_GRAM_ROWS_FUSED 1536 // rows per Gram chunk of a plane whose partials k_planes16_gram computes
#define LRF_GRAM_PAIRS 10             // upper-triangle pairs of the four 16-column tiles
#define LRF_GRAM_SLOT (LRF_GRAM_PAIRS * 256) // 128-bit sums per partial, [pair][reg][lane]
#define LRF_GRAM_EXP_FROM_DATA (-100000)

// geometry of one colour plane of an image (lrf/compression/qmf.py:230-242)
struct PlaneGeom {
    int h, w;          // plane size (chroma: floor(H/2), floor(W/2))
    int hp, wp;        // after reflect padding to multiples of 8
    int top, left;     // pad_top / pad_left == unpad start (utils.py:127-130, :148-150)
    int top_crop, left_crop;
    int nw;            // patches per row
    int nh;            // patch rows
    int pr0;           // first patch-row index of this plane inside the image (k_planes grid)
    int M;             // number of patches
    long xoff;         // floats from the image's X base
    long o4;           // first float4 output index of this plane inside the image
};
struct ImageGeom {
    PlaneGeom p[3];
    long tot4;         // float4 outputs per image
    long img_floats;   // floats per image in X
};

// one matrix to factorise
struct PlaneDesc {
    long x_off;        // floats from the X base
    long u_off;        // elements from the U (int8) base
    long v_off;        // elements from the V (int8) base
    long u0_off;       // elements from the fp32 U0 base (init in/out)
    long v0_off;       // elements from the fp32 V0 base
    int M, R;
    int blk0, nblk;    // slots in the X^T U partial table
    int native_t2_u;   // ATen native order for `uu @ bb` in update_u: (R-1)*M < 400
    int sign_off;      // offset into the sign vector, or -1
    int gch0, ngch;    // slots in the Gram partial table (lrf_gram_kernels.hip): one per chunk of LRF_GRAM_ROWS rows
    int init_src;      // the plane whose SVD initialisation this plane takes its first R columns from: itself, or — in a sweep
                       // call (lrf_qmf_encode_sweep_rgb_u8) — the plane of the same matrix X with the call's largest rank
    int gram_fused;    // 1: a luma plane whose Gram partials the planes kernel itself computes (k_planes16_gram); k_gram64 skips it
};
struct BlockDesc {
    int plane;         // index into the PlaneDesc table
    int row0;          // first row of the block
    int blk;           // block number inside the plane
    union {
        int x_nt;      // 1: the rank <= 8 body of k_bcd_p streams the block's X source (fp32 rows or image bytes) with non-temporal
                       // loads (plan_x_residency, lrf_plan.h); 0: plain loads — every block of a call without the policy
        int pad;       // (the word's name while it was unused: comparisons of whole tables still say so)
    };
};
// Where k_bcd_p's rank <= 8 body finds the luma matrices of a call that reads them from the caller's image bytes instead of X
// (plan_luma_bytes, lrf_plan.h): plane i < nluma of the table is the luma plane of image i, whose [3][H][W] bytes start at
// img + 3 hw i.  nluma == 0: every block reads X.  Passed to the kernel by value.
struct LumaSrc {
    const uint8_t* img;
    int hw, W;         // H W, W
    int nwl;           // luma patches per patch row (W / 8)
    int nluma;
};
struct GramChunk {
    int plane; // index into the PlaneDesc table
    int row0;  // first row of the chunk
    int slot;  // partial slot (pd.gch0 + chunk number)
    int nrows;
};

// ---- the ragged decode (lrf_qmf_decode_ragged_rgb_u8; kernels: lrf_decode_ragged_kernel.hip) ----
// One image of the call, as the kernels read it (uniform loads: the index comes from the workgroup's table entry).
struct RaggedDesc {
    ImageGeom g;
    long u_off, v_off; // int8 elements from U / V to the image's factors
    long rgb_off;      // bytes from rgb to the image's [3][H][W]
    int H, W;
    int R0, R1, R2;
    int kind, cls;     // the decode body that serves it and, for the tiled ones, the index of its rank bounds (decode_plan)
    int per_strip;     // tiled bodies: workgroups per 16-row strip
};
// One workgroup of a launch: which image, and which tile (tiled bodies) or group of 256 x reps pixel quads inside it
struct RaggedBlock {
    int image, tile;
};

// ---- the decode of windows (lrf_qmf_decode_crops_rgb_u8; kernels: lrf_decode_crops_kernel.hip) ----
// One window of the call's (h, w), as the kernels read it (a uniform load per workgroup); the image: an index into RaggedDesc
struct CropEntry {
    int image, y0, x0; // the window's origin inside the image
    int out;           // which [3][h][w] of the output it fills: its place in the caller's list
};

// ---- the decode at 1/2, 1/4, 1/8 scale (lrf_qmf_decode_scaled_rgb_u8, lrf_qmf_decode_scaled_crops_rgb_u8; kernels:
// lrf_decode_scaled_kernel.hip) ----
// One window of one scaled image, as the kernels read it (a uniform load per workgroup); a whole image is the window
// (0, 0, ceil(H / f), ceil(W / f)).  image: an index into RaggedDesc
struct ScaledItem {
    int image, f;      // the scale: 2, 4 or 8
    int y0, x0, h, w;  // the window inside the scaled image
    int place;         // its place in the caller's list
    int pad;
    long out_off;      // bytes from rgb to its [3][h][w]
    long pool_off;     // tiled body: int16 elements from the pooled-table workspace to the tables of (image, f)
};

// ---- resized crops (lrf_qmf_decode_resized_crops_rgb_u8; kernels: lrf_decode_resized_kernel.hip) ----
// One box of the call, as the kernels read it (a uniform load per workgroup).  image: an index into RaggedDesc
struct ResizedItem {
    int image, f;       // the level the box is sampled from: 1, 2, 4 or 8 (resized_level)
    int y0, x0, hb, wb; // the box in full-resolution image pixels
    int flip;           // != 0: output column c holds the value of column ow - 1 - c
    int place;          // its place in the caller's list: its output is [3][oh][ow] at 3 oh ow place
};

// ---- the tensor format of the model-ready decode entries as the kernels take it (lrf_tensor_format; the epilogue:
// lrf_decode_tensor_kernel.hip).  A kernel argument; the gray entries read element 0 of scale and bias alone
struct TensorFmt {
    float scale[3], bias[3];
    int nhwc;
};

// ---- the gray loader (lrf_qmf_decode_gray_ragged_u8, _crops_, _resized_crops_; kernels: lrf_gray_loader_kernel.hip) ----
// One gray image of the call, as the kernels read it (uniform loads): U [M][R] at u_off, V [64][R] at v_off, the padding of
// lrf_chan_dims(H, W, 1, 8, 8).  No padding bytes: the table's bytes are its key
struct GrayDesc {
    long u_off, v_off; // int8 elements from U / V to the image's factors
    int H, W, R;
    int top, left;     // padded rows above / columns left of the image
    int nw;            // patches per row of the padded image
};
// One window or one box of the call (a uniform load per workgroup).  image: an index into GrayDesc
struct GrayItem {
    int image, f;      // the level: 1, 2, 4 or 8
    int y0, x0, h, w;  // windows: the window inside level f of the image; resized crops: the box in full-resolution pixels
    int flip;          // resized crops: != 0: output column c holds the value of column ow - 1 - c
    int place;         // its place in the caller's list
    long out_off;      // elements from the output's start to the item's first pixel
    long pitch;        // elements from one output row of the item to the next
};

// ---- the ragged encode (lrf_qmf_encode_ragged_rgb_u8; kernels: lrf_planes_ragged_kernel.hip) ----
// One image of the call, as the planes kernels read it (uniform loads, like RaggedDesc; the workgroup table is RaggedBlock's:
// image, unit = strip * per_strip + column group)
struct EncRaggedDesc {
    ImageGeom g;
    long rgb_off;      // bytes from rgb to the image's [3][H][W]
    long x_off;        // floats from the X workspace to the image's three matrices
    int H, W;
    int body;          // ENC_* (lrf_plan.h): the planes body that serves it
    int per_strip;     // workgroups per 16-row strip
};

// ---- the ragged gray encode (lrf_qmf_encode_gray_ragged_sweep_u8; kernels: lrf_gray_encode_kernel.hip) ----
// One gray image of the call, as the planes kernels read it (uniform loads; the workgroup table is RaggedBlock's: image, tile =
// the group of 256 items inside it).  No padding bytes: the table's bytes are its key
struct EncGrayDesc {
    long gray_off;     // bytes from gray to the image's [H][W]
    long x_off;        // floats from the X workspace to the image's matrix [M][64]
    int H, W;
    int top, left;     // padded rows above / columns left of the image (lrf_chan_dims(H, W, 1, 8, 8))
    int nw;            // patches per row of the padded image
    int items;         // the body's work items: (hp / 8) (W / 16) 8 (ENC_GRAY16) or 16 M (ENC_GRAY_ANY)
};

// ---- the ragged metrics (lrf_image_metrics_ragged_u8, lrf_qmf_ssim_ragged_rgb_u8; kernels: lrf_metrics_ragged_kernel.hip) ----
// One pair of the call, as the kernels read it (uniform loads behind a prefix search over wg0).  Its workgroups — and its
// float64 slots, one per workgroup — are wg0 .. wg0 + C nt - 1 in the order (channel, tile row, tile column).  No padding bytes
struct MetricsPairDesc {
    long a_off, b_off; // bytes from a / b to the pair's [C][H][W]
    int H, W;
    int ntx, nt;       // tiles of 24 x 64 window positions: per tile row, per channel (k_ssim_tiles' tiling of (H, W))
    int wg0;           // the pair's first workgroup and slot
    int src;           // which entry of the source table holds (max, 255 - min) of its a image
    int vec;           // 16, 4 or 1: the widest piece every row of both images can be read in
    int pad_;
};
// One flat range of bytes of k_ragged_metrics_pre: a distinct a image (min / max) or a pair (squared error only).  Its
// workgroups are wg0 .. wg0 + ceil(n / LRF_MT_PRE_BYTES) - 1.  No padding bytes
struct MetricsSpanDesc {
    long a_off, b_off; // bytes from a / b to the range (b_off: the squared error only)
    long n;            // its bytes
    int wg0;
    int vec;           // 16, 4 or 1: the widest piece the range can be read in
};

struct GsParams {
    float lo, hi;      // clamp
    float flimit;      // |q~| >= flimit: certainly outside [lo,hi] after rounding
    float fthr;        // |q~ - rint(q~)| <= fthr: rint(q~) == rint(fl(num/den))
    int exact_int;     // iterations >= 2 only: every term and partial sum of `uu @ bb` is an exact integer in fp32 for the
                       // call's largest rank and bounds ((R-1) 64 mx^3 < 2^24), so the order of that sum is immaterial
};
#endif
