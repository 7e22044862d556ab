/*
 * lrf_hip.h — C ABI of liblrf_hip.so: the MI355X (gfx950) implementation of pashtari/lrf's
 * QMF factorisation hot path.
 *
 * The reference has no FFI: it is pure Python on torch CPU tensors.  The seam this library cuts is
 * the one SURVEY.md §8(b) names, and every entry point cites the reference code it replaces
 * (paths relative to the reference root).  A maintainer of the reference binds these with ctypes;
 * INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - Every data pointer is a DEVICE pointer (HBM) unless the parameter name ends in `_host`.
 *     lrf_malloc / lrf_free / lrf_memcpy_* let a host without any GPU runtime of its own
 *     (plain ctypes + numpy) move data.  No torch types cross this boundary.
 *   - Caller owns inputs and outputs.  The library owns only the per-context scratch workspace,
 *     grown on demand and released by lrf_ctx_destroy.
 *   - All work is enqueued on the context's HIP stream (lrf_ctx_set_stream); calls return after
 *     enqueueing unless stated.  lrf_ctx_synchronize waits for the stream.
 *   - Return value: 0 = ok, negative = LRF_E*.  lrf_last_error() returns a thread-local message.
 *   - A context is not thread-safe; use one per (host thread, device).  Distinct contexts are
 *     independent.
 *   - Factors are int8 (requires -128 <= lo <= hi <= 127; the reference default is (-16, 15),
 *     lrf/compression/qmf.py:124) in row-major [M,R] / [N,R] layout, exactly the layout
 *     `u.to(int8)`, `v.to(int8)` have at lrf/compression/qmf.py:258-260.
 */
#ifndef LRF_HIP_H
#define LRF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRF_OK 0
#define LRF_EINVAL (-1)      /* bad argument (the reference raises AssertionError / ValueError) */
#define LRF_ENOTSUP (-2)     /* valid in the reference but not implemented on this path yet */
#define LRF_EHIP (-3)        /* a HIP runtime call failed; see lrf_last_error() */
#define LRF_ENOMEM (-4)

#define LRF_MAX_RANK 64      /* largest rank of the 64-column kernels (ranks above 16 run on the untuned big-rank kernels) */
#define LRF_PATCH_ELEMS 64   /* N = p*q of the tuned kernels (8x8 patches); other N run on the any-shape kernels */
#define LRF_ANY_MAX_SIDE 2048 /* any-shape path: largest min(M, N) of the SVD initialisation */
#define LRF_ANY_MAX_RANK 639  /* any-shape path: largest rank */

typedef struct lrf_ctx lrf_ctx;

/* ---- runtime ------------------------------------------------------------------------------ */
const char* lrf_last_error(void);
int lrf_device_count(void);
int lrf_version(void);

int lrf_ctx_create(int device, lrf_ctx** out);
void lrf_ctx_destroy(lrf_ctx* ctx);
/* A new context enqueues on a non-blocking stream of its own.  lrf_ctx_set_stream switches to the
 * caller's hipStream_t, taken as is (NULL = HIP's default stream, which is what a torch process uses
 * unless it changed streams); lrf_ctx_use_own_stream switches back.  Both first wait for the stream in use. */
int lrf_ctx_set_stream(lrf_ctx* ctx, void* hip_stream);
int lrf_ctx_use_own_stream(lrf_ctx* ctx);
int lrf_ctx_synchronize(lrf_ctx* ctx);
/* Asynchronous failures.  Large calls run their iterations (all K at ranks <= 16, else 2..K) in ONE launch (k_bcd_p) whose waves wait for each
 * other with BOUNDED polls; a poll that expires (never observed in service; the exit every wave reaches) makes the launch
 * give up and report its number in page-locked host memory.  Because calls only enqueue, the report is read where results are
 * handed back: lrf_ctx_synchronize (after its wait), lrf_pipe_wait_next (for the piece it returns), the next persistent
 * call's entry, and lrf_ctx_check — which does NOT wait: call it after the stream has been waited for by other means (a
 * device-to-host copy on the stream, an event).  A non-zero return means: the factors of the named call and of every later
 * call on this context up to the check are invalid; the context itself stays usable (the next call clears the state).
 * Replaces nothing in the reference (its calls are synchronous Python): this is the error half of the async boundary. */
int lrf_ctx_check(lrf_ctx* ctx);
/* Where the persistent kernel of the context's last lrf_qmf_encode_rgb_u8 read the luma matrices from: 0 = the fp32 workspace X,
 * 1 = the caller's image bytes (large calls on sides that are multiples of 16; LRF_LUMA_BYTES=0 turns it off); -1: no such call
 * yet, or ctx is NULL.
 * The factors are the same bit for bit; tests use it to see that a call took the path they mean to test. */
int lrf_ctx_last_luma_source(const lrf_ctx* ctx);
/* What the last lrf_qmf_encode_rgb_u8 of this context kept in the Infinity Cache: the number of chroma planes whose fp32 patch
 * matrices the persistent kernel loads on the default cache policy, their bytes in *kept_bytes (may be NULL); every other
 * matrix of such a call streams with non-temporal loads.  0 and 0 bytes: the policy did not apply (a call below the persistent
 * kernel's threshold or whose matrices all fit the budget, ranks above 8, under a pipe, LRF_X_KEEP_MB=0) and every load was
 * plain; -1: no such call yet, or ctx is NULL.
 * A cache policy changes no result; tests use it to see that a call took the path they mean to test. */
int lrf_ctx_last_x_residency(const lrf_ctx* ctx, int64_t* kept_bytes);
/* bytes of scratch the context currently holds.  The scratch grows to the largest call seen (2.4 KB per input pixel of the
 * default branch: a 512 x 1365x2048 batch holds ~9 GB) and is kept for reuse; lrf_ctx_trim waits for the stream and gives
 * all of it back (the next call allocates again). */
size_t lrf_ctx_workspace_bytes(const lrf_ctx* ctx);
int lrf_ctx_trim(lrf_ctx* ctx);

/* Per-kernel timing with HIP events on the context's stream (off by default; when on, every launch
 * of the kernels below is bracketed by events).  kernel ids: LRF_K_*.  lrf_ctx_kernel_time
 * synchronises the stream and returns the accumulated milliseconds and launch count. */
#define LRF_K_PLANES 0       /* rgb -> patch matrices          */
#define LRF_K_INIT 1         /* SVD initialisation             */
#define LRF_K_BCD 2          /* U update + X^T U partials      */
#define LRF_K_VUPDATE 3      /* V update                       */
#define LRF_K_DECODE 4       /* factors -> rgb                 */
#define LRF_K_GRAM 5         /* exact Gram matrices (input of the SVD initialisation) */
#define LRF_K_BCD_PERSIST 6  /* the iterations of a large call in ONE launch (k_bcd_p: U updates + V updates) */
#define LRF_K_PLANES_GRAM 7  /* rgb -> patch matrices + the luma planes' exact Gram partials in one kernel (k_planes16_gram: large calls) */
#define LRF_K_METRICS 8      /* scoring: squared error + SSIM of image pairs (lrf_image_metrics_u8) and the squared error of a sweep from its
                                factors (lrf_qmf_sweep_sse_rgb_u8); the whole launch sequence of a call counts as one */
#define LRF_K_COUNT 9
/* Ids behind LRF_K_COUNT: launches that are not a step of the codec's own encode / decode / scoring sequences (LRF_K_COUNT stays the
 * number of those); timed and read exactly like the ids above.  LRF_K_SLOTS is the number of timers a context keeps. */
#define LRF_K_INFLATE LRF_K_COUNT /* 9: the inflate of factor columns (lrf_inflate_columns_i8: one launch per call) */
#define LRF_K_SLOTS (LRF_K_COUNT + 1)
int lrf_ctx_profile(lrf_ctx* ctx, int enable);
/* The same for a subset of the kernels: bit (1 << LRF_K_x) per kernel id, 0 = off.  An event pair costs a few
 * microseconds of stream time per launch (0.15 ms per 22-launch encode when every kernel is timed); bench.py times
 * only the dominant kernel inside its timed region. */
int lrf_ctx_profile_kernels(lrf_ctx* ctx, unsigned mask);
int lrf_ctx_kernel_time(lrf_ctx* ctx, int kernel_id, double* total_ms, long* launches);
int lrf_ctx_profile_reset(lrf_ctx* ctx);

/* ---- memory helpers (for hosts with no GPU runtime of their own) --------------------------- */
int lrf_malloc(lrf_ctx* ctx, size_t bytes, void** out_dev);
int lrf_free(lrf_ctx* ctx, void* dev);
int lrf_memcpy_h2d(lrf_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes); /* synchronous */
int lrf_memcpy_d2h(lrf_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes); /* synchronous */

/* ---- geometry ------------------------------------------------------------------------------
 * Plane c (0 = Y, 1 = Cb, 2 = Cr) of an H x W image under the default qmf_encode branch
 * (color_space="YCbCr", scale_factor=(0.5,0.5), patch 8x8): size after chroma down-sampling
 * (lrf/compression/qmf.py:230), after reflect padding (lrf/compression/utils.py:108-132) and the
 * number of patches M (lrf/compression/qmf.py:43-56). */
int lrf_plane_dims(int64_t H, int64_t W, int c, int64_t* h, int64_t* w, int64_t* hp, int64_t* wp, int64_t* M);

/* ---- the hot path -------------------------------------------------------------------------- */

/*
 * uint8 RGB images [B,3,H,W] -> patch matrices.  Replaces, for every image, image.float();
 * rgb_to_ycbcr; chroma_downsampling(mode="area"); pad_image(reflect); patchify:
 * lrf/compression/qmf.py:227-242, lrf/compression/utils.py:24-47,76-95,108-132.
 * X: per image the three matrices back to back, [M_Y,64] [M_Cb,64] [M_Cr,64], fp32 row-major
 * (image stride = (M_Y + M_Cb + M_Cr) * 64 floats).
 */
int lrf_qmf_planes_from_rgb_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, float* X);

/*
 * QMF(rank=R, num_iters=K, bounds=(lo,hi), factor=(0,1)).decompose(x) for a batch of B matrices of
 * one shape: replaces the call sites lrf/compression/qmf.py:190,209,257,281 and the body
 * lrf/factorization/qmf.py:197-214 (SVDInit :42-71, CoordinateDescent.update_u/update_v :93-139,
 * QMF._project :191-195).
 *   X    [B,M,N] fp32, K >= 1.  N == LRF_PATCH_ELEMS with R <= LRF_MAX_RANK runs on the tuned kernels; every other shape
 *        (the patch sizes of experiments/ablation_patchsize/eval.py:49-55, patch=False) on the any-shape kernels
 *        (lrf_anyshape_kernels.hip; R <= LRF_ANY_MAX_RANK, min(M,N) <= LRF_ANY_MAX_SIDE for the initialisation)
 *   sign optional [B,R] int8 (NULL = default): sign imposed on sum_j (j+1) v0[j,r] of initial
 *        component r; 0 entries mean default (-1).  The reference's sign is LAPACK's arbitrary
 *        choice (SURVEY.md §7 hard part 1); passing the reference's signs reproduces its factors.
 *   U    [B,M,R] int8,  V [B,N,R] int8
 */
int lrf_qmf_decompose_f32(lrf_ctx* ctx, const float* X, int64_t B, int64_t M, int64_t N, int R, int K,
                          int lo, int hi, const int8_t* sign, int8_t* U, int8_t* V);

/*
 * The K block-coordinate-descent iterations alone, from caller-supplied initial factors: the loop
 * lrf/factorization/qmf.py:207-212 (CoordinateDescent.forward :149-164).  U0 [B,M,R], V0 [B,N,R] fp32.
 */
int lrf_qmf_bcd_f32(lrf_ctx* ctx, const float* X, int64_t B, int64_t M, int64_t N, int R, int K,
                    int lo, int hi, const float* U0, const float* V0, int8_t* U, int8_t* V);

/*
 * QMF.decompose in its general form — the class as the reference defines it, beyond what qmf_encode asks of it
 * (lrf/factorization/qmf.py:74-214; the reference's own smoke test, test/test_factorization.py:5-10, is
 * QMF(rank=5, num_iters=10): unbounded, all three factors).  Float factors out (an unbounded factor need not fit int8).
 *   bounded / lo / hi   QMF._project (:191-195): round, then clamp to [ceil(lo), floor(hi)] when bounded
 *   l2_u, l2_v, l1_ratio  the elastic-net terms of CoordinateDescent (:77-91, 154-157, 116-118; soft_thresholding
 *                       lrf/factorization/utils.py:36-40)
 *   factors             bit 0: update u, bit 1: update v, bit 2: update w — the affine pair of x ~ w0 + w1 u v^T: the u / v
 *                       updates then see safe_divide(x - w0, w1) (:104-105, utils.py:18-33) and update_w (:141-147) refits
 *                       (w0, w1) after them.  The reference solves that least-squares problem with torch.linalg.lstsq
 *                       (LAPACK); this library with the 2 x 2 normal equations in fp64: everything downstream of an updated
 *                       w is parity by tolerance (loss to 2e-4), everything else is the reference's bit for bit.  For a constant
 *                       z = u v^T = c != 0 the determinant is exactly zero and this library returns (mean x, 0), where the
 *                       reference's lstsq returns an ill-conditioned pair whose reconstruction w0 + w1 c only nears the mean.
 *   U0 [B,M,R], V0 [B,N,R] fp32, both or neither: initial factors; NULL = this library's SVD initialisation (sign as in
 *                       lrf_qmf_decompose_f32).
 *   U [B,M,R], V [B,N,R], W [B,2] = (w0, w1) fp32, device memory.  eps (opts, default 1e-16) is also the eps of that safe_divide
 *   (qmf.py:105): a pair with |w1| < eps divides by eps * sign(w1) — the default pair (0, 1) included, when eps > 1.  K = 0 returns the
 *   initial factors.  Runs on the any-shape kernels for every shape (R <= LRF_ANY_MAX_RANK).
 */
typedef struct lrf_qmf_opts {
    int bounded;
    float lo, hi;
    double l2_u, l2_v, l1_ratio;
    int factors;
    double eps;   /* CoordinateDescent(eps=...) (lrf/factorization/qmf.py:82, 90, 117-118); 0 selects the default 1e-16 */
    int w_init;   /* non-zero: W [B][2] holds the INITIAL pair (w0, w1) on entry — SVDInit(num_levels=...), qmf.py:56-68 —
                     and U0 / V0 the factors it belongs to; the u / v updates then see safe_divide(x - w0, w1) (qmf.py:104-105)
                     also when bit 2 of `factors` is clear.  Zero: [0; 1]. */
} lrf_qmf_opts;
int lrf_qmf_decompose_ex_f32(lrf_ctx* ctx, const float* X, int64_t B, int64_t M, int64_t N, int R, int K, const lrf_qmf_opts* opts,
                             const int8_t* sign, const float* U0, const float* V0, float* U, float* V, float* W);

/*
 * The initial factors alone (what SVDInit.forward returns, lrf/factorization/qmf.py:42-71):
 * u0 = U sqrt(s) [B,M,R], v0 = (sqrt(s) Vh)^T [B,N,R], fp32.  Also the arithmetic of svd_encode's
 * lrf/compression/svd.py:179-183 for N == LRF_PATCH_ELEMS.
 */
int lrf_qmf_svd_init_f32(lrf_ctx* ctx, const float* X, int64_t B, int64_t M, int64_t N, int R,
                         const int8_t* sign, float* U0, float* V0);

/*
 * QMF.loss(x, u, v, w) for a batch: the relative error ||x - (w0 + w1 u v^T)||_F / (||x||_F + 1e-16) per matrix —
 * lrf/factorization/qmf.py:225-227, relative_error lrf/factorization/utils.py:12-15 — which QMF(verbose=True) prints before every
 * iteration (qmf.py:208-210).  X [B,M,N], U [B,M,R], V [B,N,R] fp32; W [B,2] = (w0, w1) or NULL (= (0, 1)); loss [B] fp32.  The
 * sums are accumulated in fp64 (the reference: torch.norm in fp32; agreement to ~1e-6 relative).
 */
int lrf_qmf_loss_f32(lrf_ctx* ctx, const float* X, const float* U, const float* V, const float* W, int64_t B, int64_t M, int64_t N, int R,
                     float* loss);

/*
 * Fused encode of B images (default qmf_encode branch, everything between image.float() and the
 * byte container): lrf/compression/qmf.py:227-262.
 *   rgb  [B,3,H,W] uint8;  R[3] ranks of (Y, Cb, Cr);  sign optional [B, R[0]+R[1]+R[2]] int8
 *   U    per image [M_Y,R0] [M_Cb,R1] [M_Cr,R2] int8 back to back; V likewise with 64 rows each.
 */
int lrf_qmf_encode_rgb_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, const int R[3],
                          int K, int lo, int hi, const int8_t* sign, int8_t* U, int8_t* V);

/*
 * The same encode for ONE batch at Q rank triples in one call: the R-D sweep of the reference's experiments
 * (experiments/comparison/eval.py:83-110 calls qmf_encode per image and quality; BASELINE config 3: 24 images x quality 1..32).
 * What does not depend on the rank is computed once per image (patch matrices, exact Gram matrices), the SVD initialisation
 * once per (image, channel) at the largest rank asked for that channel — the lower ranks take its leading columns, which are
 * the same singular pairs bit for bit — and the BCD of all (triple, image) pairs runs as one call of Q x B matrices sets that
 * share X (large launches per rank family; the persistent kernel from 3584 blocks, 2304 for one rank family).  Every (triple, image) result is
 * byte-identical to lrf_qmf_encode_rgb_u8's for that triple.
 *   R     [Q][3] ranks (Y, Cb, Cr) per triple, each 1..32 (larger ranks: one lrf_qmf_encode_rgb_u8 call per triple)
 *   sign  optional [B][Rmax_Y + Rmax_Cb + Rmax_Cr] int8 (Rmax_c = the largest rank of channel c over the triples): the signs
 *         of the initial components; every triple uses the leading ones of its ranks
 *   U, V  for q = 0 .. Q-1 the factors of the B images at triple q back to back, each block in lrf_qmf_encode_rgb_u8's
 *         layout: U offset sum_{q' < q} B u_img(q'), u_img(q) = sum_c M_c R[q][c]; V likewise with 64 R[q][c]
 */
int lrf_qmf_encode_sweep_rgb_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, int Q, const int* R, int K, int lo, int hi,
                                const int8_t* sign, int8_t* U, int8_t* V);

/*
 * Fused decode of B images: QMF.reconstruct, depatchify, unpad_image, chroma_upsampling(nearest),
 * ycbcr_to_rgb, to_dtype(uint8): lrf/compression/qmf.py:329-351, lrf/factorization/qmf.py:216-223,
 * lrf/compression/utils.py:50-73,98-105,135-182.  U, V laid out as lrf_qmf_encode_rgb_u8 writes them.
 */
int lrf_qmf_decode_rgb_u8(lrf_ctx* ctx, const int8_t* U, const int8_t* V, int64_t B, int64_t H, int64_t W,
                          const int R[3], uint8_t* rgb);

/*
 * The same decode (lrf/compression/qmf.py:295-353) for a list of n images that differ in size and in ranks, in one call: what a
 * per-image quality choice or a dataset of mixed sizes hands to a decoder.
 *   images  [n] descriptors in host memory
 *   U, V    device buffers of u_len / v_len int8 elements; image i's factors start at u_off / v_off and are laid out as
 *           lrf_qmf_encode_rgb_u8 writes ONE image: [M_Y,R_Y] [M_Cb,R_Cb] [M_Cr,R_Cr], and three [64,R_c]
 *   rgb     device buffer of rgb_len bytes; image i is written as [3][H][W] at rgb_off
 * Image i's bytes are those the uniform decoder writes when called for that image alone (B = 1, U + u_off, V + v_off,
 * rgb + rgb_off), for every geometry and rank it accepts: the kernels run the same device functions.  They do not depend on
 * the image's place in the list or on the other images.
 * Launches: the images whose sides are multiples of 16 (with rgb + rgb_off a multiple of 8) and whose ranks are within
 * (32,16,16) share one launch whatever their ranks; the other images the tiled decoder covers take one launch per rank-bound
 * class (at most five); one launch each for the images only the rank <= 8 kernel and the general kernel serve: at most eight.
 * Asynchronous on the context's stream and timed under LRF_K_DECODE, except that the first call of a new list uploads a table
 * (the descriptors and an entry per workgroup) and waits for the stream; lrf_ctx_trim releases the table.
 * Everything is validated on the host before any launch.  LRF_EINVAL: a NULL pointer, n outside [1,65535], a rank outside
 * [1,64], a size the uniform decoder refuses, a negative offset, an image whose U, V or rgb range leaves its buffer, 2^31 or
 * more workgroups in one launch.
 */
typedef struct {
    int64_t H, W;         /* image size */
    int R[3];             /* ranks Y, Cb, Cr, each 1..64 */
    int64_t u_off, v_off; /* int8 elements from U / V to this image's factors */
    int64_t rgb_off;      /* bytes from rgb to this image's [3][H][W] output */
} lrf_ragged_image;
int lrf_qmf_decode_ragged_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_image* images /* host */, const int8_t* U, int64_t u_len,
                                 const int8_t* V, int64_t v_len, uint8_t* rgb, int64_t rgb_len);

/*
 * Windows of compressed images straight from their factors: n_crops windows of one size (h, w) out of a list of images that
 * differ in size and in ranks, in one call — the decode of lrf/compression/qmf.py:329-351, lrf/factorization/qmf.py:216-223,
 * lrf/compression/utils.py:50-73,98-105,135-182 followed by a slice, without the pixels outside the slice.  A pixel depends on
 * one row of U per plane and on the three V tables, so a window costs its own patches only: what a training loader that keeps
 * a dataset resident as int8 factors asks for at every step.
 *   images  [n_images] descriptors in host memory, as for lrf_qmf_decode_ragged_rgb_u8 (rgb_off is ignored)
 *   crops   [n_crops] windows in host memory: rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of image `image`
 *   rgb     device buffer of rgb_len bytes; crop j is written as [3][h][w] at 3 h w j
 * Crop j = (image i, y0, x0) equals decode(image i)[:, y0:y0+h, x0:x0+w] byte for byte, decode being what
 * lrf_qmf_decode_rgb_u8 writes for that image alone, for every geometry and rank triple that decoder accepts: the kernels run
 * the same device functions at the image's coordinates.  A crop's bytes depend on nothing else in the call.
 * Launches: one per rank-bound class present among the images the tiled decoders cover (at most five), one each for those only
 * the rank <= 8 kernel and the general kernel serve: at most seven.
 * Asynchronous on the context's stream and timed under LRF_K_DECODE.  The image descriptors stay on the device between calls,
 * keyed on their bytes (the first call of a new image list uploads them and waits for the stream; lrf_ctx_trim releases
 * them).  The crop list does not: it travels stream-ordered through pinned staging slots the context owns, and a slot is
 * reused only after an event says its copy has run, so calls with fresh lists follow each other without a stream wait.
 * Everything is validated on the host before any launch, and a refused call writes nothing.  LRF_EINVAL: a NULL pointer,
 * n_images outside [1,65535], n_crops outside [1,2^20], h or w below 1, a crop whose image index is out of range or whose
 * rectangle leaves its image, a rank outside [1,64], a size the uniform decoder refuses, a negative offset, a U, V or rgb range
 * that leaves its buffer, 2^31 or more workgroups in one launch.
 */
typedef struct {
    int32_t image, y0, x0;
} lrf_crop;
int lrf_qmf_decode_crops_rgb_u8(lrf_ctx* ctx, int64_t n_images, const lrf_ragged_image* images /* host; rgb_off ignored */, const int8_t* U,
                                int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_crop* crops /* host */, int64_t h,
                                int64_t w, uint8_t* rgb /* [n_crops][3][h][w] */, int64_t rgb_len);

/*
 * Compressed images at 1/2, 1/4 or 1/8 scale straight from their factors: the decode of lrf/compression/qmf.py:329-351,
 * lrf/factorization/qmf.py:216-223, lrf/compression/utils.py:50-73,98-105,135-182 with an area pooling in front of its colour
 * conversion (utils.py:50-73), without the full-resolution pixels.  lrf_scaled_dims: the scaled size, Hs = ceil(H / scale),
 * Ws = ceil(W / scale); LRF_EINVAL for a scale outside {2, 4, 8}, a size outside [1,2^31) or a NULL pointer.
 * Output pixel (i, j) covers image rows scale i .. min(scale i + scale, H) - 1 and the columns likewise (n pixels: the partial
 * blocks at the bottom and right edge average the pixels that exist).  Per plane the integers the decoder holds before its
 * colour conversion — luma at the pixel, chroma at its nearest-neighbour sample min(floor(float(y) * (float(h_c) / float(H))),
 * h_c - 1) — are summed exactly (int32), the mean is float(sum) / float(n), and the means go through the decoder's colour
 * chain, clamp and truncation.  A luma patch is u . V^T, so a block's sum is u . (the sum of those rows of V): the pooling
 * moves onto a small table per image, the call reads the same U and writes 1 / scale^2 of the pixels.
 *   images  [n] descriptors in host memory, as for lrf_qmf_decode_ragged_rgb_u8; image i is written as [3][Hs_i][Ws_i] at rgb_off
 * Images whose sides are multiples of 16 and whose ranks lie inside the tiled decoders' bounds (32, 16, 16) take the tiled kernel,
 * every other geometry and rank the general one; both give the bytes of the definition above, and an image's bytes depend on
 * nothing else in the call.  Launches: one that builds the pooled tables, one per (scale, rank-bound class) of the tiled images
 * and one per scale of the others: at most 1 + 5 + 1 here, 1 + 15 + 3 in the crops entry.
 * Asynchronous on the context's stream and timed under LRF_K_DECODE.  The image descriptors stay on the device between calls,
 * keyed on their bytes and shared with lrf_qmf_decode_crops_rgb_u8 (lrf_ctx_trim releases them); the item list travels
 * stream-ordered through that entry's pinned staging slots.  Everything is validated on the host before any launch, and a
 * refused call writes nothing.  LRF_EINVAL: a NULL pointer, n outside [1,65535], a scale outside {2, 4, 8}, a rank outside
 * [1,64], a size the uniform decoder refuses, a negative offset, a U, V or rgb range that leaves its buffer, 2^31 or more
 * workgroups in one launch.
 */
int lrf_scaled_dims(int64_t H, int64_t W, int scale, int64_t* Hs, int64_t* Ws);
int lrf_qmf_decode_scaled_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_image* images /* host */, int scale, const int8_t* U, int64_t u_len,
                                 const int8_t* V, int64_t v_len, uint8_t* rgb, int64_t rgb_len);

/*
 * Windows of scaled images: n_crops windows of one size (h, w), each out of the image `image` at its own scale — a loader takes
 * each window from the level nearest the zoom it drew.  Window j = rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of the scaled
 * image, equal byte for byte to that slice of what lrf_qmf_decode_scaled_rgb_u8 writes for the image at that scale (a whole
 * image is the window (0, 0, Hs, Ws): the two entries share their kernels); written as [3][h][w] at 3 h w j.
 * As lrf_qmf_decode_crops_rgb_u8 otherwise: images (rgb_off ignored), the resident descriptors, the staging slots, the
 * validation before any launch.  LRF_EINVAL in addition to the list above: n_images outside [1,65535], n_crops outside
 * [1,2^20], h or w below 1, a crop whose image index is out of range, whose scale is outside {2, 4, 8} or whose rectangle
 * leaves its image's scaled size.
 */
typedef struct {
    int32_t image, scale, y0, x0; /* y0, x0 in the scaled image */
} lrf_scaled_crop;
int lrf_qmf_decode_scaled_crops_rgb_u8(lrf_ctx* ctx, int64_t n_images, const lrf_ragged_image* images /* host; rgb_off ignored */, const int8_t* U,
                                       int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops /* host */,
                                       int64_t h, int64_t w, uint8_t* rgb /* [n_crops][3][h][w] */, int64_t rgb_len);

/*
 * Resized crops: n_crops boxes of any size and position, out of images that differ in size and ranks, resampled to one output
 * size (oh, ow) in one call — what a random-resized-crop loader asks for at every step.  A box reads the patches it touches
 * and nothing full-size is written.  Box j = rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of image `image` in
 * full-resolution pixels; its output is written as [3][oh][ow] at 3 oh ow j.  Exact integers:
 *   level   f = the largest of 8, 4, 2 with f oh <= h and f ow <= w, else 1.  L = what lrf_qmf_decode_rgb_u8 writes for the
 *           image (f = 1) or lrf_qmf_decode_scaled_rgb_u8 at scale f, Hs x Ws = ceil(H / f) x ceil(W / f).  A box more than 16
 *           times the output on its shorter ratio is sampled from level 8 without further prefiltering.
 *   taps    per axis, (r, n_out, b0, nb, n_lvl) = (row, oh, y0, h, Hs) or the column values, in int64:
 *           N = (2 r + 1) nb + 2 n_out b0 - n_out f, D = 2 n_out f, q = clamp(floor(256 N / D), 0, 256 (n_lvl - 1)),
 *           i0 = q >> 8, i1 = min(i0 + 1, n_lvl - 1), t = q & 255
 *   pixel   per channel ((256 - ty)(256 - tx) L[iy0][ix0] + (256 - ty) tx L[iy0][ix1] + ty (256 - tx) L[iy1][ix0]
 *           + ty tx L[iy1][ix1] + 32768) >> 16; with flip != 0 output column c holds the value defined for column ow - 1 - c.
 * So a box of the output's size is the crop of lrf_qmf_decode_crops_rgb_u8 byte for byte, a box with y0, x0 multiples of f,
 * h = f oh and w = f ow the crop of lrf_qmf_decode_scaled_crops_rgb_u8 at scale f and (y0 / f, x0 / f), and every result lies
 * within 2.5 levels of the real-valued bilinear interpolation of L at the same centres.  These are not torchvision's bytes.
 * A box's bytes depend on nothing else in the call.  Launches: one per (path, level, rank class) present, at most sixteen.
 * As lrf_qmf_decode_crops_rgb_u8 otherwise: images (rgb_off ignored), the resident descriptors, the staging slots, no stream
 * wait for a fresh list, LRF_K_DECODE, the validation before any launch.  LRF_EINVAL in addition to that entry's list: oh or
 * ow outside [1,16384], a box side below 1.
 */
typedef struct {
    int32_t image, y0, x0, h, w, flip;
} lrf_resized_crop;
int lrf_qmf_decode_resized_crops_rgb_u8(lrf_ctx* ctx, int64_t n_images, const lrf_ragged_image* images /* host; rgb_off ignored */, const int8_t* U,
                                        int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_resized_crop* crops /* host */,
                                        int64_t oh, int64_t ow, uint8_t* rgb /* [n_crops][3][oh][ow] */, int64_t rgb_len);

/*
 * Model-ready crops: the three entries above with the to-tensor and normalise steps of a training loader in their epilogue, so
 * that no uint8 batch is written and read back.  A tensor format is (dtype, layout, scale[3], bias[3]):
 *   dtype    LRF_T_F32, LRF_T_F16 (IEEE binary16) or LRF_T_BF16 (bfloat16)
 *   layout   LRF_T_NCHW: crop j is [3][h][w] elements at 3 h w j; LRF_T_NHWC: [h][w][3] elements at 3 h w j (torch's
 *            channels_last memory of a [n,3,h,w] tensor)
 *   scale, bias   finite fp32 numbers per channel: 1 / (255 std_k) and -mean_k / std_k for torchvision's
 *            ToDtype(scale=True) + Normalize(mean, std)
 * For the byte b that the _rgb_u8 entry of the same name defines for (crop j, channel k, row y, column x) — flips included: the
 * reversal is of pixels — the element is
 *   t = fl32(float(b) * scale[k]);   v = fl32(t + bias[k]);   out = v rounded to nearest even into dtype
 * two fp32 roundings and one conversion, NOT a fused multiply-add (for the ImageNet constants the fused form differs on 133,
 * 132 and 124 of the 256 byte values of the three channels).  torch reproduces it bit for bit on the CPU: b.float().mul(s).add(o).to(dtype).  A float16
 * result beyond 65504 is +-inf, as torch's conversion gives.
 * Everything else is the _rgb_u8 entry's: the leading arguments, the resident descriptors, the pinned staging slots with no
 * stream wait for a fresh list, the same launch plan (the format only selects the instantiation a launch names), LRF_K_DECODE,
 * the validation of everything on the host before any launch, a refused call writing nothing.  LRF_EINVAL in addition to that
 * entry's list: a NULL fmt, a dtype or layout outside the enums, a scale or bias that is not finite, an `out` that is not
 * aligned to the element size, out_bytes below n_crops * 3 * h * w * sizeof(element).
 */
#define LRF_T_F32 0
#define LRF_T_F16 1
#define LRF_T_BF16 2
#define LRF_T_NCHW 0
#define LRF_T_NHWC 1
typedef struct {
    int32_t dtype;  /* LRF_T_F32, LRF_T_F16, LRF_T_BF16 */
    int32_t layout; /* LRF_T_NCHW, LRF_T_NHWC */
    float scale[3], bias[3];
} lrf_tensor_format;
int lrf_qmf_decode_crops_tensor(lrf_ctx* ctx, int64_t n_images, const lrf_ragged_image* images /* host; rgb_off ignored */, const int8_t* U,
                                int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_crop* crops /* host */, int64_t h,
                                int64_t w, const lrf_tensor_format* fmt /* host */, void* out, int64_t out_bytes);
int lrf_qmf_decode_scaled_crops_tensor(lrf_ctx* ctx, int64_t n_images, const lrf_ragged_image* images /* host; rgb_off ignored */, const int8_t* U,
                                       int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops /* host */,
                                       int64_t h, int64_t w, const lrf_tensor_format* fmt /* host */, void* out, int64_t out_bytes);
int lrf_qmf_decode_resized_crops_tensor(lrf_ctx* ctx, int64_t n_images, const lrf_ragged_image* images /* host; rgb_off ignored */, const int8_t* U,
                                        int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_resized_crop* crops /* host */,
                                        int64_t oh, int64_t ow, const lrf_tensor_format* fmt /* host */, void* out, int64_t out_bytes);

/*
 * The fused encode (lrf/compression/qmf.py:227-262) for a list of n images that differ in size and in ranks, in one call: what a
 * dataset of mixed sizes or a per-image quality choice hands to an encoder.
 *   images  [n] descriptors in host memory
 *   rgb     device buffer of rgb_len bytes; image i is read as [3][H][W] at rgb_off
 *   sign    optional device buffer of sign_len int8; image i's R[0]+R[1]+R[2] signs (as lrf_qmf_encode_rgb_u8's) start at
 *           sign_off; a sign_off of -1, or a NULL sign, gives the image the default signs
 *   U, V    device buffers of u_len / v_len int8 elements; image i's factors are written at u_off / v_off, laid out as
 *           lrf_qmf_encode_rgb_u8 writes ONE image: [M_Y,R_Y] [M_Cb,R_Cb] [M_Cr,R_Cr], and three [64,R_c]
 * Image i's U / V bytes are exactly those lrf_qmf_encode_rgb_u8 writes when called for that image alone (B = 1) with the same
 * R, K, lo, hi and signs: the planes kernels run the same device functions, every BCD kernel family computes the same bits, the
 * Gram matrix is exact.  They do not depend on the image's place in the list or on the other images.
 * Launches of the planes stage: the images whose sides are multiples of 16 (with rgb + rgb_off a multiple of 8) share one, the
 * others take one per pooling-window size (2 or 3 by the parity of H and of W): at most five, timed under LRF_K_PLANES.  From
 * there on the call is one table of 3 n matrices — large launches per rank family, the persistent kernel from its usual block
 * counts — whatever the sizes.  Asynchronous on the context's stream, except that the first call of a new list uploads its
 * tables and waits for the stream; lrf_ctx_trim releases them.
 * Everything is validated on the host before any launch or write.  LRF_EINVAL: a NULL pointer, n outside [1,65535], a size or
 * rank or bounds lrf_qmf_encode_rgb_u8 refuses with it, a negative offset, an image whose pixels, signs or factors leave their
 * buffer, factor ranges of two images that overlap.  LRF_ENOTSUP: a rank above 32 (encode those images with
 * lrf_qmf_encode_rgb_u8), an image of 2^31 / 3 pixels or more, 2^31 or more blocks in the call.
 */
typedef struct {
    int64_t H, W;                   /* image size */
    int R[3];                       /* ranks Y, Cb, Cr, each 1..32 */
    int64_t rgb_off;                /* bytes from rgb to this image's [3][H][W] input */
    int64_t u_off, v_off, sign_off; /* int8 elements from U / V / sign to this image's factors / signs; sign_off -1: default signs */
} lrf_ragged_encode_image;
int lrf_qmf_encode_ragged_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_encode_image* images /* host */, const uint8_t* rgb, int64_t rgb_len,
                                 int K, int lo, int hi, const int8_t* sign /* optional, flat */, int64_t sign_len, int8_t* U, int64_t u_len,
                                 int8_t* V, int64_t v_len);

/*
 * A ragged sweep: n images of differing sizes, each at a list of candidate rank triples of its own, m candidates in all, in one
 * call — lrf_qmf_encode_sweep_rgb_u8 and lrf_qmf_encode_ragged_rgb_u8 married (rate control over a list of mixed sizes).
 *   images  n descriptors in host memory: size, where the image's [3][H][W] bytes start in rgb, and where its signs start
 *           in sign (-1, or a NULL sign: the default signs).  The signs of an image are [Rmax_Y + Rmax_Cb + Rmax_Cr], the largest
 *           rank of each channel over the image's candidates; every candidate uses the leading signs of its ranks (the uniform
 *           sweep's convention)
 *   cands   m descriptors in host memory: the image a candidate belongs to, its ranks (1..32) and where its factors are
 *           written in U / V, in lrf_qmf_encode_rgb_u8's layout of ONE image.  The candidates of an image may lie anywhere in
 *           the list; every image needs at least one
 * Candidate j's U / V bytes are exactly those lrf_qmf_encode_ragged_rgb_u8 writes for (image, R) alone with the same K, lo, hi
 * and signs, which in turn are lrf_qmf_encode_rgb_u8's at B = 1.
 * Shared per image: the planes stage (the ragged planes kernels, plan_encode_ragged's launches), the X workspace (the sum over
 * images, not candidates), the exact Gram matrix and the SVD initialisation, once per (image, channel) at the image's largest
 * rank for the channel; the other candidates take its leading columns.  The BCD of all m candidates is one table in the uniform
 * sweep's order, its kernels chosen by the same plan.  Asynchronous on the context's stream, except that a new list uploads its
 * tables and waits for the stream.
 * Everything is validated on the host before any launch or write.  LRF_EINVAL: a NULL pointer, n outside [1,65535], m outside
 * [n,2^20], a candidate naming no image, an image without a candidate, a size or rank or bounds lrf_qmf_encode_rgb_u8 refuses
 * with it, a negative offset, pixels, signs or factors that leave their buffer, factor ranges of two candidates that overlap.
 * LRF_ENOTSUP: a rank above 32, an image of 2^31 / 3 pixels or more, 2^31 or more blocks in the call.
 */
typedef struct {
    int64_t H, W;      /* image size */
    int64_t rgb_off;   /* bytes from rgb to this image's [3][H][W] input */
    int64_t sign_off;  /* int8 elements from sign to this image's signs; -1: default signs */
} lrf_ragged_sweep_image;
typedef struct {
    int32_t image;        /* index into images */
    int R[3];             /* ranks Y, Cb, Cr, each 1..32 */
    int64_t u_off, v_off; /* int8 elements from U / V to this candidate's factors */
} lrf_ragged_sweep_candidate;
int lrf_qmf_encode_ragged_sweep_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_sweep_image* images /* host */, int64_t m,
                                       const lrf_ragged_sweep_candidate* cands /* host */, const uint8_t* rgb, int64_t rgb_len, int K, int lo,
                                       int hi, const int8_t* sign /* optional, flat */, int64_t sign_len, int8_t* U, int64_t u_len, int8_t* V,
                                       int64_t v_len);

/* ---- scoring (the third stage of the reference's experiment loop) ----------------------------- */

/*
 * Squared error and SSIM of B pairs of uint8 images, a [B,C,H,W] against b [B,C,H,W] (contiguous, device memory): what
 * lrf/utils/misc.py:107-108 computes per image on the host with lrf/utils/metrics.py:57-71 (psnr) and :74-91 (ssim, through
 * scikit-image's structural_similarity(channel_axis=0, data_range=img1.max() - img1.min())).
 *   sse  [B]  sum over the C*H*W samples of (a - b)^2, an exact integer (PSNR = 20 log10(max_value / sqrt(sse / (C H W))) is the
 *             caller's one line)
 *   ssim [B]  float64, or NULL to skip the SSIM work: 7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance (49/48),
 *             data_range = max - min of a's image (per image), S averaged over the window positions that lie wholly inside the
 *             image (rows 3 .. H-4, columns 3 .. W-4 of every channel), then the mean of the C channel means.  The window sums
 *             are exact integers; float64 enters with the four brackets of S, and one division per window.  A constant first
 *             image (data_range 0) gives what the host formula gives: NaN wherever b's window is constant too.
 * Deterministic, and an image's results do not depend on B or on its place in the batch (no floating-point atomics: one
 * partial sum per tile of 24 x 64 window positions, added in a fixed order).  Asynchronous on the context's stream.
 * LRF_EINVAL: NULL a / b / sse, B or C < 1, B > 65535, H or W < 7 when ssim is asked for (the reference raises ValueError).
 */
int lrf_image_metrics_u8(lrf_ctx* ctx, const uint8_t* a, const uint8_t* b, int B, int C, int H, int W, uint64_t* sse /* [B] */,
                         double* ssim /* [B] or NULL */);

/*
 * Squared error of a quality sweep straight from its factors: for q = 0 .. Q-1 and every image b,
 *   sse[q][b] = sum over the 3*H*W samples of (rgb_b - decode(U_q,b, V_q,b))^2, an exact integer,
 * where decode is byte for byte what lrf_qmf_decode_rgb_u8 writes — the kernels run the same device functions and compare each run
 * of decoded bytes with the source where the decode kernel stores it; no decoded image exists.  Equal to lrf_qmf_decode_rgb_u8
 * followed by lrf_image_metrics_u8(ssim = NULL) per triple, for every geometry and rank (1..64 per plane) those accept.
 *   rgb   [B,3,H,W] uint8, the source images
 *   U, V  laid out as lrf_qmf_encode_sweep_rgb_u8 writes them for (B, H, W, Q, R); Q = 1 is lrf_qmf_encode_rgb_u8's layout
 *   R     [Q][3] ranks per triple (host memory)
 *   sse   [Q][B] uint64 (device memory)
 * Integer sums (uint32 per lane and wave, uint64 per workgroup, one 64-bit integer atomic per workgroup): deterministic, and an
 * image's result depends on neither B, Q nor its place.  Asynchronous on the context's stream, except that the first call of a
 * new (B, H, W, R) uploads a small table and waits for the stream.  One launch covers all (triple, image, tile) items when both
 * sides are multiples of 16 and every triple is within ranks (32,16,16); other geometries take one launch per rank-bound class
 * of the strip kernel (at most five), plus one each for the triples only the general kernels serve.
 * LRF_EINVAL: a NULL pointer, Q outside [1,4096], B outside [1,65535], a rank outside [1,64].  After lrf_ctx_trim the table is
 * uploaded again.
 */
int lrf_qmf_sweep_sse_rgb_u8(lrf_ctx* ctx, const uint8_t* rgb /* [B,3,H,W] */, const int8_t* U, const int8_t* V, int64_t B, int64_t H,
                             int64_t W, int Q, const int* R /* [Q][3] */, uint64_t* sse /* [Q][B] */);

/*
 * The same for a list of items that differ in size and ranks: sse[i] = sum over the 3 H_i W_i samples of
 * (source_i - decode(U_i, V_i))^2, an exact integer, where decode is byte for byte the image lrf_qmf_decode_ragged_rgb_u8 writes
 * for the same descriptor and source_i is the [3][H_i][W_i] at rgb + items[i].rgb_off.  Several items may read one source (the
 * candidates of an image do) and the items may come in any order; the value depends on neither.
 *   items  n descriptors in host memory, lrf_qmf_decode_ragged_rgb_u8's, with rgb_off naming where the SOURCE is read
 *   sse    [n] uint64 (device memory); zeroed by the call on its stream
 * The kernels are the ragged decode kernels with the uniform scorer's sink: integer sums (uint32 per lane and wave, uint64 per
 * workgroup, one 64-bit integer atomic per workgroup).  At most eight launches (plan_decode_ragged), timed under LRF_K_DECODE.
 * The table travels stream-ordered through pinned slots and is not kept: the call does not wait for the stream.
 * LRF_EINVAL: what lrf_qmf_decode_ragged_rgb_u8 refuses (a NULL pointer, n outside [1,65535], a rank outside [1,64], a negative
 * offset, factors or a source that leave their buffer); source ranges may overlap.
 */
int lrf_qmf_sse_ragged_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_image* items /* host */, const int8_t* U, int64_t u_len, const int8_t* V,
                              int64_t v_len, const uint8_t* rgb, int64_t rgb_len, uint64_t* sse /* [n] */);

/*
 * Squared error and SSIM of n pairs of uint8 images that differ in size, in one call: pair i is the [C][H_i][W_i] at
 * a + pairs[i].a_off against the [C][H_i][W_i] at b + pairs[i].b_off (device memory) — lrf/utils/metrics.py:57-71 and :74-91
 * per pair, as lrf_image_metrics_u8 states them.
 *   pairs  n descriptors in host memory; several pairs may read one a image (the candidates of an image do) and ranges may
 *          overlap: both buffers are read-only
 *   sse    [n] uint64 (device memory); zeroed by the call on its stream
 *   ssim   [n] float64, or NULL to skip the SSIM work
 * sse[i] and ssim[i] are bit for bit what lrf_image_metrics_u8 gives for pair i alone (B = 1), NaN included: the kernels run that
 * entry's device functions on its tiling of (H_i, W_i).  Deterministic; the result depends on neither the order of the list
 * nor the other pairs nor where the images start (exact integer window sums, one float64 partial sum per tile of 24 x 64
 * window positions added in a fixed order, 64-bit integer atomics for the squared error, no floating-point atomics).
 * Launches, with ssim: one flat read for (max, 255 - min) of every DISTINCT a image (pairs that share (a_off, H, W) share it),
 * a workgroup per (pair, channel, tile) — one launch per load width that occurs in the list, at most three —, one launch of a
 * workgroup per pair; without: one flat read.  Images are read 16, 4 or 1 bytes at a time, decided per pair from where its
 * images start and W_i; the width changes no value.  Asynchronous on the context's stream
 * and timed under LRF_K_METRICS; the table travels stream-ordered through pinned slots and is not kept.  Everything is
 * validated on the host before any launch, and a refused call writes nothing.  LRF_EINVAL: a NULL pointer, n outside
 * [1,65535], C outside [1,65535], a side below 1 (with ssim: below 7, the reference's ValueError) or above 2^20, an image of
 * 2^40 samples or more, a negative offset, an image that leaves its buffer, 2^31 or more workgroups.
 */
typedef struct {
    int64_t H, W;         /* the size both images of the pair share */
    int64_t a_off, b_off; /* bytes from a / b to the pair's [C][H][W] */
} lrf_image_pair;
int lrf_image_metrics_ragged_u8(lrf_ctx* ctx, int64_t n, const lrf_image_pair* pairs /* host */, int C, const uint8_t* a, int64_t a_len,
                                const uint8_t* b, int64_t b_len, uint64_t* sse /* [n] */, double* ssim /* [n] or NULL */);

/*
 * Squared error and SSIM of n (factors, source) items that differ in size and ranks, scored from the factors: what
 * lrf_qmf_decode_ragged_rgb_u8 followed by lrf_image_metrics_u8(source_i, decoded_i) gives per item, bit for bit, and sse[i]
 * is lrf_qmf_sse_ragged_rgb_u8's.  What qmf_encode_target(ssim=...) scores the candidates of a sweep with (the SSIM curve of
 * the reference's experiments: lrf/utils/metrics.py:74-91).
 *   items          lrf_qmf_sse_ragged_rgb_u8's: rgb_off names where the SOURCE [3][H][W] is read; sources may be shared
 *   scratch_bytes  the cap on the decoded bytes alive at once; 0: 256 MiB (a cap, not a tuned value)
 *   sse, ssim      [n] (device memory)
 * Consecutive items form a chunk while their decoded bytes (3 H W each, rounded up to 16) fit the cap; an item larger than the
 * cap is a chunk of its own.  Per chunk: the ragged decode into the context's scratch buffer (at most eight launches), then the
 * launches of lrf_image_metrics_ragged_u8 with the sources as a and the scratch as b.  Memory is bounded by the cap (or
 * the largest item), not by n, and the results are identical for every scratch_bytes.  Deterministic as both parts are.
 * Asynchronous on the context's stream (a stream the caller set included) and timed under LRF_K_METRICS; every table travels
 * stream-ordered through pinned slots; the call waits for the stream only when the scratch buffer has to grow.
 * lrf_ctx_trim frees the scratch.  Everything — every chunk's tables too — is validated on the host before any launch, and a
 * refused call writes nothing.  LRF_EINVAL: what lrf_qmf_sse_ragged_rgb_u8 refuses, H or W below 7, a negative scratch_bytes.
 */
int lrf_qmf_ssim_ragged_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_image* items /* host; rgb_off = the SOURCE */, const int8_t* U,
                               int64_t u_len, const int8_t* V, int64_t v_len, const uint8_t* rgb, int64_t rgb_len,
                               int64_t scratch_bytes /* 0: default */, uint64_t* sse /* [n] */, double* ssim /* [n] */);

/* ---- the SVD baseline ------------------------------------------------- */

/*
 * svd_encode, default branch (color_space="RGB", patch 8x8, uint8 factors), everything between image.float() and the byte
 * container: pad_image(reflect) + patchify to X [M,192] (lrf/compression/svd.py:160-162), the top-R singular pairs
 * u = U sqrt(s), v = (sqrt(s) Vh)^T (:179-183; Gram matrix + eigen-solve instead of LAPACK, tolerance-checked) and
 * quantize(., uint8) of both (:185-187, lrf/compression/utils.py:185-220).
 *   U [B,M,R] uint8, V [B,192,R] uint8, qparams [B,4] float = (scale_u, min_u, scale_v, min_v), all device memory.
 *   sign optional [B,R] as in lrf_qmf_decompose_f32.
 */
int lrf_svd_encode_rgb_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, int R, const int8_t* sign,
                          uint8_t* U, uint8_t* V, float* qparams);

/*
 * svd_decode, RGB branch: dequantize (lrf/compression/utils.py:223-243), u @ v.mT, depatchify, unpad_image, to_dtype(uint8)
 * (lrf/compression/svd.py:310-326,359).  qparams6 [B,6] float (device) = (scale_u, min_u, qmin_u, scale_v, min_v, qmin_v)
 * where qmin is the smallest stored code of the tensor (dequantize subtracts `q.min()`).
 */
int lrf_svd_decode_rgb_u8(lrf_ctx* ctx, const uint8_t* U, const uint8_t* V, int64_t B, int64_t H, int64_t W, int R,
                          const float* qparams6, uint8_t* rgb);

/* svd_encode's RGB branch for the other patch sizes, patch=False and float factors (lrf/compression/svd.py:157-193): the host
 * forms the matrices with lrf_qmf_rgbspace_matrix_u8 (the same X, svd.py:160-167), takes u = U sqrt(s), v = (sqrt(s) Vh)^T from
 * lrf_qmf_svd_init_f32 (any shape) and, unless dtype is a float type, quantises each factor tensor as a whole:
 *   lrf_quantize_u8: quantize(t, uint8) (lrf/compression/utils.py:185-220) of B tensors of `per` floats each:
 *                    scale = (max - min) / 255, q = clamp((t - min) / scale + 0, 0, 255) truncated; qparams [B][2] = (scale, min).
 *   lrf_svd_decode_any_u8: svd_decode of those streams (svd.py:310-326, 359); U / V uint8 with qparams6 [B][6] = (scale_u, min_u,
 *                    qmin_u, scale_v, min_v, qmin_v), or float factors (factors_are_float, qparams6 NULL); layouts as
 *                    lrf_qmf_rgbspace_decode_any_u8.
 * The YCbCr branch of svd_encode is not built: in the reference it raises TypeError for an integer rank (svd.py:234, 267) and
 * its streams do not decode ("padded size" is appended twice per plane, svd.py:226,237, so svd_decode reads the wrong entry). */
int lrf_quantize_u8(lrf_ctx* ctx, const float* T, int64_t B, int64_t per, uint8_t* Q, float* qparams);
int lrf_svd_decode_any_u8(lrf_ctx* ctx, const void* U, const void* V, int factors_are_float, int64_t B, int64_t H, int64_t W, int p, int q,
                          int R, const float* qparams6, uint8_t* rgb);

/* ---------------------------------------------------------------------------------------------------
 * QMF, RGB colour-space branch: qmf_encode(color_space="RGB", patch=True, patch_size=(8,8))
 * (lrf/compression/qmf.py:164-187).  One matrix X [M,192] per image (reflect padding to multiples of 8, rows =
 * patches in row-major order, columns = (c, p, q)), rank R = max(round(min(M,192) * quality / 100), 1) chosen by
 * the host, QMF(rank=R, bounds, factor=(0,1)).decompose, int8 factors U [B,M,R], V [B,192,R] (device memory).
 *   U0 [B,M,R] / V0 [B,192,R] fp32 (device), both or neither: the initial factors (lrf/factorization/qmf.py:42-71);
 *   NULL = this library's SVD initialisation (sign optional [B,R] as in lrf_qmf_decompose_f32).
 * Ranks up to 192 (the reference's colour-space ablation sweeps quality 0..10 -> R <= 19), K >= 1.
 * The factorisation runs on the any-shape kernels (lrf_anyshape_kernels.hip).
 */
int lrf_qmf_rgbspace_encode_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, int R, int K, int lo, int hi,
                               const int8_t* sign, const float* U0, const float* V0, int8_t* U, int8_t* V);

/* qmf_decode, RGB colour-space branch (lrf/compression/qmf.py:311-323, :351): u @ v.mT, depatchify, unpad_image,
 * to_dtype(uint8).  rgb [B,3,H,W] uint8 (device). */
int lrf_qmf_rgbspace_decode_u8(lrf_ctx* ctx, const int8_t* U, const int8_t* V, int64_t B, int64_t H, int64_t W, int R, uint8_t* rgb);

/* The RGB colour-space branch for the other patch sizes and for patch=False (lrf/compression/qmf.py:164-212, decode :309-323).
 * The host forms the matrices with lrf_qmf_rgbspace_matrix_u8, factorises them with lrf_qmf_decompose_f32 /
 * lrf_qmf_bcd_f32 / lrf_qmf_svd_init_f32 (any shape) and decodes with lrf_qmf_rgbspace_decode_any_u8.
 *   p, q > 0: X [B, M, 3 p q] — reflect-padded image, rows = patches, columns in (c, a, b) order (qmf.py:167-169);
 *   p = q = 0 (patch=False): X [B, 3, H, W], the channel planes as three matrices per image (qmf.py:193-194), factors
 *   U [B,3,H,R], V [B,3,W,R].  lrf_rgbspace_dims_any: padded size and the matrix shape [M, N] (p = 0: M = H, N = W). */
int lrf_rgbspace_dims_any(int64_t H, int64_t W, int p, int q, int64_t* hp, int64_t* wp, int64_t* M, int64_t* N);
int lrf_qmf_rgbspace_matrix_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, int p, int q, float* X);
int lrf_qmf_rgbspace_decode_any_u8(lrf_ctx* ctx, const int8_t* U, const int8_t* V, int64_t B, int64_t H, int64_t W, int p, int q, int R,
                                   uint8_t* rgb);

/* ---------------------------------------------------------------------------------------------------
 * The same branch for images of another channel count: qmf_encode(image[C,H,W], color_space="RGB") takes any C, because
 * patchify "c (h p) (w q) -> (h w) (c p q)" infers c (lrf/compression/qmf.py:43-56, :164-212) and qmf_decode infers it from
 * the factor shapes (:309-323).  The three-channel entries above keep their code; these serve gray and n-channel images.
 *
 * lrf_chan_dims: the geometry (host only).  Reflect padding to multiples of (p, q) with top = pad / 2, left = pad / 2
 *   (lrf/compression/utils.py:108-132), M = (hp / p)(wp / q), N = C p q; p = q = 0 (patch=False): hp, wp, M, N = H, W, H, W per
 *   channel.  Refuses what lrf_rgbspace_dims_any refuses, C outside [1, 16], sides above 2^20 and patches above 1024. */
int lrf_chan_dims(int64_t H, int64_t W, int64_t C, int p, int q, int64_t* hp, int64_t* wp, int64_t* M, int64_t* N);

/* Gray images, 8x8 patches, K >= 1 (qmf.py:164-187 with c = 1): the image is ONE matrix X [M,64] of uint8-valued floats, the
 * shape of the tuned 64-column kernels.  A planes kernel (uint8 -> float, reflect padding, patchify) writes X into the context's
 * X workspace; the call then runs what lrf_qmf_decompose_f32 runs for N = 64 on that X (U0 / V0 NULL; sign optional [B,R]), or what
 * lrf_qmf_bcd_f32 runs (U0 [B,M,R], V0 [B,64,R] fp32, both or neither), ranks above the tuned ones included.  The factors
 * U [B,M,R], V [B,64,R] int8 are those entries' on the same X, bit for bit.  gray [B,H,W] uint8 (device). */
int lrf_qmf_encode_gray_u8(lrf_ctx* ctx, const uint8_t* gray, int64_t B, int64_t H, int64_t W, int R, int K, int lo, int hi,
                           const int8_t* sign, const float* U0, const float* V0, int8_t* U, int8_t* V);

/* qmf_decode of those streams (qmf.py:311-323, :351 with c = 1): clamp(sum_r U[m,r] V[n,r], 0, 255), depatchify, centre crop.
 * int32 sums of int8 products: exact for any int8 factors and any R <= LRF_MAX_RANK.  gray [B,H,W] uint8 (device). */
int lrf_qmf_decode_gray_u8(lrf_ctx* ctx, const int8_t* U, const int8_t* V, int64_t B, int64_t H, int64_t W, int R, uint8_t* gray);

/*
 * The resident-factor loader for gray images: lists of gray 8x8 streams that differ in size and rank, decoded whole, at
 * 1/2, 1/4, 1/8 scale, as windows and as resized crops, in one call each — the gray counterparts of
 * lrf_qmf_decode_ragged_rgb_u8, lrf_qmf_decode_scaled_rgb_u8, lrf_qmf_decode_scaled_crops_rgb_u8 and
 * lrf_qmf_decode_resized_crops_rgb_u8 with their _tensor forms.  One plane, no chroma, no colour conversion, no floating point
 * before the tensor format: every byte below is defined in exact integers.
 *   P        the int32 plane of an image: sum_r U[m,r] V[n,r], depatchified, centre-cropped to H x W (the padding of
 *            lrf_chan_dims(H, W, 1, 8, 8): top = pad / 2, left = pad / 2)
 *   level 1  L1 = clamp(P, 0, 255): the bytes of lrf_qmf_decode_gray_u8
 *   level f  f = 2, 4, 8: Hs x Ws = ceil(H / f) x ceil(W / f) (lrf_scaled_dims).  Output pixel (i, j) covers image rows
 *            f i .. min(f i + f, H) - 1 and the columns likewise (n pixels, 1..64: the partial blocks at the bottom and right
 *            edge hold the pixels that exist); s = the sum of P over them (|s| <= 2^26: int32 is exact);
 *            Lf = clamp(s, 0, 255 n) / n, the integer quotient.  The pooling comes before the clamp, as in the colour decoder.
 *   images   [n] descriptors in host memory: U [M][R] at u_off, V [64][R] at v_off (int8 elements), 1 <= R <= 64
 * lrf_qmf_decode_gray_ragged_u8: image i at level `scale` (1, 2, 4 or 8) is written as [Hs_i][Ws_i] bytes at out_off.
 * lrf_qmf_decode_gray_crops_u8: window j = rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of level `scale` of image `image`
 *   (lrf_scaled_crop; scale 1 is allowed here, so one call serves crops of mixed levels), written as [h][w] at h w j.
 * lrf_qmf_decode_gray_resized_crops_u8: box j of lrf_resized_crop resampled to (oh, ow) by exactly the level rule, the taps and
 *   the blend of lrf_qmf_decode_resized_crops_rgb_u8 with L the gray level above, written as [oh][ow] at oh ow j.  So a box of
 *   the output's size is the plain crop, a box with y0, x0 multiples of f, h = f oh and w = f ow the crop of level f at
 *   (y0 / f, x0 / f), and flip mirrors the columns.
 * The _tensor forms write lrf_tensor_format's chain for one channel instead of the byte b: t = fl32(float(b) * scale[0]),
 *   v = fl32(t + bias[0]), rounded to nearest even into dtype — not an fma.  Only element 0 of scale and bias is used (all
 *   six must be finite); for one channel NCHW and NHWC are the same memory, so `layout` is validated and otherwise immaterial.
 * An image's, a window's or a box's bytes depend on nothing else in the call.  Launches: one per level present for the ragged
 * and the crops entries (at most 4), one per (path, level) for the resized crops (at most 8; the staged path decodes a tile's
 * footprint into LDS once, boxes whose footprint does not fit take one output pixel per thread).
 * Asynchronous on the context's stream (a caller's stream after lrf_ctx_set_stream) and timed under LRF_K_DECODE.  The image
 * descriptors stay on the device between calls, keyed on their bytes, in a table of their own (the first call of a new image
 * list uploads them and waits for the stream; lrf_ctx_trim releases them); the item lists travel stream-ordered through the
 * pinned staging slots of lrf_qmf_decode_crops_rgb_u8, with no stream wait.  Everything is validated on the host before any
 * launch, and a refused call writes nothing.  LRF_EINVAL: a NULL pointer, n / n_images outside [1,65535], n_crops outside
 * [1,2^20], a rank outside [1,64], a size lrf_chan_dims(H, W, 1, 8, 8) refuses or of 2^31 pixels or more, a negative offset, a
 * U, V or output range that leaves its buffer, a scale outside {1, 2, 4, 8}, h or w below 1, oh or ow outside [1,16384], a
 * crop whose image index is out of range or whose rectangle leaves its (scaled) image, 2^31 or more workgroups in one launch,
 * and for the _tensor forms what lrf_qmf_decode_crops_tensor lists for its format, `out` and out_bytes.
 */
typedef struct {
    int64_t H, W;
    int R;
    int64_t u_off, v_off, out_off; /* out_off: lrf_qmf_decode_gray_ragged_u8 alone */
} lrf_gray_image;
int lrf_qmf_decode_gray_ragged_u8(lrf_ctx* ctx, int64_t n, const lrf_gray_image* images /* host */, int scale, const int8_t* U, int64_t u_len,
                                  const int8_t* V, int64_t v_len, uint8_t* out, int64_t out_len);
int lrf_qmf_decode_gray_crops_u8(lrf_ctx* ctx, int64_t n_images, const lrf_gray_image* images /* host; out_off ignored */, const int8_t* U,
                                 int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops /* host */, int64_t h,
                                 int64_t w, uint8_t* out /* [n_crops][h][w] */, int64_t out_len);
int lrf_qmf_decode_gray_crops_tensor(lrf_ctx* ctx, int64_t n_images, const lrf_gray_image* images /* host; out_off ignored */, const int8_t* U,
                                     int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_scaled_crop* crops /* host */,
                                     int64_t h, int64_t w, const lrf_tensor_format* fmt /* host */, void* out, int64_t out_bytes);
int lrf_qmf_decode_gray_resized_crops_u8(lrf_ctx* ctx, int64_t n_images, const lrf_gray_image* images /* host; out_off ignored */, const int8_t* U,
                                         int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops, const lrf_resized_crop* crops /* host */,
                                         int64_t oh, int64_t ow, uint8_t* out /* [n_crops][oh][ow] */, int64_t out_len);
int lrf_qmf_decode_gray_resized_crops_tensor(lrf_ctx* ctx, int64_t n_images, const lrf_gray_image* images /* host; out_off ignored */,
                                             const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len, int64_t n_crops,
                                             const lrf_resized_crop* crops /* host */, int64_t oh, int64_t ow,
                                             const lrf_tensor_format* fmt /* host */, void* out, int64_t out_bytes);

/*
 * Lists of gray images on the encode side: images that differ in size and rank in one call, each image at a list of candidate
 * ranks in one call, and the squared error of gray factors against their sources — the gray counterparts of
 * lrf_qmf_encode_ragged_rgb_u8, lrf_qmf_encode_ragged_sweep_rgb_u8 and lrf_qmf_sse_ragged_rgb_u8.  A gray image is one matrix
 * X [M,64] (lrf_qmf_encode_gray_u8): no colour conversion, no chroma.
 *   gray     one uint8 buffer (device); image i is [H][W] bytes at gray_off
 *   sign     optional int8 buffer (device); sign_off -1 (or sign NULL): the default signs
 * lrf_qmf_encode_gray_ragged_u8: image i at rank R_i; U [M][R] at u_off, V [64][R] at v_off, its [R] signs at sign_off.  Its
 *   bytes are exactly those lrf_qmf_encode_gray_u8(B = 1, U0 = V0 = NULL) writes for that image alone with the same R, K, lo,
 *   hi and signs, whatever else the list holds and in whatever order.  It is the sweep below with one candidate per image.
 * lrf_qmf_encode_gray_ragged_sweep_u8: m candidates (image, R) over n images; candidate j's bytes are exactly those the ragged
 *   encode writes for (image, R) alone.  An image's signs are [Rmax], Rmax its largest candidate rank; a candidate uses the
 *   leading R of them and the leading R columns of the Rmax initialisation (the colour sweep's convention).  The planes stage,
 *   X, the Gram matrix and the initialisation run once per image; the X workspace is the sum over images, not candidates.
 * lrf_qmf_sse_gray_ragged_u8: sse[i] = sum over the H W samples of (source - clamp(P, 0, 255))^2, an exact integer: what
 *   lrf_qmf_decode_gray_ragged_u8 at scale 1 followed by lrf_image_metrics_u8(C = 1, ssim = NULL) gives.  items: lrf_gray_image
 *   with out_off naming where the SOURCE [H][W] is read in `gray`; ranks 1..64; several items may read one source.  Integer
 *   sums (uint32 per lane and wave, uint64 per workgroup, one 64-bit integer atomic per workgroup); sse [n] uint64 (device) is
 *   zeroed by the call on its stream; the item table travels through the pinned staging slots, with no stream wait.
 * The planes stage: at most two launches, timed under LRF_K_PLANES — images with W % 16 == 0 whose bytes start at a multiple
 * of 16 take lrf_qmf_encode_gray_u8's 16-byte body, the others its general body: X is the same bits either way.  The scorer
 * is timed under LRF_K_DECODE.  Asynchronous on the context's stream (a caller's stream after lrf_ctx_set_stream); a new list
 * uploads its tables and waits once.  Everything is validated on the host before any launch or write, and a refused call writes
 * nothing.  LRF_EINVAL: a NULL pointer, n outside [1,65535], m outside [n,2^20], a candidate naming no image, an image without
 * a candidate, a size lrf_chan_dims(H, W, 1, 8, 8) refuses, a rank below 1, bounds outside int8, a negative offset, pixels,
 * signs or factors that leave their buffer, overlapping factor ranges.  LRF_ENOTSUP: K < 1, an encode rank above 32 (those
 * iterate on the any-shape kernels: lrf_qmf_encode_gray_u8 per image), an image of 2^31 pixels or more, 2^31 or more blocks or
 * workgroups in a launch.
 */
typedef struct {
    int64_t H, W;
    int64_t gray_off, sign_off; /* sign_off -1: default signs */
} lrf_gray_sweep_image;
typedef struct {
    int32_t image;
    int R; /* 1..32 */
    int64_t u_off, v_off;
} lrf_gray_sweep_candidate;
int lrf_qmf_encode_gray_ragged_sweep_u8(lrf_ctx* ctx, int64_t n, const lrf_gray_sweep_image* images /* host */, int64_t m,
                                        const lrf_gray_sweep_candidate* cands /* host */, const uint8_t* gray, int64_t gray_len, int K, int lo,
                                        int hi, const int8_t* sign /* optional */, int64_t sign_len, int8_t* U, int64_t u_len, int8_t* V,
                                        int64_t v_len);
typedef struct {
    int64_t H, W;
    int R;
    int64_t gray_off, u_off, v_off, sign_off;
} lrf_gray_encode_image;
int lrf_qmf_encode_gray_ragged_u8(lrf_ctx* ctx, int64_t n, const lrf_gray_encode_image* images /* host */, const uint8_t* gray, int64_t gray_len,
                                  int K, int lo, int hi, const int8_t* sign, int64_t sign_len, int8_t* U, int64_t u_len, int8_t* V, int64_t v_len);
int lrf_qmf_sse_gray_ragged_u8(lrf_ctx* ctx, int64_t n, const lrf_gray_image* items /* host; out_off = where the SOURCE [H][W] is read */,
                               const int8_t* U, int64_t u_len, const int8_t* V, int64_t v_len, const uint8_t* gray, int64_t gray_len,
                               uint64_t* sse /* [n], device */);

/* The general route, 1 <= C <= 16, any patch size or none (qmf.py:164-212, decode :309-323): the host forms the matrices with
 * lrf_qmf_chan_matrix_u8, factorises them with lrf_qmf_decompose_f32 / lrf_qmf_bcd_f32 / lrf_qmf_svd_init_f32 (any shape; their
 * limits and errors apply) and decodes with lrf_qmf_chan_decode_u8.
 *   p, q > 0: X [B, M, C p q], columns in (c, a, b) order; factors U [B,M,R], V [B,C p q,R];
 *   p = q = 0: X [B, C, H, W], C matrices per image; factors U [B,C,H,R], V [B,C,W,R].  img / out [B,C,H,W] uint8 (device).
 * For C = 1 with 8x8 patches the matrix entry runs the planes stage of lrf_qmf_encode_gray_u8: the same X, into the caller's buffer. */
int lrf_qmf_chan_matrix_u8(lrf_ctx* ctx, const uint8_t* img, int64_t B, int64_t C, int64_t H, int64_t W, int p, int q, float* X);
int lrf_qmf_chan_decode_u8(lrf_ctx* ctx, const int8_t* U, const int8_t* V, int64_t B, int64_t C, int64_t H, int64_t W, int p, int q, int R,
                           uint8_t* out);

/* ---------------------------------------------------------------------------------------------------
 * YCbCr branch with any patch size, or none: qmf_encode(color_space="YCbCr", patch_size=(p,q)) and patch=False
 * (lrf/compression/qmf.py:227-262 and :264-286; swept by experiments/ablation_patchsize/eval.py:49-55).
 * The host forms the matrices of one plane, factorises them with lrf_qmf_decompose_f32 (any M, N, R) and decodes with
 * lrf_qmf_decode_any_u8.  p = q = 0 means patch=False: the matrix is the plane itself, [h, w].
 */

/* plane ch (0 = Y, 1 = Cb, 2 = Cr): size after chroma down-sampling, after reflect padding to multiples of (p,q)
 * (lrf/compression/utils.py:108-132), and the matrix shape [M, N] (N = p*q; p = 0: M = h, N = w) */
int lrf_plane_dims_any(int64_t H, int64_t W, int p, int q, int ch, int64_t* h, int64_t* w, int64_t* hp, int64_t* wp, int64_t* M,
                       int64_t* N);

/* rgb [B,3,H,W] uint8 -> X [B,M,N] fp32 for plane ch: rgb_to_ycbcr, chroma_downsampling(area), pad_image(reflect),
 * patchify (qmf.py:227-242 with patch_size = (p,q); :264-269 when p = 0).  Device pointers. */
int lrf_qmf_planes_any_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, int p, int q, int ch, float* X);

/* qmf_decode of that branch (qmf.py:325-351): per plane u @ v.mT, depatchify + unpad_image (p > 0), nearest chroma
 * up-sampling, ycbcr_to_rgb, to_dtype(uint8).  Uc [B,M_c,R_c], Vc [B,N_c,R_c] int8 per plane c; rgb [B,3,H,W] uint8. */
int lrf_qmf_decode_any_u8(lrf_ctx* ctx, const int8_t* U0, const int8_t* V0, const int8_t* U1, const int8_t* V1, const int8_t* U2,
                          const int8_t* V2, int64_t B, int64_t H, int64_t W, int p, int q, const int R[3], uint8_t* rgb);

/* ---------------------------------------------------------------------------------------------------
 * Host -> host pipelined encoder.  This is the protocol a caller of the reference experiences — a host tensor goes in,
 * the encoded factors come back on the host (lrf/utils/misc.py:90-100 times exactly that around `encoder(image)`;
 * experiments/comparison/eval.py:105-110 loops it over a dataset) — and the metric SURVEY.md section 8(d) defines.
 * A pipe owns `slots` encoder contexts (stream + scratch + device staging each).  A batch is cut into sub-batches of
 * `sub_batch` images (0 = chosen by the library: ~40 MB of input); sub-batch i runs on slot i % slots as
 *     H2D(rgb) -> lrf_qmf_encode_rgb_u8 -> D2H(U, V)
 * — the uploads of all sub-batches in order on one upload stream (each gets the whole link, the first lands early), the
 * kernels and the download on the slot's stream — so uploads, kernels and downloads of different sub-batches overlap.
 * Two slots are the measured optimum on MI355X (three or more streams of kernels plus the upload stream exceed the HIP
 * runtime's default of four hardware queues, and streams that share a queue serialise).
 *   rgb_host [B,3,H,W] uint8, U_host / V_host as lrf_qmf_encode_rgb_u8 lays them out, sign_host optional
 *   [B, R[0]+R[1]+R[2]] int8: HOST pointers.  Page-locked memory (lrf_host_alloc, lrf_host_register, or torch's
 *   pin_memory) is what lets the copies run asynchronously at link speed; pageable memory works, slowly.
 * The results equal lrf_qmf_encode_rgb_u8's on the same images bit for bit (images are independent).
 * A pipe is not thread-safe: one per (host thread, device), which is also the multi-GPU model (one process per GPU).
 */
typedef struct lrf_pipe lrf_pipe;
int lrf_pipe_create(int device, int slots /* 1..8 */, int64_t sub_batch /* images, 0 = auto */, lrf_pipe** out);
void lrf_pipe_destroy(lrf_pipe* pipe);
int lrf_pipe_slots(const lrf_pipe* pipe);
/* the encoder context of one slot (owned by the pipe): for lrf_ctx_profile* / lrf_ctx_kernel_time */
lrf_ctx* lrf_pipe_slot_ctx(lrf_pipe* pipe, int slot);
size_t lrf_pipe_workspace_bytes(const lrf_pipe* pipe);
/* whole batch, returns when every factor is in U_host / V_host */
int lrf_pipe_qmf_encode_rgb_u8_host(lrf_pipe* pipe, const uint8_t* rgb_host, int64_t B, int64_t H, int64_t W, const int R[3],
                                    int K, int lo, int hi, const int8_t* sign_host, int8_t* U_host, int8_t* V_host);
/* the same in two steps, so that the host can pack the container of finished sub-batches (lrf/compression/utils.py:354-455)
 * while the GPU works on the next ones: submit enqueues everything and returns the number of sub-batches; each
 * lrf_pipe_wait_next blocks until the next sub-batch (in order) is on the host and reports its image range
 * (n_images = 0: nothing left).  The host buffers must stay valid until the last wait returns. */
int lrf_pipe_qmf_encode_submit(lrf_pipe* pipe, const uint8_t* rgb_host, int64_t B, int64_t H, int64_t W, const int R[3], int K,
                               int lo, int hi, const int8_t* sign_host, int8_t* U_host, int8_t* V_host, int* n_sub);
int lrf_pipe_wait_next(lrf_pipe* pipe, int64_t* first_image, int64_t* n_images);

/* page-locked host memory for the pipe's callers (hosts without a GPU runtime of their own) */
int lrf_host_alloc(size_t bytes, void** out_host);
int lrf_host_free(void* host);
int lrf_host_register(void* host, size_t bytes);   /* page-locks memory the caller already owns */
int lrf_host_unregister(void* host);

/* The same three with an explicit chroma plane size hc x wc, for scale_factor other than (0.5, 0.5) (lrf/compression/qmf.py:230:
 * F.interpolate(scale_factor, mode="area") produces floor(H * s_h) x floor(W * s_w), which the host computes; the pooling
 * windows follow from the two sizes alone, lrf/compression/utils.py:92-94; decode :346-348 up-samples to the luma size with
 * mode="nearest").  hc, wc <= 0: the default halves. */
int lrf_plane_dims_any_hw(int64_t H, int64_t W, int64_t hc, int64_t wc, int p, int q, int ch, int64_t* h, int64_t* w, int64_t* hp,
                          int64_t* wp, int64_t* M, int64_t* N);
int lrf_qmf_planes_any_hw_u8(lrf_ctx* ctx, const uint8_t* rgb, int64_t B, int64_t H, int64_t W, int64_t hc, int64_t wc, int p, int q, int ch,
                             float* X);
int lrf_qmf_decode_any_hw_u8(lrf_ctx* ctx, const int8_t* U0, const int8_t* V0, const int8_t* U1, const int8_t* V1, const int8_t* U2,
                             const int8_t* V2, int64_t B, int64_t H, int64_t W, int64_t hc, int64_t wc, int p, int q, const int R[3],
                             uint8_t* rgb);

/* ---------------------------------------------------------------------------------------------------
 * Deflate of factor columns on the device: every column of n int8 matrices becomes a zlib stream (RFC 1950 / 1951, Huffman
 * only — literals and end-of-block, no matches) that any inflate reads.  The format, the choice between a dynamic, a fixed and
 * stored blocks, the code-length builder and the header's run-length rule are defined once, in lrf_amd/csrc/lrf_deflate_shared.h;
 * liblrf_pack.so restates the coder on the host from the same file (include/lrf_pack_deflate.h) and gives the same bytes.
 * Matrix i is [rows, cols] int8, row-major, at src + src_off (the layout lrf_qmf_encode_rgb_u8 and the ragged encoder write).
 * Column j's stream goes to the slot dst + dst_off + j * bound(rows), bound(len) = 2 + 5 * ceil(len / 65535) + len + 4 being the
 * most a stream can take (stored blocks), and its length to out_len[len_off + j]; no byte of a slot behind that length is written.
 * Everything is checked on the host before a launch: 1 <= n <= 2^20, 1 <= rows <= 2^30, 1 <= cols <= 4096, every range against
 * src_len, dst_len and out_len_count, no two matrices sharing slot bytes or length entries.  `mats` is host memory and free again
 * on return; the table goes to the device stream-ordered and the call does not wait for the stream.  One workgroup per column.
 */
typedef struct { int64_t src_off, rows, cols, dst_off, len_off; } lrf_deflate_matrix;
int64_t lrf_deflate_bound(int64_t len);
int lrf_deflate_columns_i8(lrf_ctx* ctx, const int8_t* src, int64_t src_len, int64_t n, const lrf_deflate_matrix* mats /* host */,
                           uint8_t* dst, int64_t dst_len, int32_t* out_len /* device */, int64_t out_len_count);

/* ---------------------------------------------------------------------------------------------------
 * The lengths of those streams without the streams: out_len[len_off + j] becomes exactly what lrf_deflate_columns_i8 would write
 * there for the same matrix, no other entry of out_len is written and no stream is written anywhere (dst_off is ignored).  A
 * stream's length is a function of its column's byte counts alone (lrfd_measure of lrf_amd/csrc/lrf_deflate_shared.h, the first
 * half of the coder's plan; liblrf_pack.so restates it on the host: lrf_pack_deflate_size_column_i8), so the kernel only counts:
 * one workgroup per LRF_DEFLATE_CG consecutive columns of a matrix reads the matrix once and measures its columns side by side.
 * The same host checks before the launch as above (n, rows, cols, negative offsets, every range against src_len and
 * out_len_count, no two matrices sharing length entries), the same stream-ordered table, no wait for the stream; asynchronous
 * and, like the call above, not timed under an LRF_K_* id.  LRF_ENOTSUP above INT32_MAX workgroups.
 */
#define LRF_DEFLATE_CG 8 /* columns per workgroup of the count */
int lrf_deflate_sizes_i8(lrf_ctx* ctx, const int8_t* src, int64_t src_len, int64_t n, const lrf_deflate_matrix* mats /* host; dst_off ignored */,
                         int32_t* out_len /* device */, int64_t out_len_count);

/* ---------------------------------------------------------------------------------------------------
 * Inflate of factor columns on the device: the reverse of the call above, for ANY zlib stream (RFC 1950 / 1951: stored, fixed
 * and dynamic blocks, matches up to distance 32,768, several blocks, the Adler-32) — the reference's level-9 streams as well as
 * lrf_deflate_columns_i8's.  The decoder is defined once, in lrf_amd/csrc/lrf_inflate_shared.h; liblrf_pack.so restates it on the
 * host from the same file (include/lrf_pack_inflate.h: lrf_pack_inflate_column_i8) and gives the same bytes and the same status.
 * `src` (device, src_len bytes) holds the streams: stream k is the col_len[k] bytes at src + col_off[k] (host arrays of ncols
 * entries).  Matrix i is [rows, cols] int8, row-major, at dst + dst_off; its column j is inflated from stream first + j and must
 * come to exactly `rows` bytes.  status[k] (device, ncols entries) becomes 0 or the LRFI_E_* of stream k; a refused stream leaves
 * unspecified bytes in its own column's elements and touches nothing else.
 * Everything is checked on the host before the launch, and a failed check (LRF_EINVAL) writes nothing: no NULL pointer,
 * 1 <= n <= 2^20, 1 <= rows <= 2^30, 1 <= cols <= 4096, every stream range inside src_len with col_len >= 8, every matrix inside
 * dst_len, no two matrices sharing dst bytes or stream indices, ncols equal to the sum of cols.  `mats`, `col_off` and `col_len`
 * are free again on return; the column table goes to the device stream-ordered and the call does not wait for the stream.  One
 * launch, one lane per stream (lrf_plan.h: plan_inflate orders them), timed under LRF_K_INFLATE.
 */
#define LRFI_E_HEADER 1     /* CMF / FLG: CM != 8, CINFO > 7, not a multiple of 31, or FDICT set */
#define LRFI_E_BTYPE 2      /* block type 3 */
#define LRFI_E_STORED 3     /* stored block: NLEN is not the complement of LEN */
#define LRFI_E_COUNTS 4     /* dynamic block: HLIT > 286 or HDIST > 30 */
#define LRFI_E_OVERSUB 5    /* an over-subscribed set of code lengths */
#define LRFI_E_INCOMPLETE 6 /* an incomplete set other than a single code of one bit */
#define LRFI_E_REPEAT 7     /* a repeat code with nothing to repeat, or one running past the lengths */
#define LRFI_E_NOEOB 8      /* dynamic block: no code for the end-of-block symbol */
#define LRFI_E_CODE 9       /* a bit pattern that is no code */
#define LRFI_E_LENSYM 10    /* literal/length symbol 286 or 287 */
#define LRFI_E_DISTSYM 11   /* distance symbol 30 or 31 */
#define LRFI_E_FAR 12       /* a distance reaching before the output's start */
#define LRFI_E_OVERRUN 13   /* more output than `rows` */
#define LRFI_E_SHORT 14     /* the stream ends with less output than `rows` */
#define LRFI_E_INPUT 15     /* the input is exhausted */
#define LRFI_E_ADLER 16     /* the Adler-32 does not match */
#define LRFI_E_CAP 17       /* the iteration cap (8 src_len + rows + 64) was reached: cannot happen while every step consumes or produces */
typedef struct { int64_t dst_off, rows, cols, first; } lrf_inflate_matrix;
int lrf_inflate_columns_i8(lrf_ctx* ctx, const uint8_t* src, int64_t src_len, int64_t n, const lrf_inflate_matrix* mats /* host */,
                           const int64_t* col_off /* host */, const int32_t* col_len /* host */, int64_t ncols, int8_t* dst, int64_t dst_len,
                           int32_t* status /* device */);

#ifdef __cplusplus
}
#endif
#endif /* LRF_HIP_H */
