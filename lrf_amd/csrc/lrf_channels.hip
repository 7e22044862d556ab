// lrf_channels.hip — qmf_encode / qmf_decode for channel counts other than three: the reference's RGB colour-space branch takes
// [C,H,W] for any C (its patchify infers c: lrf/compression/qmf.py:43-56, :164-212; decode :309-323).  Two routes:
//   gray (C = 1, 8x8 patches, K >= 1): the image IS one [M,64] matrix of uint8-valued floats, so a planes kernel writes X into the
//       context's X workspace and the 64-column solver of lrf_qmf_decompose_f32 / lrf_qmf_bcd_f32 takes it from there
//       (decompose64 / bcd64, lrf_encode8.hip); k_gray_decode turns the factors back into pixels.
//   general (1 <= C <= 16, any patch size or none): matrix and decoder kernels around the any-shape entries, which the host calls.
// Kernels: lrf_channels_kernel.hip.  The resident-factor loader for gray images (lists of mixed sizes and ranks, levels 1/2/4/8,
// windows, resized crops, tensors) lives in lrf_gray_loader_host.inc / lrf_gray_loader_kernel.hip, the gray encode lists (images of
// mixed sizes and ranks, candidate ranks per image, the squared error of factors against their sources) in
// lrf_gray_encode_host.inc / lrf_gray_encode_kernel.hip; both are included at the end.
#include "lrf_host.h"
#include "lrf_channels_kernel.hip"
#include "lrf_decode_tensor_kernel.hip"
#include "lrf_gray_loader_kernel.hip"
#include "lrf_gray_encode_kernel.hip"

#define LRF_CHAN_MAX 16

struct ChanGeom {
    int hp, wp, top, left, nw;
    long M, N;
};

// reflect padding to multiples of (p, q), top = pad / 2 (lrf/compression/utils.py:108-132); p = q = 0: per channel the plane [H, W]
static int chan_geom(int64_t H, int64_t W, int64_t C, int p, int q, ChanGeom* g)
{
    if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return set_err(LRF_EINVAL, "image size %ldx%ld", (long)H, (long)W);
    if (C < 1 || C > LRF_CHAN_MAX) return set_err(LRF_EINVAL, "%ld channels: 1 to %d are served", (long)C, LRF_CHAN_MAX);
    if ((p == 0) != (q == 0) || p < 0 || q < 0 || p > 1024 || q > 1024) return set_err(LRF_EINVAL, "patch size (%d, %d)", p, q);
    if (p == 0) {
        g->hp = (int)H; g->wp = (int)W; g->top = 0; g->left = 0; g->nw = 0; g->M = H; g->N = W;
        return LRF_OK;
    }
    const int64_t ph = (p - H % p) % p, pw = (q - W % q) % q;
    if (ph / 2 >= H || ph - ph / 2 >= H || pw / 2 >= W || pw - pw / 2 >= W)
        return set_err(LRF_EINVAL, "reflect padding larger than the image (%ldx%ld, patches %dx%d)", (long)H, (long)W, p, q);
    g->hp = (int)(H + ph); g->wp = (int)(W + pw); g->top = (int)(ph / 2); g->left = (int)(pw / 2);
    g->nw = g->wp / q;
    g->M = (long)(g->hp / p) * (g->wp / q);
    g->N = (long)C * p * q;
    return LRF_OK;
}

static int chan_batch(int64_t B)
{
    return (B < 1 || B > 65535) ? set_err(LRF_EINVAL, "B=%ld out of range [1,65535]", (long)B) : LRF_OK;
}

// X [B,M,64] of B gray images on the context's stream
static int gray_planes(lrf_ctx* c, const uint8_t* gray, int64_t B, int64_t H, int64_t W, const ChanGeom& g, float* X)
{
    Prof p(c, LRF_K_PLANES);
    if (W % 16 == 0 && (reinterpret_cast<uintptr_t>(gray) & 15) == 0) {
        const long items = (long)(g.hp / 8) * (W / 16) * 8;
        hipLaunchKernelGGL(k_gray_planes16, dim3((unsigned)((items + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, gray, (int)H, (int)W, g.top,
                           items, X);
    } else {
        const long items = g.M * 16;
        hipLaunchKernelGGL(k_gray_planes, dim3((unsigned)((items + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, gray, (int)H, (int)W, g.top,
                           g.left, g.nw, items, X);
    }
    LAUNCH_CHECK();
    return LRF_OK;
}

extern "C" {

int lrf_chan_dims(int64_t H, int64_t W, int64_t C, int p, int q, int64_t* hp, int64_t* wp, int64_t* M, int64_t* N)
{
    if (!hp || !wp || !M || !N) return set_err(LRF_EINVAL, "NULL argument");
    ChanGeom g;
    int rc = chan_geom(H, W, C, p, q, &g);
    if (rc) return rc;
    *hp = g.hp; *wp = g.wp; *M = g.M; *N = g.N;
    return LRF_OK;
}

int lrf_qmf_encode_gray_u8(lrf_ctx* c, const uint8_t* gray, int64_t B, int64_t H, int64_t W, int R, int K, int lo, int hi, const int8_t* sign,
                           const float* U0, const float* V0, int8_t* U, int8_t* V)
{
    if (!c || !gray || !U || !V) return set_err(LRF_EINVAL, "NULL argument");
    if ((U0 == nullptr) != (V0 == nullptr)) return set_err(LRF_EINVAL, "U0 and V0 must be given together");
    ChanGeom g;
    int rc = chan_geom(H, W, 1, 8, 8, &g);
    if (rc) return rc;
    if ((rc = chan_batch(B))) return rc;
    if (H * W >= (1L << 31)) return set_err(LRF_ENOTSUP, "image too large for 32-bit pixel indexing");
    // the solver's own refusals before anything is launched (the any-shape entries behind ranks above the tuned ones repeat theirs)
    if (R <= LRF_MAX_RANK && (rc = check_params(g.M, LRF_PATCH_ELEMS, R, K, lo, hi))) return rc;
    LRF_ON_DEVICE(c);
    if ((rc = ensure(c, c->x, (size_t)B * g.M * 64 * sizeof(float)))) return rc;
    float* X = (float*)c->x.p;
    if ((rc = gray_planes(c, gray, B, H, W, g, X))) return rc;
    if (U0) {
        if (R > LRF_BIG_TO_ANY_RANK) return any_bcd(c, X, B, g.M, 64, R, K, lo, hi, U0, V0, U, V);
        return bcd64(c, X, B, g.M, R, K, lo, hi, U0, V0, U, V);
    }
    if (R > LRF_MAX_RANK) return any_decompose(c, X, B, g.M, 64, R, K, lo, hi, sign, U, V);
    return decompose64(c, X, B, g.M, R, K, lo, hi, sign, U, V);
}

int lrf_qmf_decode_gray_u8(lrf_ctx* c, const int8_t* U, const int8_t* V, int64_t B, int64_t H, int64_t W, int R, uint8_t* gray)
{
    if (!c || !U || !V || !gray) return set_err(LRF_EINVAL, "NULL argument");
    if (R < 1 || R > LRF_GRAY_DEC_MAX_RANK) return set_err(LRF_EINVAL, "rank %d out of range [1,%d]", R, LRF_GRAY_DEC_MAX_RANK);
    ChanGeom g;
    int rc = chan_geom(H, W, 1, 8, 8, &g);
    if (rc) return rc;
    if ((rc = chan_batch(B))) return rc;
    if (H * W >= (1L << 31)) return set_err(LRF_ENOTSUP, "image too large for 32-bit pixel indexing");
    LRF_ON_DEVICE(c);
    Prof p(c, LRF_K_DECODE);
    const int u_words = (R % 4 == 0 && (reinterpret_cast<uintptr_t>(U) & 3) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_gray_decode, dim3((unsigned)((g.M * 4 + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, U, V, (int)H, (int)W, g.top,
                       g.left, g.nw, (int)g.M, R, u_words, gray);
    LAUNCH_CHECK();
    return LRF_OK;
}

int lrf_qmf_chan_matrix_u8(lrf_ctx* c, const uint8_t* img, int64_t B, int64_t C, int64_t H, int64_t W, int p, int q, float* X)
{
    if (!c || !img || !X) return set_err(LRF_EINVAL, "NULL argument");
    ChanGeom g;
    int rc = chan_geom(H, W, C, p, q, &g);
    if (rc) return rc;
    if ((rc = chan_batch(B))) return rc;
    const long elems = p ? g.M * g.N : (long)C * H * W;
    if ((elems + 255) / 256 > INT32_MAX) return set_err(LRF_ENOTSUP, "matrix of %ld elements: more than 2^31 - 1 workgroups in one launch", elems);
    LRF_ON_DEVICE(c);
    if (C == 1 && p == 8 && q == 8 && H * W < (1L << 31)) return gray_planes(c, img, B, H, W, g, X); // the X lrf_qmf_encode_gray_u8 forms
    Prof pr(c, LRF_K_PLANES);
    hipLaunchKernelGGL(k_chan_matrix, dim3((unsigned)((elems + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, img, (int)C, (int)H, (int)W, p, q,
                       g.top, g.left, g.nw, elems, X);
    LAUNCH_CHECK();
    return LRF_OK;
}

int lrf_qmf_chan_decode_u8(lrf_ctx* c, const int8_t* U, const int8_t* V, int64_t B, int64_t C, int64_t H, int64_t W, int p, int q, int R,
                           uint8_t* out)
{
    if (!c || !U || !V || !out) return set_err(LRF_EINVAL, "NULL argument");
    if (R < 1 || R > LRF_ANY_MAX_RANK) return set_err(LRF_EINVAL, "rank %d out of range", R);
    ChanGeom g;
    int rc = chan_geom(H, W, C, p, q, &g);
    if (rc) return rc;
    if ((rc = chan_batch(B))) return rc;
    const long n = (long)C * H * W;
    if ((n + 255) / 256 > INT32_MAX) return set_err(LRF_ENOTSUP, "image of %ld samples: more than 2^31 - 1 workgroups in one launch", n);
    LRF_ON_DEVICE(c);
    const long u_img = (p ? g.M : (long)C * H) * R, v_img = (p ? g.N : (long)C * W) * R;
    Prof pr(c, LRF_K_DECODE);
    hipLaunchKernelGGL(k_chan_decode, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, c->stream, U, V, (int)C, (int)H, (int)W, p, q,
                       g.top, g.left, g.nw, u_img, v_img, R, out);
    LAUNCH_CHECK();
    return LRF_OK;
}

} // extern "C"

#include "lrf_gray_loader_host.inc"
#include "lrf_gray_encode_host.inc"
