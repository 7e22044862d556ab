"""Case tables and definitions for the SVD baseline and the RGB colour-space kernels (lrf_svd_kernels.hip and the host code at
the top of lrf_any.hip).  Host only: tests/test_svd_cases.py holds these tables to what they claim, tests/test_svd_gpu.py
runs the kernels on them.

Definitions.  Encoders: the oracle run the way the library runs (oracle.rgb_matrix_any, oracle.svd_topr_u8 — the exact Gram
matrix and the restated eigen-solver —, oracle.quantize_u8 per factor tensor).  Decoders: oracle.svd_decode_any (dequantize,
the fp32 product, depatchify + centre crop, clamp + truncate) and oracle.rgb_decode_any (exact integers).

Long matrices.  Zero rows add nothing to X^T X, and u = X w is computed row by row, so the factors of a matrix that has
the rows of a compact Xc [m0,192] at `rows` and zeros elsewhere are Xc's v and Xc's u rows scattered among rows of +0
(a chain of fma(0, w, +0) stays +0).  m0 >= 192 keeps the rank cap min(M, N) of the eigen-solver the same for both.  A
100001-row matrix is then checked from a 300-row oracle run; tests/test_svd_cases.py holds the argument at 7681 rows.
"""
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lrf_amd", "csrc")


def source_constant(name):
    """an integer #define read out of the two sources under test"""
    for fn in ("lrf_svd_kernels.hip", "lrf_any.hip"):
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % re.escape(name), open(os.path.join(CSRC, fn)).read(), re.M)
        if m:
            return int(m.group(1))
    raise KeyError(name)


G192_ROWS = source_constant("LRF_G192_ROWS")          # rows per workgroup of k_gram192_u8
G192_MAX_ROWS = source_constant("LRF_G192_MAX_ROWS")  # above it: k_gram_blk (fp64), and the fp32 matrix for every rank


def chunking(M):
    """(chunks of k_gram192_u8, rows of the last one)"""
    n = (M + G192_ROWS - 1) // G192_ROWS
    return n, M - (n - 1) * G192_ROWS


ENC_RANKS = (1, 3, 8, 9, 12)  # <= 8: the byte matrix + k_prod192_u8; above: the fp32 matrix + k_any_prod
BYTES_RANK_MAX = 8


# ---- geometry (lrf/compression/utils.py:108-153) ------------------------------------------------------------------------
def pad_of(n, p):
    """(before, after) of the reflect padding of a side n to a multiple of p"""
    d = (p - n % p) % p
    return d // 2, d - d // 2


def side_is_legal(n, p):
    """reflect padding needs both pads smaller than the side"""
    a, b = pad_of(n, p)
    return n >= 1 and a < n and b < n


def smallest_legal(p):
    return next(n for n in range(1, p + 1) if side_is_legal(n, p))


def matrix_dims(H, W, ps):
    """(M, N) of the matrix of an H x W RGB image: patches ps = (p, q); None: per channel [H, W]"""
    if ps is None:
        return H, W
    p, q = ps
    return ((H + sum(pad_of(H, p))) // p) * ((W + sum(pad_of(W, q))) // q), 3 * p * q


def image_of_patch_matrix(X, hb, wb):
    """uint8 [3, 8 hb, 8 wb] whose 8 x 8 RGB patch matrix (rows (h, w), columns (c, p, q)) is X [hb wb, 192]"""
    return np.ascontiguousarray(X.reshape(hb, wb, 3, 8, 8).transpose(2, 0, 3, 1, 4).reshape(3, 8 * hb, 8 * wb)).astype(np.uint8)


def scattered(Xc, M, rows):
    """[M,192] fp32: the rows of the compact Xc [m0,192] at `rows`, zeros elsewhere"""
    rows = np.asarray(rows)
    assert Xc.shape == (len(rows), 192) and len(set(rows.tolist())) == len(rows) and rows.min() >= 0 and rows.max() < M
    X = np.zeros((M, 192), np.float32)
    X[rows] = Xc
    return X


def scatter_rows(u, M, rows):
    """the compact matrix's u [m0,R] among rows of +0"""
    out = np.zeros((M, u.shape[1]), np.float32)
    out[np.asarray(rows)] = u
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- encoders: expected quantised factors -------------------------------------------------------------------------------
def quantised(oracle, u, v):
    """(codes of u, codes of v, [scale_u, min_u, scale_v, min_v] fp32) as svd_encode stores them"""
    qu, su, mu = oracle.quantize_u8(u)
    qv, sv, mv = oracle.quantize_u8(v)
    return qu, qv, np.array([su, mu, sv, mv], np.float32)


# ---- dense matrices: [3, 8, 8 M] images of random bytes, and one padded image ----------------------------------------------
DENSE = {  # name -> (H, W); beside each: chunks of k_gram192_u8, rows of the last one (DENSE_CHUNKS, checked on the CPU)
    "m1537": (8, 8 * 1537),   # 2 chunks, last of 1
    "m3135": (8, 8 * 3135),   # 3, 63
    "m6209": (8, 8 * 6209),   # 5, 65
    "m9215": (8, 8 * 9215),   # 6, 1535
    "m9217": (8, 8 * 9217),   # 7, 1
    "pad13x12301": (13, 12301),  # reflect padding on both sides, 2 x 1538 = 3076 rows: 3, 4
}
DENSE_CHUNKS = {"m1537": (2, 1), "m3135": (3, 63), "m6209": (5, 65), "m9215": (6, 1535), "m9217": (7, 1), "pad13x12301": (3, 4)}


@functools.lru_cache(maxsize=None)
def dense_image(name):
    H, W = DENSE[name]
    return np.random.default_rng(sorted(DENSE).index(name) + 100).integers(0, 256, (3, H, W), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def dense_factors(oracle, name, R):
    """(u, v) fp32 of a dense case.  For these matrices (M >= 192, uint8-valued) oracle.svd_topr_any returns the same bits:
    its fp64 fma chains are exact on such integers and its rank cap is 192 too (tests/test_svd_cases.py checks it once)."""
    return oracle.svd_topr_u8(oracle.rgb_matrix_any(dense_image(name), (8, 8)), R)


# ---- scattered matrices on both sides of the LRF_G192_MAX_ROWS switch -----------------------------------------------------
SCATTERED = {"m100000": (250, 400), "m100001": (11, 9091)}  # name -> (hb, wb) patches, M = hb wb
SCATTERED_M0 = 300
SCATTERED_RANKS = (5, 12)


@functools.lru_cache(maxsize=None)
def scattered_case(name):
    """(Xc [300,192] fp32, rows [300] ascending, M): row 0 and row M - 1, both sides of the first chunk boundary, of the last
    chunk's start and of a 64-row block boundary inside the last chunk, the rest at random"""
    hb, wb = SCATTERED[name]
    M = hb * wb
    rng = np.random.default_rng(M)
    last = (chunking(M)[0] - 1) * G192_ROWS
    fixed = {0, M - 1, G192_ROWS - 1, G192_ROWS, last - 1, last, last + 63, last + 64}
    rest = [int(r) for r in rng.permutation(M) if int(r) not in fixed][:SCATTERED_M0 - len(fixed)]
    rows = np.array(sorted(fixed | set(rest)), dtype=np.int64)
    Xc = rng.integers(0, 256, (SCATTERED_M0, 192)).astype(np.float32)
    return Xc, rows, M


def scattered_image(name):
    Xc, rows, M = scattered_case(name)
    return image_of_patch_matrix(scattered(Xc, M, rows), *SCATTERED[name])


# ---- batches of three small images whose factor tensors are not multiples of 16 bytes ----------------------------------------
BATCH = [(40, 56, R) for R in (1, 3, 5, 9)] + [(16, 24, R) for R in (1, 3, 9)]  # M = 35: M R odd; M = 6: M R = 2 mod 4


def batch_images(H, W):
    """uint8 [3,3,H,W]: images 0 and 2 dim noise around a grey level, image 1 a full-range gradient with noise — its factors'
    extremes are far from its neighbours', which a k_minmax reading another image's rows would show"""
    rng = np.random.default_rng(H * 1000 + W)
    out = np.empty((3, 3, H, W), np.uint8)
    out[0] = rng.integers(118, 139, (3, H, W))
    out[2] = rng.integers(60, 75, (3, H, W))
    ramp = np.linspace(0, 255, H * W).reshape(H, W)
    out[1] = np.clip(np.stack([ramp, ramp[::-1], ramp.T.reshape(H, W)]) + rng.integers(-40, 41, (3, H, W)), 0, 255)
    out[1, 0, 0, 0], out[1, 1, -1, -1] = 0, 255
    return out


def image1_offset_bytes(M, R):
    """where image 1's fp32 u tensor starts behind image 0's"""
    return 4 * M * R


# ---- size residues --------------------------------------------------------------------------------------------------------
def _residues():
    t = {}
    t[(8, 8)] = [(H, W) for H in range(8, 16) for W in range(8, 16)] + [(h, 9) for h in range(4, 8)] + [(9, w) for w in range(4, 8)]
    t[(4, 4)] = [(H, W) for H in range(4, 8) for W in range(4, 8)] + [(2, 5), (5, 2), (3, 5), (5, 3)]
    t[(16, 16)] = [(H, W) for H in range(16, 32) for W in range(16, 32)] + [(6, 17), (17, 6)]
    t[(32, 32)] = [(n, n) for n in range(32, 64)] + [(32, 63), (63, 32), (12, 33), (33, 12)]
    t[(8, 16)] = [(8 + i % 8, 16 + i) for i in range(16)] + [(8, 31), (15, 16), (4, 17), (9, 6)]
    t[None] = [(5, 7), (37, 53), (64, 96)]
    return t


RESIDUES = _residues()
PATCH_SETTINGS = [(8, 8), (4, 4), (16, 16), (32, 32), (8, 16), None]
RESIDUE_CASES = [(ps, H, W) for ps in PATCH_SETTINGS for H, W in RESIDUES[ps]]


def case_id(ps, H, W):
    return ("nopatch" if ps is None else "p%dx%d" % ps) + "-%dx%d" % (H, W)


def residue_images(H, W, B=3):
    return np.random.default_rng(H * 4099 + W).integers(0, 256, (B, 3, H, W), dtype=np.uint8)


# largest rank each decoder entry takes, read out of the entries themselves (lrf_any.hip, include/lrf_hip.h)
def _any_max_rank():
    m = re.search(r"^#define\s+LRF_ANY_MAX_RANK\s+(\d+)", open(os.path.join(ROOT, "include", "lrf_hip.h")).read(), re.M)
    return int(m.group(1))


def _entry_max_rank(entry):
    """the N of the first `R > N` in the body of a C entry of lrf_any.hip"""
    src = open(os.path.join(CSRC, "lrf_any.hip")).read()
    body = src[src.index("\nint %s(" % entry):]
    m = re.search(r"\bR > (\w+)\)", body[:body.index("\n}\n")])
    return _any_max_rank() if m.group(1) == "LRF_ANY_MAX_RANK" else int(m.group(1))


ENTRY_MAX_RANK = {"svd_decode_rgb": _entry_max_rank("lrf_svd_decode_rgb_u8"), "qmf_rgbspace_decode": _entry_max_rank("lrf_qmf_rgbspace_decode_u8"),
                  "svd_decode_any": _entry_max_rank("lrf_svd_decode_any_u8"), "qmf_rgbspace_decode_any": _entry_max_rank("lrf_qmf_rgbspace_decode_any_u8")}


def decoder_ranks(entry, H, W, ps):
    """1, 7 and the widest: the number of columns of the matrix (3 p q; W without patches), capped by the entry"""
    return (1, 7, min(matrix_dims(H, W, ps)[1], ENTRY_MAX_RANK[entry]))


# ---- where the fp32 product of the definition is held to the reference's (torch.mm on the CPU, one thread) ------------------
def product_is_pinned(M, N, R):
    """lrf_oracle_mm_blas restates torch.mm's order for matrices of 16 rows or more (but for 48 columns past 768 ranks), for one
    rank, and for up to 7 ranks on two rows or more.  Elsewhere — few rows, a long contraction: every widest-rank case of
    the residue tables, M <= 4 — the reference's BLAS takes routines with orders of their own, and the kernels are held to
    the oracle's statement only.  tests/test_svd_cases.py checks the pinned shapes against torch's recorded products."""
    return (M >= 16 and not (N < 192 and R > 768)) or R == 1 or (M >= 2 and R <= 7)


# wide ranks where the product is pinned: 20 patch rows, reflect padding on both sides; 500 and 385 ranks take the two halves
WIDE = [((8, 8), 30, 37, 192), ((4, 4), 14, 18, 48), ((16, 16), 61, 70, 768), ((16, 16), 61, 70, 500), ((32, 32), 125, 130, 3072),
        ((8, 16), 30, 70, 384), ((8, 16), 30, 70, 385)]


def product_cases():
    """{key: (u, v)} fp32: the products recorded from torch in tests/golden/svd_product.json (tools/gen_golden_svd_product.py):
    one case per pinned (M, N, R) of the residue tables, every wide case, every case without patches ([3,H,R] @ [3,W,R].mT),
    and a single 8x8 patch at rank 2"""
    out, shapes = {}, set()
    for ps, H, W in RESIDUE_CASES:
        for R in sorted(set(decoder_ranks("svd_decode_any", H, W, ps))):
            M, N = matrix_dims(H, W, ps)
            if ps is None or (product_is_pinned(M, N, R) and (M, N, R) not in shapes):
                shapes.add((M, N, R))
                out[case_id(ps, H, W) + "-R%d" % R] = float_factors(H, W, ps, R, 0)
    for ps, H, W, R in WIDE:
        out["wide-" + case_id(ps, H, W) + "-R%d" % R] = float_factors(H, W, ps, R, 0)
    rng = np.random.default_rng(8)
    out["single-patch-R2"] = ((rng.normal(size=(1, 2)) * 9).astype(np.float32), (rng.normal(size=(192, 2)) * 9).astype(np.float32))
    return out


# ---- decoder factors: three images per case, every one clamping on both sides ------------------------------------------------
def factor_shapes(H, W, ps, R):
    M, N = matrix_dims(H, W, ps)
    return ((3, H, R), (3, W, R)) if ps is None else ((M, R), (N, R))


def pixels_of(X, H, W, ps):
    """[3,H,W] of the product matrix X ([M,N], or [3,H,W] itself without patches): depatchify + centre crop, any dtype"""
    if ps is None:
        return X
    p, q = ps
    (top, bot), (left, right) = pad_of(H, p), pad_of(W, q)
    Hp, Wp = H + top + bot, W + left + right
    x = X.reshape(Hp // p, Wp // q, 3, p, q).transpose(2, 0, 3, 1, 4).reshape(3, Hp, Wp)
    return x[:, top:top + H, left:left + W]


def _product(u, v, ps):
    return np.einsum("chr,cwr->chw", u, v) if ps is None else u @ v.T


def clamps_both_sides(img_values):
    """some pixel below 0, some strictly inside, some above 255 (with a margin of one grey level against fp32 rounding)"""
    x = np.asarray(img_values, dtype=np.float64)
    return bool((x < -1).any() and ((x > 1) & (x < 254)).any() and (x > 256).any())


def _drawn(seed, draw, H, W, ps):
    """the first draw of `draw(rng, variant)` -> (payload, u float64, v float64) whose product clamps on both sides; the v
    tensor (shared by the sizes of a patch setting) is only drawn anew, as the next variant, after 25 failures with one"""
    for attempt in range(200):
        payload, u, v = draw(np.random.default_rng(list(seed) + [attempt]), attempt // 25)
        if clamps_both_sides(pixels_of(_product(u, v, ps), H, W, ps)):
            return payload
    raise AssertionError("no clamping factors drawn")


def _seed(shape, ps, R, b, kind):
    return list(shape) + [0 if ps is None else ps[0] * 64 + ps[1], R, b, kind]


def dequantised(q, scale, minv):
    """dequantize in float64 (for drawing only; the definition is the oracle's fp32 one)"""
    return (q.astype(np.float64) - float(q.min())) * np.float32(scale) + np.float32(minv)


def _codes(rng, shape, lo):
    q = rng.integers(lo, 256, shape, dtype=np.uint8)
    q.flat[0], q.flat[-1] = lo, 255
    if q.size > 1 and rng.random() < 0.5:  # the extreme codes where the centre crop keeps them or not, as it falls
        rng.shuffle(q.reshape(-1))
    return q


def _quant_params(rng, R):
    """(scale, min) of factors in about [-a, a], a^2 sqrt(R) far above 255"""
    a = math.sqrt((450.0 if R <= 2 else 900.0) / math.sqrt(R)) * float(rng.uniform(0.8, 1.6))
    return float(np.float32(2 * a / 255 * rng.uniform(0.9, 1.1))), float(np.float32(-a))


# the v tensor of a patch setting does not depend on the image size: drawn once per (shape, rank, image), u per size
@functools.lru_cache(maxsize=None)
def _quant_v(shape, ps, R, b, variant):
    rng = np.random.default_rng(_seed(shape, ps, R, b, 10) + [variant])
    qv, pv = _codes(rng, shape, 3 if b == 2 else 0), _quant_params(rng, R)
    return qv, pv, dequantised(qv, *pv)


@functools.lru_cache(maxsize=None)
def _float_v(shape, ps, R, b, variant):
    rng = np.random.default_rng(_seed(shape, ps, R, b, 11) + [variant])
    v = (rng.normal(size=shape) * math.sqrt(500.0 / math.sqrt(R))).astype(np.float32)
    return v, v.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _int8_v(shape, ps, R, b, variant):
    rng = np.random.default_rng(_seed(shape, ps, R, b, 12) + [variant])
    v = rng.integers(-128, 128, shape)
    if R <= 2:  # a sum of one or two terms lands inside 0..255 only with small entries about
        v = np.where(rng.random(shape) < 0.4, rng.integers(-3, 4, shape), v)
    v = v.astype(np.int8)
    v.flat[0], v.flat[-1] = -128, 127
    return v, v.astype(np.float64)


@functools.lru_cache(maxsize=4096)
def quant_factors(H, W, ps, R, b):
    """(codes u, codes v, (scale_u, min_u), (scale_v, min_v)): uint8 codes over the full range (image 2 from 3 upwards, so the
    q.min() that dequantize subtracts is not 0 everywhere)"""
    su_shape, sv_shape = factor_shapes(H, W, ps, R)

    def draw(rng, variant):
        qv, pv, v64 = _quant_v(sv_shape, ps, R, b, variant)
        qu, pu = _codes(rng, su_shape, 3 if b == 2 else 0), _quant_params(rng, R)
        return (qu, qv, pu, pv), dequantised(qu, *pu), v64

    return _drawn(_seed((H, W), ps, R, b, 0), draw, H, W, ps)


@functools.lru_cache(maxsize=4096)
def float_factors(H, W, ps, R, b):
    """(u, v) fp32 with the same property"""
    su_shape, sv_shape = factor_shapes(H, W, ps, R)

    def draw(rng, variant):
        v, v64 = _float_v(sv_shape, ps, R, b, variant)
        u = (rng.normal(size=su_shape) * math.sqrt(500.0 / math.sqrt(R)) * float(rng.uniform(0.8, 1.6))).astype(np.float32)
        return (u, v), u.astype(np.float64), v64

    u, v = _drawn(_seed((H, W), ps, R, b, 1), draw, H, W, ps)
    if b == 0 and small_product(H, W, ps, R) and R >= 2:
        u, v = u.copy(), v.copy()
        u[0, 0], v[0, 0] = 0, 0
        (u[0, 0, 0], u[0, 0, 1]), (v[0, 0, 0], v[0, 0, 1]) = SMALL_PRODUCT_PIXEL
    return u, v


def small_product(H, W, ps, R):
    """patch=False makes u @ v.mT a batched product, and torch's CPU bmm takes its small-product kernel (every product rounded,
    then added) instead of BLAS when contraction x rows x columns < 400"""
    return ps is None and R * H * W < 400


# (1, a) . (c, b): a b = 1 + 36869 / 2^26 needs 27 bits and rounds up by 3 / 2^26; c = 1 - fp32(a b).  Products rounded one by
# one give c + fp32(a b) = 1.0, pixel 1; one fma chain gives fma(a, b, c) = 1 - 3 / 2^26 -> 1 - 2^-24, pixel 0.  Planted at
# pixel (0, 0, 0) of image 0.
SMALL_PRODUCT_PIXEL = ((np.float32(1), np.float32(1 + 2.0 ** -12)), (np.float32(-4609 / 2.0 ** 23), np.float32(1 + 5 * 2.0 ** -14)))


@functools.lru_cache(maxsize=4096)
def int8_factors(H, W, ps, R, b):
    """(u, v) int8: v over the full range, u sparse (about three small entries per row, one in ten of them -128 or 127), so
    that the exact sums fall on all three sides; |sum| <= R 128^2 < 2^24"""
    su_shape, sv_shape = factor_shapes(H, W, ps, R)

    def draw(rng, variant):
        v, v64 = _int8_v(sv_shape, ps, R, b, variant)
        keep = rng.random(su_shape) < min(1.0, 3.0 / R)
        small = rng.integers(-2, 3, su_shape)
        big = rng.choice(np.array([-128, 127]), su_shape)
        u = (keep * np.where(rng.random(su_shape) < 0.1, big, small)).astype(np.int8)
        return (u, v), u.astype(np.float64), v64

    return _drawn(_seed((H, W), ps, R, b, 2), draw, H, W, ps)


# ---- refusals: sizes whose reflect padding is not smaller than the image ----------------------------------------------------
def refused_sizes(ps):
    """every H (against a legal W) and W (against a legal H) below the smallest legal one"""
    p, q = ps
    return [(h, q + 1) for h in range(1, smallest_legal(p))] + [(p + 1, w) for w in range(1, smallest_legal(q))]


# ---- constant tensors -------------------------------------------------------------------------------------------------------
CONSTANT_IMAGES = [((24, 40), 77, 1), ((24, 40), 77, 3), ((13, 21), 200, 1), ((13, 21), 200, 3)]  # (H, W), value, rank
