"""The geometry sweep shared by tests/test_geometry.py (CPU) and tests/test_geometry_gpu.py: a second, independent definition of
the front end (image -> patch matrices) and of the decoder (int8 factors -> image) written with torch's own CPU operators alone,
the grids of sizes, ranks, scale factors and patch settings it is run on, and factors whose pixels stay clear of the clamp.

The definition follows the reference's qmf_encode / qmf_decode (lrf/compression/qmf.py and utils.py) step by step:
  planes   the RGB -> YCbCr matrix and the +128 offsets, F.interpolate(scale_factor=, mode="area") on Cb and Cr,
           F.pad(mode="reflect") with top = pad // 2, left = pad // 2, patchify by reshape + permute
  decode   u @ v.T, depatchify by reshape + permute, unpad from (padded - original) // 2, F.interpolate(size=, mode="nearest") on
           Cb and Cr, the YCbCr -> RGB matrix behind the -128 offsets, clamp(0, 255).to(uint8)
It shares no code with oracle/ or lrf_amd/ (this module imports neither).  All work here runs at one thread; the thread count is
put back afterwards.

The two 3 x 3 colour products are the one step that is NOT left to torch.einsum.  An fp32 einsum goes to the host's BLAS, and how a
BLAS sums three terms depends on the CPU it finds: on the hosts where the reference's fixtures were recorded (and on one of the two
hosts this suite runs on) it is the chain acc = fma(m[i][j], x[j], acc) over j = 0, 1, 2 from zero; on the other host values of a
random image's planes came out up to two ulp away.  So colour_product states that chain itself, each fused multiply-add evaluated
exactly: the product and the sum in float64, where both are exact (a TwoSum check raises if a sum ever is not), then one rounding to
float32.  It gives the same bits on every host.  ref_planes_einsum / the einsum= switch keep torch.einsum beside it:
tests/test_geometry.py holds the two within the four roundings that any order of an fp32 three-term sum can differ by, which pins
the matrices, their orientation and the offsets to torch's own operator.

Every kernel of the front end and of the decoders branches on the image size modulo 16 (paddings (8 - H % 8) % 8 and
(8 - (H // 2) % 8) % 8, crops from pad // 2, pooling windows 2 or 3 wide, the 16-aligned / strip / general bodies), so the main grid
is every residue pair once: RESIDUES.  The decode tests need pixels that are NOT clamped — a chroma row taken one off, a crop
offset off by one, another nearest index are invisible under a pixel at 0 or 255 — hence midrange_factors, and the mutants of
ref_decode that tests/test_geometry.py uses to show that such mistakes would change the expected bytes."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

# ---- the grids ----------------------------------------------------------------------------------------------------------------
RESIDUES = [(32 + i, 32 + j) for i in range(16) for j in range(16)]          # every (H mod 16, W mod 16) once
WIDE = [(32 + (5 * j) % 16, 512 + j) for j in range(16)]                     # more than 32 luma patches a row; every residue of H and of W once
DIAGONAL = [(32 + i, 32 + i) for i in range(16)]
# the five classes of the tiled decode bodies (0, 0, 1, 2, 4, 4), and a triple only the general kernel serves; (1,1,1), (7,3,3) and
# (8,8,5) are of ranks <= 8: DEC_R8 where no tiled body applies, the others DEC_ANY there
TRIPLES = [(1, 1, 1), (7, 3, 3), (8, 8, 5), (16, 8, 8), (26, 13, 13), (32, 16, 16), (64, 64, 64)]
WIDE_TRIPLES = [(7, 3, 3), (26, 13, 13), (64, 64, 64)]
# TRIPLES holds no triple of class 3 (luma <= 16 with chroma 9..16): the decode tests run this one too
CLASS3 = (16, 9, 16)
DECODE_TRIPLES = TRIPLES + [CLASS3]
SCALE_FACTORS = [(0.25, 0.25), (1.0, 1.0), (0.5, 0.25), (0.3, 0.7), (1 / 3, 2 / 3), (0.75, 0.6), (0.9, 0.11)]
PATCH_SETTINGS = [(8, 8), (4, 4), (16, 16), (8, 4), None]                      # None: patch=False
ANY_SIZES = [(H, W) for H in (33, 40, 47, 64, 97, 111) for W in (35, 48, 61, 100, 129)]
ANY_RANKS = (3, 2, 2)
MUTANTS = ("top", "left", "nearest")


def chroma_of(H, W, scale_factor=(0.5, 0.5)):
    """the size F.interpolate(scale_factor=) gives the chroma planes: floor(size * factor), in double"""
    return int(math.floor(float(H) * float(scale_factor[0]))), int(math.floor(float(W) * float(scale_factor[1])))


def plane_geometry(H, W, patch_size=(8, 8), chroma=None):
    """[(h, w, hp, wp, M, N)] of Y, Cb, Cr: plane size, padded size, rows and columns of the matrix that is factorised"""
    hc, wc = (H // 2, W // 2) if chroma is None else chroma
    out = []
    for h, w in ((H, W), (hc, wc), (hc, wc)):
        if patch_size is None:
            out.append((h, w, h, w, h, w))
        else:
            p, q = patch_size
            hp, wp = h + (p - h % p) % p, w + (q - w % q) % q
            out.append((h, w, hp, wp, (hp // p) * (wp // q), p * q))
    return out


def any_cases(scale_factor):
    """[(H, W, patch_size, chroma)] of ANY for one scale factor.  A combination whose chroma plane is smaller than a patch side is
    dropped: reflect padding is not defined there (F.pad raises when a padding is not smaller than the side)."""
    out = []
    for H, W in ANY_SIZES:
        hc, wc = chroma_of(H, W, scale_factor)
        for ps in PATCH_SETTINGS:
            if ps is not None and (hc < ps[0] or wc < ps[1]):
                continue
            if hc < 1 or wc < 1:
                continue
            out.append((H, W, ps, (hc, wc)))
    return out


def _one_thread(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        nt = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*a, **kw)
        finally:
            torch.set_num_threads(nt)
    return run


# ---- the definition -----------------------------------------------------------------------------------------------------------
# ITU-T T.871 (JFIF) full-range BT.601, the digits the reference carries
_TO_YCC = [[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]]
_TO_RGB = [[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]]


def _fma(a, b, c):
    """round(a * b + c) to float32 with one rounding, for float32 tensors: a * b is exact in float64 (24 + 24 bits), and so is the
    sum whenever it fits 53 bits — checked by TwoSum's error term, which is zero exactly then"""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    assert not bool(err.any()), "a float64 sum was not exact: colour_product cannot state this fused multiply-add"
    return s.float()


def colour_product(matrix, x, einsum=False):
    """[3, 3] x float32 [3, ...] -> float32 [3, ...]: row i is the chain acc = fma(matrix[i][j], x[j], acc), j = 0, 1, 2, from zero.
    einsum=True: torch.einsum instead (the host BLAS's order; for the gate that holds the two together)"""
    m = torch.tensor(matrix, dtype=torch.float32)
    if einsum:
        return torch.einsum("ck,k...->c...", m, x)
    rows = []
    for i in range(3):
        acc = torch.zeros_like(x[0])
        for j in range(3):
            acc = _fma(m[i, j], x[j], acc)
        rows.append(acc)
    return torch.stack(rows)


def _pads(n, p):
    pad = (p - n % p) % p
    return pad // 2, pad - pad // 2


@_one_thread
def ref_planes(img, scale_factor=(0.5, 0.5), patch_size=(8, 8), einsum=False):
    """uint8 [3,H,W] (tensor or array) -> [X_Y, X_Cb, X_Cr] float32 numpy: [M, p q] patch matrices, or the planes themselves [h, w]
    for patch_size None"""
    x = torch.as_tensor(np.asarray(img)).to(torch.float32)
    ycc = torch.tensor([0.0, 128.0, 128.0]).view(3, 1, 1) + colour_product(_TO_YCC, x, einsum)
    planes = [ycc[0:1]] + [F.interpolate(ycc[None, c:c + 1], scale_factor=tuple(scale_factor), mode="area")[0] for c in (1, 2)]
    assert tuple(planes[1].shape[-2:]) == chroma_of(x.shape[1], x.shape[2], scale_factor)
    out = []
    for pl in planes:
        if patch_size is None:
            out.append(pl[0].contiguous().numpy())
            continue
        p, q = patch_size
        (top, bottom), (left, right) = _pads(pl.shape[1], p), _pads(pl.shape[2], q)
        pl = F.pad(pl, (left, right, top, bottom), mode="reflect")
        _, hp, wp = pl.shape
        X = pl.reshape(hp // p, p, wp // q, q).permute(0, 2, 1, 3).reshape((hp // p) * (wp // q), p * q)
        out.append(X.contiguous().numpy())
    return out


def _nearest_half_up(pl, H, W):
    """the "nearest" mutant: source index round(y * (h / H)) with halves up, where F.interpolate's nearest mode takes the floor"""
    h, w = pl.shape[-2:]
    iy = torch.clamp(torch.floor(torch.arange(H, dtype=torch.float32) * (h / H) + 0.5).long(), max=h - 1)
    ix = torch.clamp(torch.floor(torch.arange(W, dtype=torch.float32) * (w / W) + 0.5).long(), max=w - 1)
    return pl[..., iy, :][..., ix]


def mutant_applies(mutant, H, W, patch_size=(8, 8), chroma=None):
    """top: the chroma planes have bottom padding; left: the luma plane has right padding (else the shifted crop would leave the
    padded plane); nearest: always"""
    if mutant == "nearest":
        return True
    if patch_size is None:
        return False
    g = plane_geometry(H, W, patch_size, chroma)
    return g[1][2] > g[1][0] if mutant == "top" else g[0][3] > g[0][1]


@_one_thread
def ref_decode(factors, H, W, patch_size=(8, 8), chroma=None, mutant=None, einsum=False, as_float=False):
    """factors [u_y, v_y, u_cb, v_cb, u_cr, v_cr] (integer arrays, u [M, R], v [N, R]) -> uint8 [3,H,W] numpy.  chroma: the chroma
    planes' size (None: floor(H / 2) x floor(W / 2)).  mutant: one deliberate mistake (MUTANTS), for the gates of the test data."""
    assert mutant is None or (mutant in MUTANTS and mutant_applies(mutant, H, W, patch_size, chroma))
    geo = plane_geometry(H, W, patch_size, chroma)
    planes = []
    for c, (h, w, hp, wp, M, N) in enumerate(geo):
        u = torch.from_numpy(np.array(factors[2 * c], dtype=np.float32))
        v = torch.from_numpy(np.array(factors[2 * c + 1], dtype=np.float32))
        assert tuple(u.shape) == (M, u.shape[1]) and tuple(v.shape) == (N, u.shape[1]), (c, tuple(u.shape), tuple(v.shape), M, N)
        X = u @ v.T
        if patch_size is not None:
            p, q = patch_size
            X = X.reshape(hp // p, wp // q, p, q).permute(0, 2, 1, 3).reshape(hp, wp)
            top, left = (hp - h) // 2, (wp - w) // 2
            if mutant == "top" and c > 0:
                top += 1
            if mutant == "left" and c == 0:
                left += 1
            X = X[top:top + h, left:left + w]
        assert tuple(X.shape) == (h, w)
        if c > 0:
            X = _nearest_half_up(X, H, W) if mutant == "nearest" else F.interpolate(X[None, None], size=(H, W), mode="nearest")[0, 0]
        planes.append(X)
    ycc = torch.stack(planes) + torch.tensor([0.0, -128.0, -128.0]).view(3, 1, 1)
    rgb = colour_product(_TO_RGB, ycc, einsum)
    if as_float:
        return rgb.numpy()  # the image before clamp and truncation, for the gate that holds colour_product and einsum together
    return torch.clamp(rgb, 0, 255).to(torch.uint8).numpy()


# ---- test data ----------------------------------------------------------------------------------------------------------------
def midrange_factors(rng, H, W, ranks, patch_size=(8, 8), chroma=None):
    """int8 [u_y, v_y, u_cb, v_cb, u_cr, v_cr] whose pixels stay clear of the clamp: every column from -2..2, then column 0 of luma
    U from 9..14 and of luma V from 8..12 (luma about 72..168), of chroma U from 10..12 and of chroma V from 10..11 (chroma about
    100..132, around the 128 that is grey)"""
    out = []
    for c, (_, _, _, _, M, N) in enumerate(plane_geometry(H, W, patch_size, chroma)):
        R = ranks[c]
        u = rng.integers(-2, 3, (M, R), dtype=np.int8)
        v = rng.integers(-2, 3, (N, R), dtype=np.int8)
        u[:, 0] = rng.integers(9, 15, M) if c == 0 else rng.integers(10, 13, M)
        v[:, 0] = rng.integers(8, 13, N) if c == 0 else rng.integers(10, 12, N)
        out += [u, v]
    return out


def flat_rows(f6):
    """[u_y, v_y, ...] -> (U, V): one image's rows in the encoder's layout, the planes' matrices back to back, row-major"""
    return np.concatenate([f.reshape(-1) for f in f6[0::2]]), np.concatenate([f.reshape(-1) for f in f6[1::2]])


def split_rows(U, V, H, W, ranks):
    """the inverse of flat_rows for 8 x 8 patches"""
    out, uo, vo = [], 0, 0
    for (_, _, _, _, M, N), R in zip(plane_geometry(H, W), ranks):
        out += [U[uo:uo + M * R].reshape(M, R), V[vo:vo + N * R].reshape(N, R)]
        uo, vo = uo + M * R, vo + N * R
    assert uo == U.size and vo == V.size
    return out


def _read_only(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def image(H, W, k=0):
    """seeded uint8 [3,H,W] tensor; k: which image of a batch"""
    g = torch.Generator().manual_seed(7919 * H + W + 1000003 * k)
    return torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g)


@functools.lru_cache(maxsize=None)
def planes(H, W, k=0):
    """ref_planes of image(H, W, k): computed once, shared, read-only"""
    return tuple(_read_only(x) for x in ref_planes(image(H, W, k)))


@functools.lru_cache(maxsize=None)
def factors(H, W, ranks, k=0):
    """midrange_factors of (H, W, ranks) from a seed of their own; k: which image of a batch"""
    return tuple(_read_only(f) for f in midrange_factors(np.random.default_rng([H, W, *ranks, k]), H, W, ranks))


@functools.lru_cache(maxsize=None)
def decoded(H, W, ranks, k=0):
    """ref_decode of factors(H, W, ranks, k): computed once, shared, read-only"""
    return _read_only(ref_decode(factors(H, W, ranks, k), H, W))


def saturated(img):
    """the share of an image's bytes at 0 or 255"""
    return float(np.mean((img == 0) | (img == 255)))


# ---- which kernel serves a size: restated by hand from the comments of decode_plan (lrf_amd/csrc/lrf_plan.cpp) and of
# lrf_qmf_planes_from_rgb_u8 (lrf_amd/csrc/lrf_encode8.hip), not by calling the library ---------------------------------------------
DEC_TILE16, DEC_STRIP, DEC_R8, DEC_ANY = range(4)
ENC_TILE16, ENC_STRIP22, ENC_STRIP23, ENC_STRIP32, ENC_STRIP33 = range(5)


def decode_group(H, W, ranks, aligned8=True):
    """(kind, class) of the decode body.  k_decode16 takes sides that are multiples of 16 (and 8-byte aligned output), k_decode_strip
    any height when the chroma columns fall four-aligned under the luma columns; both are instantiated for rank bounds (luma,
    chroma) (8,4) (8,8) (16,<=8) (<=16,16) (32,16) = classes 0..4.  Elsewhere ranks <= 8 take DEC_R8 and the rest DEC_ANY."""
    rcm = max(ranks[1], ranks[2])
    left_luma, left_chroma = ((8 - W % 8) % 8) // 2, ((8 - (W // 2) % 8) % 8) // 2
    sides16 = H % 16 == 0 and W % 16 == 0 and aligned8
    strip_ok = W % 2 == 0 and left_luma % 2 == 0 and (left_chroma - left_luma // 2) % 4 == 0
    if ranks[0] <= 32 and rcm <= 16 and (sides16 or strip_ok):
        if ranks[0] <= 8:
            cls = 0 if rcm <= 4 else (1 if rcm <= 8 else 3)
        elif ranks[0] <= 16:
            cls = 2 if rcm <= 8 else 3
        else:
            cls = 4
        return (DEC_TILE16 if sides16 else DEC_STRIP), cls
    return (DEC_R8 if max(ranks) <= 8 else DEC_ANY), 0


def planes_body(H, W, aligned8=True):
    """the planes kernel: k_planes16 for sides that are multiples of 16 on 8-byte aligned bytes, else k_planes_strip<KH, KW> with
    pooling windows 2 (even side) or 3 (odd side)"""
    if H % 16 == 0 and W % 16 == 0 and aligned8:
        return ENC_TILE16
    return ENC_STRIP22 + 2 * (H & 1) + (W & 1)


def per_strip(W):
    """workgroups per strip of the tiled bodies: 32 luma patches' width each"""
    return (-(-W // 8) + 31) // 32
