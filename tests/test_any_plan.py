"""CPU suite: which kernel variant a call of the any-shape path takes, and with which loop counts (plan_any_prod, plan_any_gs,
plan_any_update, plan_any_init_chunk: lrf_amd/csrc/lrf_plan.cpp; executed by any_prod / any_update / any_run_init,
lrf_anyshape_host.inc).  The plan source needs no device: it is built here with g++ together with tests/any_plan_shim.cpp and
called through ctypes.

Expected values never come from the plan.  They are worked out by hand, in the tables and docstrings below, from the
thresholds of the source: blocks of LRF_KC = 384 of the contraction; thin products for ranks <= 16; `tpw` 16-row tiles per wave
doubled while ceil(I / 16) B / (2 tpw) >= 8192; `tiles` 64-row tiles per workgroup doubled while D <= 64 and ceil(I / 64) gy B /
(2 tiles) >= 4096; the 128 x 64 kernel for D > 32, I > 64, R > 16; ATen's order below 400 multiply-adds; 160 KB of LDS for the
Gauss-Seidel sweep; 2 GiB of eigen-solver work space per chunk of the initialisation.

The case tables of tests/_anyshape_at_size_worker.py (the GPU comparison with the oracle at these sizes) are imported: for every
GPU case this module states which variants and loop counts it reaches, and the last test asserts that together they reach all of
them."""
import ctypes
import os
import subprocess

import pytest

import _anyshape_at_size_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
LONG, SHORT4, SHORT8, SHORT16, BIG, TILED = "THIN_LONG", "THIN_SHORT4", "THIN_SHORT8", "THIN_SHORT16", "BIG", "TILED"
PROD_KERNELS = (LONG, SHORT4, SHORT8, SHORT16, BIG, TILED)   # enum AnyProdKernel
GS_KERNELS = ("GS_I8", "GS_F32_LDS", "GS_F32_NOLDS")          # enum AnyGsKernel
PROD = ("k", "nblk", "fold", "tpw", "tiles", "gx", "gy", "gz", "threads", "fold_gx", "native", "refused")
GS = ("k", "gx", "gy", "lds", "native_gs")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("any_plan") / "libany_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "any_plan_shim.cpp")])
    so = ctypes.CDLL(so)
    so.lrf_test_plan_any_init_chunk.restype = ctypes.c_long
    return so


def _prod_dict(v):
    d = dict(zip(PROD, v))
    d["k"] = PROD_KERNELS[d["k"]]
    return d


def _gs_dict(v):
    d = dict(zip(GS, v))
    d["k"] = GS_KERNELS[d["k"]]
    return d


def prod(lib, I, D, R, B, sai, sak, native=False, prod_small=False):
    out = (ctypes.c_long * len(PROD))()
    lib.lrf_test_plan_any_prod(I, D, R, B, ctypes.c_long(sai), ctypes.c_long(sak), int(native), int(prod_small), out)
    return _prod_dict(out)


def gs(lib, rows, R, B, int_rows, gs_f32=False):
    out = (ctypes.c_long * len(GS))()
    lib.lrf_test_plan_any_gs(rows, R, B, int(int_rows), int(gs_f32), out)
    return _gs_dict(out)


def update(lib, B, M, N, R, trans, int_rows=False, prod_small=False):
    """(product a, product b, sweep) of one factor update"""
    out = (ctypes.c_long * (2 * len(PROD) + len(GS)))()
    lib.lrf_test_plan_any_update(B, M, N, R, int(trans), int(int_rows), int(prod_small), 0, out)
    return _prod_dict(out[:len(PROD)]), _prod_dict(out[len(PROD):2 * len(PROD)]), _gs_dict(out[2 * len(PROD):])


def init_prod(lib, B, M, N, R):
    """the long factor of the initialisation (any_run_init): u0 = X e for tall matrices (N <= M), v0 = X^T e for wide ones"""
    return prod(lib, M, N, R, B, N, 1) if N <= M else prod(lib, N, M, R, B, 1, N)


def chunk(lib, n, Rc, B):
    return int(lib.lrf_test_plan_any_init_chunk(n, Rc, ctypes.c_long(B)))


# ---- the expectations, by hand -------------------------------------------------------------------------------------------------
# (M, N, R): {product: (kernel, blocks of 384 of its contraction, tpw (THIN_SHORT*) or tiles (TILED) or 1[, "native"])}
#   ua = x @ v      [M, R]: I = M, D = N        ub = v.mT @ v [R, R]: I = R, D = N
#   va = x.mT @ u   [N, R]: I = N, D = M        vb = u.mT @ u [R, R]: I = R, D = M
#   init: I = max side, D = min side.           A product folds exactly when it has more than one block.
# The rules, in the order any_prod applies them (native: D I R < 400 multiply-adds, always k_any_prod):
#   R <= 16, I <= 16, D > 64 -> THIN_LONG;  R <= 16, D <= 64, I >= 256 -> THIN_SHORT4 / 8 / 16 for D <= 16 / 32 / 64;
#   D > 32, I > 64, R > 16 -> BIG;  else TILED.
NATIVE = (TILED, 1, 1, "native")
# 256 x 512x768 at quality 20, 4x4: ceil(24576 / 16) = 1536 tiles; 1536 * 256 / (2 tpw) = 196608 / tpw >= 8192 up to tpw = 16
# (12288 at 16: the loop stops at its cap).  ub: 16 * 3 * 3 = 144 < 400: native.  24576 / 384 = 64 blocks.
Y4 = dict(ua=(SHORT4, 1, 16), ub=NATIVE, va=(LONG, 64, 1), vb=(LONG, 64, 1), init=(SHORT4, 1, 16))
# chroma: 384 tiles; 384 * 256 / 2 = 49152, / 4 = 24576, / 8 = 12288 -> tpw 8; / 16 = 6144 < 8192.  6144 / 384 = 16 blocks
C4 = dict(ua=(SHORT4, 1, 8), ub=NATIVE, va=(LONG, 16, 1), vb=(LONG, 16, 1), init=(SHORT4, 1, 8))
# 16x16: ub has I = 51 <= 64: TILED, ceil(51 / 32) = 2 column tiles; va contracts over 1536 = 4 blocks
Y16 = dict(ua=(BIG, 1, 1), ub=(TILED, 1, 1), va=(BIG, 4, 1), vb=(TILED, 4, 1), init=(BIG, 1, 1))
C16 = dict(ua=(BIG, 1, 1), ub=(TILED, 1, 1), va=(BIG, 1, 1), vb=(TILED, 1, 1), init=(BIG, 1, 1))  # [384, 256] R 26: 384 is one block
# 32x32: 1024 = 3 blocks (2.67); ub / vb have I = 77 > 64: BIG as well.  Wide: the initialisation's product is [1024, 77] over 384
Y32 = dict(ua=(BIG, 3, 1), ub=(BIG, 3, 1), va=(BIG, 1, 1), vb=(BIG, 1, 1), init=(BIG, 1, 1))
# chroma [96, 1024] R 10: rank <= 16, so never BIG; ua I = 96 (neither <= 16 nor D <= 64): TILED; ub I = 10, D = 1024: THIN_LONG;
# va I = 1024, D = 96 > 64: TILED (tiles stay 1: D > 64); vb I = 10, D = 96: THIN_LONG in one block, no fold
C32 = dict(ua=(TILED, 3, 1), ub=(LONG, 3, 1), va=(TILED, 1, 1), vb=(LONG, 1, 1), init=(TILED, 1, 1))
# patch=False: [512, 768] R 102: 768 and 512 are two blocks each; chroma [256, 384] R 26: one block each, I = 26: TILED
YN = dict(ua=(BIG, 2, 1), ub=(BIG, 2, 1), va=(BIG, 2, 1), vb=(BIG, 2, 1), init=(BIG, 2, 1))
CN = dict(ua=(BIG, 1, 1), ub=(TILED, 1, 1), va=(BIG, 1, 1), vb=(TILED, 1, 1), init=(BIG, 1, 1))
# 4x8 at quality 60: [12288, 32] R 19: rank > 16 but D = 32 is not > 32: TILED with 192 row tiles, one column tile:
# 192 * 256 / 2 = 24576, / 4 = 12288, / 8 = 6144 >= 4096 -> tiles 8 (the cap).  ub: one row tile, 256 / 2 = 128: tiles 1.
# va: I = 32 <= 64: TILED over 12288 = 32 blocks.
Y48 = dict(ua=(TILED, 1, 8), ub=(TILED, 1, 1), va=(TILED, 32, 1), vb=(TILED, 32, 1), init=(TILED, 1, 8))
# chroma [3072, 32] R 10: D = 32: THIN_SHORT8; 192 tiles of 16 rows: 192 * 256 / 2 = 24576, / 4 = 12288 -> tpw 4; / 8 = 6144 < 8192.
# ub I = 10 < 256, D = 32 <= 64: neither thin kernel: TILED.  va I = 32: TILED, 8 blocks; vb I = 10, D = 3072: THIN_LONG
C48 = dict(ua=(SHORT8, 1, 4), ub=(TILED, 1, 1), va=(TILED, 8, 1), vb=(LONG, 8, 1), init=(SHORT8, 1, 4))
# 48 x 6x8 at quality 20: [8256, 48] R 10: D = 48: THIN_SHORT16; 516 tiles: 516 * 48 / 2 = 12384 >= 8192, / 4 = 6192 < 8192: tpw 2.
# 8256 / 384 = 21.5: 22 blocks.  chroma [2064, 48] R 5: 129 tiles, 129 * 48 / 2 = 3096: tpw 1; 2064 / 384 = 5.4: 6 blocks;
# ub: 48 * 5 * 5 = 1200 >= 400: not native
Y68 = dict(ua=(SHORT16, 1, 2), ub=(TILED, 1, 1), va=(TILED, 22, 1), vb=(LONG, 22, 1), init=(SHORT16, 1, 2))
C68 = dict(ua=(SHORT16, 1, 1), ub=(TILED, 1, 1), va=(TILED, 6, 1), vb=(LONG, 6, 1), init=(SHORT16, 1, 1))
# 256 x 500x760 at 4x4: 125 * 190 = 23750 rows = 1484.4 tiles of 16: 1485, tpw 16, 93 waves a matrix, the last with 13 tiles;
# 23750 / 384 = 61.8: 62 blocks.  chroma 250x380 -> padded 252x380: 63 * 95 = 5985 rows = 374.1 tiles: 375, tpw 8 (375 * 256 / 16 =
# 6000 < 8192), 47 waves, the last with 7 tiles; 5985 / 384 = 15.6: 16 blocks
YR = dict(ua=(SHORT4, 1, 16), ub=NATIVE, va=(LONG, 62, 1), vb=(LONG, 62, 1), init=(SHORT4, 1, 16))
CR = dict(ua=(SHORT4, 1, 8), ub=NATIVE, va=(LONG, 16, 1), vb=(LONG, 16, 1), init=(SHORT4, 1, 8))
# name -> ((B, H, W), [(M, N)] of luma and chroma by lrf/compression/qmf.py's geometry, [luma, chroma] expectations)
BATCH_EXPECT = {
    "4x4": ([(24576, 16), (6144, 16)], [Y4, C4]), "4x4 signs": ([(24576, 16), (6144, 16)], [Y4, C4]),
    "16x16": ([(1536, 256), (384, 256)], [Y16, C16]),
    "32x32": ([(384, 1024), (96, 1024)], [Y32, C32]), "32x32 signs": ([(384, 1024), (96, 1024)], [Y32, C32]),
    "none": ([(512, 768), (256, 384)], [YN, CN]),
    "4x8 q60": ([(12288, 32), (3072, 32)], [Y48, C48]),
    "6x8": ([(8256, 48), (2064, 48)], [Y68, C68]),
    "4x4 ragged": ([(23750, 16), (5985, 16)], [YR, CR]),
}
# the general solver's shapes, three matrices per call.  [24576, 16]: 1536 * 3 / 2 = 2304 < 8192: tpw 1.  [5, 16] R 3: 16 * 5 * 3 =
# 240, 144, 240 and 5 * 3 * 3 = 45 multiply-adds: all four native.  [130, 100] R 101: every I > 64, D > 32: BIG in one block
GENERAL_EXPECT = {
    (24576, 16, 3): dict(ua=(SHORT4, 1, 1), ub=NATIVE, va=(LONG, 64, 1), vb=(LONG, 64, 1)),
    (1536, 256, 51): Y16, (96, 1024, 10): C32,
    (5, 16, 3): dict(ua=NATIVE, ub=NATIVE, va=NATIVE, vb=NATIVE),
    (130, 100, 101): dict(ua=(BIG, 1, 1), ub=(BIG, 1, 1), va=(BIG, 1, 1), vb=(BIG, 1, 1)),
}
# the rank ladder: [700, 660] and [660, 700], ranks above 64: every product BIG over 2 blocks (660 and 700 > 384), folded;
# the column tiles of 64 times the blocks: 2 ceil(R / 64)
LADDER_ALL = dict(ua=(BIG, 2, 1), ub=(BIG, 2, 1), va=(BIG, 2, 1), vb=(BIG, 2, 1), init=(BIG, 2, 1))
LADDER_GY = {121: 4, 128: 4, 129: 6, 192: 6, 256: 8, 257: 10, 400: 14, 512: 16, 629: 20, 630: 20, 639: 20}
# [300, 2048] R 200: 2048 / 384 = 5.3: 6 blocks (24 grid rows: four column tiles); the other side 300: one block.  Wide: init over 300
WIDE = dict(ua=(BIG, 6, 1), ub=(BIG, 6, 1), va=(BIG, 1, 1), vb=(BIG, 1, 1), init=(BIG, 1, 1))


GS_F32_LDS_MAX_RANK = 629  # by hand in test_gs_variant_flips_at_rank_630: 163540 bytes at 629 fit 163840, 164056 at 630 do not


def gs_kernel_by_hand(R, int_rows):
    """int8 rows after the first sweep; fp32 rows with the diagonal in LDS up to rank 629, without it above"""
    return "GS_I8" if int_rows else "GS_F32_LDS" if R <= GS_F32_LDS_MAX_RANK else "GS_F32_NOLDS"


def check_products(lib, B, M, N, R, want):
    """the plan of both updates (and of the initialisation's product, where expected) against the hand-made table; returns what
    the call reaches: {(kernel, 'fold' | 'no fold')}, {tpw}, {tiles}"""
    ua, ub, _ = update(lib, B, M, N, R, False)
    va, vb, _ = update(lib, B, M, N, R, True)
    got = dict(ua=ua, ub=ub, va=va, vb=vb)
    if "init" in want:
        got["init"] = init_prod(lib, B, M, N, R)
    kernels, tpws, tiles = set(), set(), set()
    for name, w in want.items():
        g = got[name]
        where = (B, M, N, R, name)
        assert (g["k"], g["nblk"]) == w[:2], (where, g)
        assert g["fold"] == (w[1] > 1) and not g["refused"], (where, g)
        assert (g["tpw"], g["tiles"]) == ((w[2], 1) if w[0].startswith("THIN_SHORT") else (1, w[2]) if w[0] == TILED else (1, 1)), (where, g)
        assert g["native"] == (len(w) > 3), (where, g)
        assert g["threads"] == (64 if w[0].startswith("THIN") else 256), (where, g)
        kernels.add((w[0], "fold" if w[1] > 1 else "no fold"))
        if w[0].startswith("THIN_SHORT"):
            tpws.add(w[2])
        if w[0] == TILED:
            tiles.add(w[2])
    return kernels, tpws, tiles


def decompose_gs(lib, B, M, N, R, K):
    """the sweeps of Context.decompose: fp32 rows in the first iteration, int8 rows from the second on; asserted against
    gs_kernel_by_hand for both factors"""
    seen = set()
    for it in range(min(K, 2)):
        for trans in (False, True):
            g = update(lib, B, M, N, R, trans, int_rows=it > 0)[2]
            assert g["k"] == gs_kernel_by_hand(R, it > 0), (B, M, N, R, it, trans, g)
            assert g["gy"] == B, g  # (grid rows and the native flag: literal values in test_production_batch_grids / test_native_mark)
            seen.add(g["k"])
    return seen


# ---- per GPU case: what it reaches ----------------------------------------------------------------------------------------------
def reached_by_batch_case(lib, case):
    name, (B, H, W_), ps, quality, ranks, _ = case
    shapes, want = BATCH_EXPECT[name]
    kernels, tpws, tiles, sweeps, chunks = set(), set(), set(), set(), set()
    for (M, N), R, w in zip(shapes, ranks[:2], want):
        k, t, s = check_products(lib, B, M, N, R, w)
        kernels |= k
        tpws |= t
        tiles |= s
        sweeps |= decompose_gs(lib, B, M, N, R, W.K_BATCH)
        c = chunk(lib, min(M, N), min(R, M, N), B)
        chunks.add((B + c - 1) // c)
    return dict(kernels=kernels, tpw=tpws, tiles=tiles, gs=sweeps, chunks=chunks)


def reached_by_ladder_case(lib, M, N, R, want):
    kernels, tpws, tiles = check_products(lib, 2, M, N, R, want)
    c = chunk(lib, min(M, N), min(R, M, N), 2)
    return dict(kernels=kernels, tpw=tpws, tiles=tiles, gs=decompose_gs(lib, 2, M, N, R, W.LADDER_K), chunks={(2 + c - 1) // c})


def reached_by_general_case(lib, shape):
    M, N, R = shape
    kernels, tpws, tiles = check_products(lib, W.GENERAL_B, M, N, R, GENERAL_EXPECT[shape])
    sweeps = set()
    for trans in (False, True):  # fp32 rows in every iteration
        g = update(lib, W.GENERAL_B, M, N, R, trans)[2]
        assert g["k"] == gs_kernel_by_hand(R, False)
        sweeps.add(g["k"])
    return dict(kernels=kernels, tpw=tpws, tiles=tiles, gs=sweeps, chunks=set())


def reached_by_chunked_case(lib, orient):
    """Context.svd_init only: no update, no sweep.  [1100, 4] = X [1100, 1024] e (or X^T e): rank <= 16 and I >= 256, but D = 1024 >
    64: k_any_prod over 3 blocks, folded; 254 matrices at 253 a chunk: two chunks, the second of one matrix"""
    M, N = W.CHUNK[orient]
    B, R = W.CHUNK["B"], W.CHUNK["R"]
    p = init_prod(lib, B, M, N, R)
    assert (p["k"], p["nblk"], p["fold"], p["tiles"], p["refused"]) == (TILED, 3, 1, 1, 0), p
    c = chunk(lib, min(M, N), R, B)
    assert (c, B - c) == (253, 1)
    return dict(kernels={(p["k"], "fold" if p["fold"] else "no fold")}, tpw=set(), tiles={p["tiles"]}, gs=set(), chunks={(B + c - 1) // c})


@pytest.mark.parametrize("case", W.BATCH_CASES, ids=[c[0] for c in W.BATCH_CASES])
def test_batch_case(lib, case):
    """the case's ranks and matrix shapes are the codec's; its products, sweeps and loop counts the hand-made ones"""
    from lrf_amd import _lib
    from lrf_amd.codec import anyshape_ranks
    name, (B, H, W_), ps, quality, ranks, _ = case
    assert tuple(anyshape_ranks((H, W_), ps, None, quality)) == tuple(ranks)
    dims = [tuple(d[4:6]) for d in _lib.plane_dims_any(H, W_, ps)]
    assert dims == [BATCH_EXPECT[name][0][0]] + [BATCH_EXPECT[name][0][1]] * 2
    r = reached_by_batch_case(lib, case)
    assert r["chunks"] == {1} and r["gs"] == {"GS_F32_LDS", "GS_I8"}


def test_production_batch_grids(lib):
    """256 x 512x768, 4x4 luma: 1536 tiles / 16 per wave = 96 waves a matrix; the fold of [16, 3] is one workgroup.  16x16 luma:
    [1536, 51] in 12 row tiles of 128 and one column tile of 64; x.mT @ u [256, 51] over 4 blocks: 2 x 4 x 256, folded by
    ceil(256 * 51 / 256) = 51 workgroups; b [51, 51]: one row tile, two column tiles of 32.  4x8 luma at tiles 8: 192 / 8 = 24."""
    ua, ub, g = update(lib, 256, 24576, 16, 3, False)
    assert (ua["gx"], ua["gy"], ua["gz"]) == (96, 256, 1)
    assert (g["gx"], g["gy"]) == (384, 256)
    va, _, g = update(lib, 256, 24576, 16, 3, True)
    assert (va["gx"], va["gy"], va["gz"], va["fold_gx"]) == (64, 256, 1, 1)
    assert g["native_gs"] == 1  # 2 * 16 = 32 < 400
    assert update(lib, 256, 6144, 16, 2, False)[0]["gx"] == 48
    ua, ub, _ = update(lib, 256, 1536, 256, 51, False)
    assert (ua["gx"], ua["gy"], ua["gz"]) == (12, 1, 256) and (ub["gx"], ub["gy"], ub["gz"]) == (1, 2, 256)
    va, vb, _ = update(lib, 256, 1536, 256, 51, True)
    assert (va["gx"], va["gy"], va["gz"], va["fold_gx"]) == (2, 4, 256, 51) and (vb["gx"], vb["gy"]) == (1, 8)
    assert update(lib, 256, 12288, 32, 19, False)[0]["gx"] == 24
    ua = update(lib, 256, 23750, 16, 3, False)[0]  # the ragged case: 93 waves for 1485 tiles, 13 in the last
    assert ua["gx"] == 93 and 1485 - 92 * 16 == 13
    ua = update(lib, 256, 5985, 16, 2, False)[0]
    assert ua["gx"] == 47 and 375 - 46 * 8 == 7


@pytest.mark.parametrize("name", ["32x32", "none"])
def test_large_patch_variants_do_not_depend_on_the_batch(lib, name):
    """32x32 and patch=False: the same kernels, blocks and loop counts from one image to 256 (the batch is a grid dimension only)"""
    case = [c for c in W.BATCH_CASES if c[0] == name][0]
    for B in (1, 2, 16, 64, 255, 256):
        reached_by_batch_case(lib, (name, (B,) + case[1][1:]) + case[2:])


def test_tpw_marks(lib):
    """[24576, 16]: 1536 tiles.  tpw 2 from 1536 B / 2 >= 8192: B >= 10.7; tpw 4 from B >= 21.3; 8 from 42.7; 16 from 85.3"""
    for B, tpw in ((1, 1), (10, 1), (11, 2), (21, 2), (22, 4), (42, 4), (43, 8), (85, 8), (86, 16), (4096, 16)):
        p = update(lib, B, 24576, 16, 3, False)[0]
        assert (p["k"], p["tpw"], p["gx"]) == (SHORT4, tpw, 1536 // tpw), (B, p)
    assert update(lib, 256, 255, 16, 3, False)[0]["k"] == TILED   # fewer than 256 rows: not the thin kernel
    assert update(lib, 256, 256, 16, 3, False)[0]["k"] == SHORT4
    assert update(lib, 256, 24576, 16, 17, False)[0]["k"] == TILED  # rank above 16: not the thin kernels
    assert update(lib, 256, 24576, 16, 3, False, prod_small=True)[0]["k"] == TILED  # the developer switch


def test_tiles_marks(lib):
    """[12288, 32] R 19: 192 row tiles, one column tile.  tiles 2 from 192 B / 2 >= 4096: B >= 42.7; 4 from 85.3; 8 from 170.7.
    A contraction above 64 never takes several tiles."""
    for B, tiles in ((1, 1), (42, 1), (43, 2), (85, 2), (86, 4), (170, 4), (171, 8), (4096, 8)):
        p = update(lib, B, 12288, 32, 19, False)[0]
        assert (p["k"], p["tiles"], p["gx"]) == (TILED, tiles, 192 // tiles), (B, p)
    assert update(lib, 4096, 1024, 96, 10, True)[0]["tiles"] == 1


def test_native_mark(lib):
    """400 multiply-adds: b of rank 5 over 16 columns is 16 * 25 = 400: not native; rank 4: 256: native.  The sweep: (R - 1) rows"""
    assert not update(lib, 2, 1000, 16, 5, False)[1]["native"] and update(lib, 2, 1000, 16, 4, False)[1]["native"]
    assert update(lib, 2, 11, 12, 3, False)[0]["native"] and not update(lib, 2, 12, 12, 3, False)[0]["native"]  # 396 and 432
    assert gs(lib, 133, 4, 1, False)["native_gs"] == 1 and gs(lib, 134, 4, 1, False)["native_gs"] == 0  # 399 and 402


def test_gs_variant_flips_at_rank_630(lib):
    """R 629: 64 * 629 * 4 = 161024 bytes of rows + 2516 of diagonal = 163540 <= 163840.  R 630: rows of 631 floats: 161536 + 2520 =
    164056 > 163840: k_any_gs<float, false> with the rows alone.  int8 rows at R 639: 64 * 4 * (160 | 1) = 41216, + 2556."""
    g = gs(lib, 700, 629, 2, False)
    assert (g["k"], g["lds"]) == ("GS_F32_LDS", 163540)
    g = gs(lib, 700, 630, 2, False)
    assert (g["k"], g["lds"]) == ("GS_F32_NOLDS", 161536)
    g = gs(lib, 700, 639, 2, False)
    assert (g["k"], g["lds"], g["gx"], g["gy"]) == ("GS_F32_NOLDS", 163584, 11, 2)
    g = gs(lib, 700, 639, 2, True)
    assert (g["k"], g["lds"]) == ("GS_I8", 41216 + 2556)
    assert gs(lib, 700, 639, 2, True, gs_f32=True)["k"] == "GS_F32_NOLDS"  # the developer switch
    for R in range(1, 640):
        assert gs(lib, 700, R, 2, False)["k"] == ("GS_F32_LDS" if R <= 629 else "GS_F32_NOLDS") == gs_kernel_by_hand(R, False)


def test_init_chunk(lib):
    """2 GiB / (8 (n^2 + 3 n Rc)) bytes.  n = 1024, Rc = 4: 2147483648 / 8486912 = 253.03: 253 matrices, below 256 — the GPU
    test's 254 matrices are chunks of 253 and 1.  n = 1024 at rank 1: 2147483648 / (8 * 1051648) = 255.2: below 256 at every rank.
    n = 1023: 2^31 / (8 (1046529 + 3069)) = 255.75; n = 1000, Rc = 4: 265.2.  n = 2048, Rc = 639: 2^31 / (8 * 8120320) = 33.06."""
    assert chunk(lib, 1024, 4, 65535) == 253 == (1 << 31) // (8 * (1024 * 1024 + 3 * 1024 * 4)) == W.CHUNK["chunk"]
    assert chunk(lib, 1024, 4, W.CHUNK["B"]) == 253 and W.CHUNK["B"] == 254 and W.CHUNK["R"] == 4
    assert chunk(lib, 1024, 4, 253) == 253 and chunk(lib, 1024, 4, 100) == 100
    assert chunk(lib, 1024, 1, 65535) == 255 and chunk(lib, 1023, 1, 65535) == 255 and chunk(lib, 1000, 4, 65535) == 265
    assert chunk(lib, 2048, 639, 65535) == 33
    for orient in ("tall", "wide"):
        assert min(W.CHUNK[orient]) == 1024
    sub = W.chunk_subset(254, 253)
    assert sub == list(range(0, 253, 16)) + [252, 253] and {252, 253} <= set(sub)


def test_launch_grid_refusal(lib):
    """65535 grid rows: k_any_prod at rank 639 has 20 column tiles: 3276 blocks (65520) pass, 3277 (65540) do not; k_any_prod_big has
    10: 6553 blocks pass, 6554 do not"""
    assert not prod(lib, 10, 3276 * 384, 639, 1, 1, 16)["refused"] and prod(lib, 10, 3276 * 384 + 1, 639, 1, 1, 16)["refused"]
    p = prod(lib, 100, 6553 * 384, 639, 1, 1, 128)
    assert p["k"] == BIG and not p["refused"] and p["gy"] == 65530
    assert prod(lib, 100, 6553 * 384 + 1, 639, 1, 1, 128)["refused"]


def test_gpu_cases_reach_every_variant(lib):
    """What tests/_anyshape_at_size_worker.py runs, case by case (each checked against the hand-made tables above), reaches: every
    product kernel, folded and not (the thin-short kernels never fold: their contraction is at most 64 < 384); tpw 1, 2, 4, 8
    and 16; several row tiles per workgroup; all three sweeps; an initialisation in more than one chunk."""
    reached = {}
    for case in W.BATCH_CASES:
        reached["batches " + case[0]] = reached_by_batch_case(lib, case)
    for M, N in W.LADDER_SHAPES:
        for R in W.LADDER_RANKS:
            r = reached[f"ladder [{M}, {N}] R={R}"] = reached_by_ladder_case(lib, M, N, R, LADDER_ALL)
            for trans in (False, True):
                a, b, _ = update(lib, 2, M, N, R, trans)
                assert a["gy"] == b["gy"] == LADDER_GY[R]
            assert r["gs"] == {"GS_I8", "GS_F32_LDS" if R <= 629 else "GS_F32_NOLDS"}
    assert max(LADDER_GY.values()) > 4
    for name, M, N, R, _ in W.LADDER_EXTRA:
        reached[f"ladder {name}"] = reached_by_ladder_case(lib, M, N, R, WIDE if name == "wide" else LADDER_ALL)
    for shape in W.GENERAL_SHAPES:
        reached["general " + str(shape)] = reached_by_general_case(lib, shape)
    for orient in ("tall", "wide"):
        reached["chunked " + orient] = reached_by_chunked_case(lib, orient)

    def union(key):
        return set().union(*[r[key] for r in reached.values()])
    kernels = union("kernels")
    want = {(k, f) for k in (LONG, BIG, TILED) for f in ("fold", "no fold")} | {(k, "no fold") for k in (SHORT4, SHORT8, SHORT16)}
    assert kernels == want, sorted(want ^ kernels)
    assert {k for k, _ in kernels} == set(PROD_KERNELS)
    assert union("tpw") == {1, 2, 4, 8, 16}
    assert max(union("tiles")) > 1
    assert union("gs") == set(GS_KERNELS)
    assert reached["ladder [700, 660] R=629"]["gs"] == {"GS_I8", "GS_F32_LDS"} and reached["ladder [700, 660] R=630"]["gs"] == {"GS_I8", "GS_F32_NOLDS"}
    assert max(union("chunks")) > 1
    # the general solver stays on fp32 rows in every iteration
    assert all(r["gs"] == {"GS_F32_LDS"} for n, r in reached.items() if n.startswith("general"))
