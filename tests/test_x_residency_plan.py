"""CPU suite: which X of a k_bcd_p call stays in the Infinity Cache (plan_x_residency, lrf_amd/csrc/lrf_plan.cpp).  In table
order the chroma planes are kept on the default cache policy while their X bytes stay within the budget; every other block of
the call — luma, whether it comes from the image bytes or from fp32 X, and the planes from the first that passes the budget
on — is marked BlockDesc::x_nt and streams with non-temporal loads.  The policy applies to calls the rank <= 8 body of the
persistent kernel iterates, outside a pipe, whose X sources do not all fit the budget (a call that fits keeps all of it in the
cache by itself); with a budget of 0 nothing is marked and the tables are the ones the call had before the policy existed,
byte for byte.  No device: built here with g++ together with tests/x_residency_shim.cpp.

Expected values never come from the code under test: the kept planes are counted by hand from the plane sizes (a plane of M
rows holds 256 M bytes of fp32 X, 384 rows a block), the block table without marks is written out from its layout."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
FIRST_W0 = 1
# 256 images of 208x176 (the GPU suite's case): luma 26 x 22 = 572 rows, two blocks; chroma 13 x 11 = 143 rows, one block;
# 1024 blocks: the smallest call LRF_PERSIST=1 puts on the persistent kernel.  Table: 256 Y planes, 256 Cb, 256 Cr.
B, ML, MC = 256, 572, 143
PLANE = 256 * MC  # bytes of one chroma plane's X: 36608
# what the call reads in one pass: luma as three bytes an element from the image or as four from X, plus the chroma X
SOURCES_BYTES = B * ML * 64 * 3 + 2 * B * PLANE  # 46858240
SOURCES_FP32 = B * ML * 64 * 4 + 2 * B * PLANE   # 56229888
_SO = []


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("x_residency_plan") / "libx_residency_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "x_residency_shim.cpp")])
    _SO.append(so)
    return ctypes.CDLL(so)


def image_planes(nimg=B, ranks=(7, 3, 3), ml=ML, mc=MC):
    """the table of the fused encode (encode_rgb_prepare): all Y planes, then Cb, then Cr"""
    return [(ml if c == 0 else mc, ranks[c]) for c in range(3) for _ in range(nimg)]


def unmarked_blocks(planes):
    """the block table as add_plane lays it out: {plane, first row, block number, 0} per 384 rows of a plane"""
    rows = [(pi, 384 * b, b, 0) for pi, (M, _) in enumerate(planes) for b in range((M + 383) // 384)]
    return np.array(rows, dtype=np.int32)


def decide(lib, planes, keep_bytes, nluma, K=10, persist=1, piped=0, apply=1, from_bytes=1):
    """-> (policy on, kept planes, kept bytes, block table as int32 [nblocks][4], plane table bytes)"""
    n = len(planes)
    M = (ctypes.c_int * n)(*[p[0] for p in planes])
    R = (ctypes.c_int * n)(*[p[1] for p in planes])
    nblk = sum((p[0] + 383) // 384 for p in planes)
    blocks = np.full((nblk, 4), -1, dtype=np.int32)
    pl = np.zeros((n, 80), dtype=np.uint8)
    dec = (ctypes.c_int * 2)()
    kb = ctypes.c_long(-1)
    f = lib.lrf_test_plan_x_residency
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                                                          ctypes.c_void_p, ctypes.c_void_p]
    got = f(n, M, R, K, FIRST_W0, persist, nluma, from_bytes, piped, keep_bytes, apply, blocks.ctypes.data_as(ctypes.c_void_p),
            pl.ctypes.data_as(ctypes.c_void_p), dec, ctypes.byref(kb))
    assert got == nblk
    return bool(dec[0]), int(dec[1]), int(kb.value), blocks, pl


def expect_marks(planes, kept):
    """the block table with x_nt = 1 on every block of a plane outside `kept`"""
    want = unmarked_blocks(planes)
    want[:, 3] = [0 if pi in kept else 1 for pi in want[:, 0]]
    return want


def test_budget_zero_is_the_table_without_the_policy(lib):
    planes = image_planes()
    on, kept, nbytes, blocks, pl = decide(lib, planes, 0, B)
    _, _, _, blocks0, pl0 = decide(lib, planes, 0, B, apply=0)  # the tables as the call builds them, plan_x_residency not run
    assert (on, kept, nbytes) == (False, 0, 0)
    assert blocks.shape == (1024, 4)
    assert np.array_equal(blocks, unmarked_blocks(planes))
    assert blocks.tobytes() == blocks0.tobytes() and pl.tobytes() == pl0.tobytes()
    # a negative budget is no budget either
    assert decide(lib, planes, -1, B)[:3] == (False, 0, 0)


def test_plane_table_never_changes(lib):
    planes = image_planes()
    pl0 = decide(lib, planes, 0, B, apply=0)[4]
    for budget in (1, 300 * PLANE, SOURCES_BYTES - 1, 1 << 40):
        assert decide(lib, planes, budget, B)[4].tobytes() == pl0.tobytes(), budget


def test_budget_that_ends_between_cb_and_cr_of_one_image(lib):
    # all 256 Cb planes and the Cr planes of images 0..70 fit, 100 bytes are left: image 71 keeps its Cb plane (plane 256 + 71)
    # and streams its Cr plane (plane 512 + 71)
    planes = image_planes()
    budget = (256 + 71) * PLANE + 100
    on, kept, nbytes, blocks, _ = decide(lib, planes, budget, B)
    assert (on, kept, nbytes) == (True, 327, 327 * PLANE)
    assert np.array_equal(blocks, expect_marks(planes, set(range(256, 256 + 327))))
    by_plane = dict(zip(blocks[:, 0].tolist(), blocks[:, 3].tolist()))
    assert by_plane[256 + 71] == 0 and by_plane[512 + 71] == 1 and by_plane[512 + 70] == 0
    # a budget that ends in the middle of a plane keeps the planes in front of it
    on, kept, nbytes, blocks, _ = decide(lib, planes, 300 * PLANE + PLANE // 2, B)
    assert (on, kept, nbytes) == (True, 300, 300 * PLANE)
    assert np.array_equal(blocks, expect_marks(planes, set(range(256, 556))))


def test_budget_that_ends_on_a_plane_boundary(lib):
    planes = image_planes()
    on, kept, nbytes, blocks, _ = decide(lib, planes, 300 * PLANE, B)
    assert (on, kept, nbytes) == (True, 300, 300 * PLANE)
    assert np.array_equal(blocks, expect_marks(planes, set(range(256, 556))))
    on, kept, nbytes, blocks, _ = decide(lib, planes, 300 * PLANE - 1, B)  # one byte short of it
    assert (on, kept, nbytes) == (True, 299, 299 * PLANE)
    assert np.array_equal(blocks, expect_marks(planes, set(range(256, 555))))
    # smaller than the first chroma plane: the policy is on and every block streams
    on, kept, nbytes, blocks, _ = decide(lib, planes, PLANE - 1, B)
    assert (on, kept, nbytes) == (True, 0, 0) and np.array_equal(blocks, expect_marks(planes, set()))


def test_budget_for_all_keeps_every_chroma_plane_and_never_luma(lib):
    planes = image_planes()
    # (the last: room for all but one byte of what the call reads, luma from the bytes included — luma still streams)
    for budget in (512 * PLANE, 512 * PLANE + 1, SOURCES_BYTES - 1):
        on, kept, nbytes, blocks, _ = decide(lib, planes, budget, B)
        assert (on, kept, nbytes) == (True, 512, 512 * PLANE), budget
        assert np.array_equal(blocks, expect_marks(planes, set(range(256, 768)))), budget
        assert blocks[:512, 3].all() and not blocks[512:, 3].any()  # 2 x 256 luma blocks in front, 512 chroma blocks behind
    # luma from fp32 X is four bytes an element: the same budgets, and up to the larger sum
    for budget in (512 * PLANE, SOURCES_BYTES, SOURCES_FP32 - 1):
        on, kept, nbytes, blocks, _ = decide(lib, planes, budget, B, from_bytes=0)
        assert (on, kept, nbytes) == (True, 512, 512 * PLANE), budget
        assert np.array_equal(blocks, expect_marks(planes, set(range(256, 768)))), budget


def test_a_call_that_fits_the_budget_is_left_alone(lib):
    # everything the call reads in a pass fits: the cache keeps it without help, nothing is marked
    planes = image_planes()
    for budget, from_bytes in ((SOURCES_BYTES, 1), (1 << 40, 1), (SOURCES_FP32, 0), (1 << 40, 0)):
        on, kept, nbytes, blocks, _ = decide(lib, planes, budget, B, from_bytes=from_bytes)
        assert (on, kept, nbytes) == (False, 0, 0), (budget, from_bytes)
        assert np.array_equal(blocks, unmarked_blocks(planes)), (budget, from_bytes)
    # 96 x 512x768 (luma 6144 rows, chroma 1536; 189 MB a pass) fit a budget of 230 x 10^6 bytes, 128 such images (252 MB) do
    # not: all 256 chroma planes (100.7 MB) are kept
    for nimg, want in ((96, (False, 0, 0)), (128, (True, 256, 256 * 1536 * 256))):
        pl = image_planes(nimg=nimg, ml=6144, mc=1536)
        assert decide(lib, pl, 230_000_000, nimg, persist=-1)[:3] == want, nimg


def test_first_plane_that_does_not_fit_ends_the_kept_run(lib):
    # a mixed table: 900 luma planes (2 blocks each), then chroma planes of 100, 500 and 100 rows; a budget for 250 rows keeps
    # the first and streams the other two: "in table order, until the budget is reached"
    planes = [(ML, 7)] * 900 + [(100, 3), (500, 3), (100, 3)]  # (98.8 MB of luma bytes: the call does not fit)
    on, kept, nbytes, blocks, _ = decide(lib, planes, 250 * 256, 900)
    assert (on, kept, nbytes) == (True, 1, 100 * 256)
    assert np.array_equal(blocks, expect_marks(planes, {900}))
    assert blocks.shape[0] == 1800 + 1 + 2 + 1


def test_calls_the_policy_does_not_apply_to(lib):
    planes = image_planes()
    everything = SOURCES_BYTES - 1  # all chroma planes; the call as a whole does not fit
    assert decide(lib, planes, everything, B)[:2] == (True, 512)
    # under a pipe: two contexts' kernels share the cache
    on, kept, nbytes, blocks, _ = decide(lib, planes, everything, B, piped=1)
    assert (on, kept, nbytes) == (False, 0, 0) and np.array_equal(blocks, unmarked_blocks(planes))
    # ranks above 8 anywhere in the call: other bodies of k_bcd_p, which have no such loads
    for ranks in [(9, 3, 3), (8, 9, 9), (16, 8, 8), (20, 10, 10)]:
        pr = image_planes(ranks=ranks)
        on, kept, nbytes, blocks, _ = decide(lib, pr, everything, B)
        assert (on, kept, nbytes) == (False, 0, 0) and np.array_equal(blocks, unmarked_blocks(pr)), ranks
    # calls that do not run on the persistent kernel: switched off, 1020 blocks, a single iteration
    for kw in ({"persist": 0}, {"K": 1}):
        on, kept, nbytes, blocks, _ = decide(lib, planes, everything, B, **kw)
        assert (on, kept, nbytes) == (False, 0, 0) and np.array_equal(blocks, unmarked_blocks(planes)), kw
    small = image_planes(nimg=255)
    on, kept, nbytes, blocks, _ = decide(lib, small, everything, 255)
    assert (on, kept, nbytes) == (False, 0, 0) and np.array_equal(blocks, unmarked_blocks(small))
    # the other rank triples of the rank <= 8 body take it
    for ranks in [(1, 1, 1), (4, 2, 2), (8, 8, 8)]:
        assert decide(lib, image_planes(ranks=ranks), everything, B)[:2] == (True, 512), ranks


def test_the_environment_sets_the_budget_in_megabytes(lib):
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); l.lrf_test_env_x_keep_bytes.restype = ctypes.c_long; "
            "print(l.lrf_test_env_x_keep_bytes())")
    for mb, want in (("0", 0), ("12", 12_000_000), ("1000", 1_000_000_000)):
        out = subprocess.check_output([sys.executable, "-c", code, _SO[0]], env=dict(os.environ, LRF_X_KEEP_MB=mb), text=True)
        assert int(out) == want, (mb, out)
