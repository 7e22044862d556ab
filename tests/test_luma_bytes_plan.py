"""CPU suite: luma from the image bytes (k_bcd_p's rank <= 8 body, lrf_amd/csrc/lrf_bcdp_kernel.hip) — the row -> patch mapping
the kernel and this test share (luma_byte_off, lrf_plan.h) and the decision which calls take the path (plan_luma_bytes,
lrf_plan.cpp).  Both need no device: built here with g++ together with tests/luma_bytes_shim.cpp and called through ctypes.

Expected values never come from the code under test: the luma matrix is the CPU oracle's (rgb_to_planes), the decision is
worked out by hand from the rules of the entry point — k_planes16's geometry, every iteration inside k_bcd_p<false, 0, true>,
the bytes still the caller's, the switch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
FIRST_W0, FIRST_U0 = 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("luma_bytes_plan") / "libluma_bytes_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "luma_bytes_shim.cpp")])
    return ctypes.CDLL(so)


@pytest.mark.parametrize("H, W", [(48, 80), (32, 1040)])
def test_mapping_reproduces_the_oracle_luma_matrix(lib, oracle, H, W):
    rng = np.random.default_rng(1000 * H + W)
    img = rng.integers(0, 256, size=(3, H, W), dtype=np.uint8)
    M = (H // 8) * (W // 8)
    off = np.empty((3, M, 64), dtype=np.int32)
    lib.lrf_test_luma_offsets(H, W, off.ctypes.data_as(ctypes.c_void_p))
    # every byte of a channel exactly once, inside that channel
    for ch in range(3):
        assert np.array_equal(np.sort(off[ch].reshape(-1)), ch * H * W + np.arange(H * W)), ch
    # element (m, n) is pixel (n >> 3, n & 7) of patch (m / nwl, m % nwl)
    m, n = np.meshgrid(np.arange(M), np.arange(64), indexing="ij")
    y, x = 8 * (m // (W // 8)) + (n >> 3), 8 * (m % (W // 8)) + (n & 7)
    assert np.array_equal(off[1], H * W + y * W + x)
    got = np.empty((M, 64), dtype=np.float32)
    flat = np.ascontiguousarray(img).reshape(-1)
    lib.lrf_test_luma_from_bytes(flat.ctypes.data_as(ctypes.c_void_p), H, W, got.ctypes.data_as(ctypes.c_void_p))
    want = np.ascontiguousarray(oracle.rgb_to_planes(img)[0], dtype=np.float32)
    assert want.shape == (M, 64)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def image_planes(B, H, W, ranks):
    """the table of the fused encode (encode_rgb_prepare): all Y planes, then Cb, then Cr"""
    def M(c):
        h, w = (H // 2, W // 2) if c else (H, W)
        return ((h + 7) // 8) * ((w + 7) // 8)
    return [(M(c), ranks[c]) for c in range(3) for _ in range(B)]


def decide(lib, B, H, W, ranks=(7, 3, 3), K=10, first_mode=FIRST_W0, persist=1, addr=0x7000_0000_1000, released=0, setting=-1):
    planes = image_planes(B, H, W, ranks)
    n = len(planes)
    M = (ctypes.c_int * n)(*[p[0] for p in planes])
    R = (ctypes.c_int * n)(*[p[1] for p in planes])
    lib.lrf_test_plan_luma_bytes.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_long, ctypes.c_long,
                                                                                                                      ctypes.c_ulong, ctypes.c_int, ctypes.c_int]
    return bool(lib.lrf_test_plan_luma_bytes(n, M, R, K, first_mode, persist, B, H, W, addr, released, setting))


def test_which_calls_take_the_path(lib):
    # 48x80: three blocks an image, so 342 images make the 1024 blocks LRF_PERSIST=1 asks for; 256 x 512x768: 6144 blocks, the
    # persistent launch by default (from 2304 blocks of one family)
    assert decide(lib, 342, 48, 80)
    assert decide(lib, 256, 512, 768, persist=-1)
    assert decide(lib, 342, 48, 80, setting=1) and not decide(lib, 342, 48, 80, setting=0)
    for ranks in [(1, 1, 1), (4, 4, 4), (5, 4, 1), (8, 8, 8)]:
        assert decide(lib, 342, 48, 80, ranks=ranks), ranks
    # geometry: sides multiples of 16 (173x264: 8 blocks an image), the bytes 8-byte aligned, 3 H W < 2^31
    assert not decide(lib, 272, 173, 264)
    assert not decide(lib, 342, 56, 80) and not decide(lib, 342, 48, 88)
    for a in range(1, 8):
        assert not decide(lib, 342, 48, 80, addr=0x7000_0000_1000 + a), a
    assert 3 * 26768 * 26768 >= 2 ** 31 and 26768 % 16 == 0 and not decide(lib, 1, 26768, 26768)
    assert 3 * 26752 * 26752 < 2 ** 31 and decide(lib, 1, 26752, 26752)
    # the plan: every iteration inside k_bcd_p<false, 0, true>
    assert not decide(lib, 341, 48, 80)                      # 1023 blocks: launch per iteration
    assert not decide(lib, 342, 48, 80, persist=0)
    assert not decide(lib, 64, 512, 768, persist=-1)         # 1536 blocks: below the default threshold
    assert not decide(lib, 342, 48, 80, K=1)                 # a single iteration stays on its launch
    assert not decide(lib, 342, 48, 80, first_mode=FIRST_U0)  # the first iteration outside the persistent launch
    assert not decide(lib, 342, 48, 80, ranks=(9, 3, 3))     # luma above rank 8
    assert not decide(lib, 342, 48, 80, ranks=(8, 9, 9))     # chroma on the rank 9..16 body: another instantiation
    # the bytes are handed back behind the planes kernel (a pipe)
    assert not decide(lib, 342, 48, 80, released=1)
