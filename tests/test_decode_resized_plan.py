"""CPU suite: the level, the taps, the tile footprints, the thread maps and the launch plan of the resized crops (lrf_plan.h,
plan_decode_resized in lrf_amd/csrc/lrf_plan.cpp; the kernels of lrf_decode_resized_kernel.hip call the same functions).  Built
here with g++ together with tests/decode_resized_plan_shim.cpp and called through ctypes: no device.

  * resized_level and resized_tap equal the numpy definition (resized_decode.py) for every output row of a grid of output
    sizes, box lengths, level sizes and origins;
  * the threads of both paths write every output pixel exactly once, flipped or not;
  * the footprint of a tile contains every tap of the tile, and fits the LDS tile whenever the path rule says staged;
  * the boxes are grouped by (path, level, rank class) in that order, call order kept inside a launch, every box in exactly
    one launch with its place in the call; at most 16 launches; 2^31 workgroups are refused."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from resized_decode import resized_level, taps

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
MAX_LAUNCHES = 16  # 2 paths x 4 levels x 2 rank classes


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("resized_plan") / "libresized_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "decode_resized_plan_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_resized_tap.restype = None
    lib.lrf_test_resized_tap.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
    lib.lrf_test_resized_span_bound.restype = ctypes.c_long
    lib.lrf_test_resized_wgs.restype = ctypes.c_long
    lib.lrf_test_resized_tile_dims.restype = None
    lib.lrf_test_resized_tile_dims.argtypes = [ctypes.c_void_p]
    lib.lrf_test_resized_cover.restype = ctypes.c_long
    lib.lrf_test_resized_cover.argtypes = [ctypes.c_int] * 4 + [ctypes.c_long, ctypes.c_void_p]
    lib.lrf_test_resized_footprint.restype = ctypes.c_long
    lib.lrf_test_resized_footprint.argtypes = [ctypes.c_int] * 8 + [ctypes.c_void_p] * 2
    lib.lrf_test_plan_decode_resized.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_level_is_the_definition(lib):
    for oh, ow in ((1, 1), (5, 7), (16, 16), (224, 224)):
        for hb in (1, oh - 1, oh, 2 * oh - 1, 2 * oh, 4 * oh - 1, 4 * oh, 8 * oh - 1, 8 * oh, 16 * oh + 3):
            for wb in (1, ow, 2 * ow - 1, 2 * ow, 4 * ow, 8 * ow - 1, 8 * ow, 100 * ow):
                if hb >= 1:
                    assert lib.lrf_test_resized_level(hb, wb, oh, ow) == resized_level(hb, wb, oh, ow), (hb, wb, oh, ow)


@pytest.mark.parametrize("n_out", [1, 5, 17, 224])
def test_taps_are_the_definition_for_every_output_row(lib, n_out):
    out = np.zeros(3, np.int32)
    checked = 0
    for nb in sorted({1, n_out - 1, n_out, 2 * n_out - 1, 2 * n_out, 16 * n_out + 3} - {0}):
        for n_lvl in (9, 45, 173, 1365):
            for f in (1, 2, 4, 8):
                if f > 1 and f * n_out > nb:
                    continue  # (a level the box is too small for on this axis)
                n_img = n_lvl * f  # an image side with ceil(n_img / f) = n_lvl
                if nb > n_img:
                    continue
                for b0 in sorted({0, n_img - nb}):
                    i0, i1, t = taps(n_out, b0, nb, f, n_lvl)
                    for r in range(n_out):
                        lib.lrf_test_resized_tap(r, n_out, b0, nb, f, n_lvl, out.ctypes.data)
                        assert out.tolist() == [int(i0[r]), int(i1[r]), int(t[r])], (r, n_out, b0, nb, f, n_lvl)
                    assert 0 <= i0.min() and i1.max() <= n_lvl - 1 and (np.diff(i0) >= 0).all()
                    checked += 1
    assert checked >= 8


def test_taps_floor_towards_minus_infinity(lib):
    # a 1-pixel box up-sampled to 5: N = 2 r + 1 - 5 is negative for r < 2, and 256 N / D is no integer: floor, then the clamp to 0
    out = np.zeros(3, np.int32)
    for r in range(5):
        lib.lrf_test_resized_tap(r, 5, 3, 1, 1, 9, out.ctypes.data)
        q = max(0, min((256 * ((2 * r + 1) + 2 * 5 * 3 - 5)) // 10, 256 * 8))
        assert out.tolist() == [q >> 8, min((q >> 8) + 1, 8), q & 255]
    # unclamped negative values: truncation would give one more than the floor
    i0, i1, t = taps(5, 0, 1, 1, 9)
    assert i0.tolist() == [0] * 5 and t.tolist() == [0, 0, 0, 51, 102]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("oh,ow", [(1, 1), (5, 7), (16, 16), (17, 33), (16, 64), (33, 130), (224, 224)])
def test_the_threads_write_every_output_pixel_once(lib, oh, ow, flip):
    for direct in (0, 1):
        count = np.zeros((oh, ow), dtype=np.int32)
        wgs = lib.lrf_test_resized_wgs(direct, oh, ow)
        assert lib.lrf_test_resized_cover(direct, oh, ow, flip, wgs, count.ctypes.data) == 0
        assert count.min() == 1 and count.max() == 1
    dims = np.zeros(4, np.int32)
    lib.lrf_test_resized_tile_dims(dims.ctypes.data)
    th, tw = int(dims[2]), int(dims[3])
    assert lib.lrf_test_resized_wgs(0, oh, ow) == -(-oh // th) * -(-ow // tw) and lib.lrf_test_resized_wgs(1, oh, ow) == -(-oh * ow // 256)


def test_a_tile_footprint_holds_every_tap_and_fits_where_the_rule_says_staged(lib):
    dims = np.zeros(4, np.int32)
    lib.lrf_test_resized_tile_dims(dims.ctypes.data)
    FH, FW = int(dims[0]), int(dims[1])
    rng = np.random.default_rng(11)
    mh, mw = ctypes.c_int(), ctypes.c_int()
    staged = direct = 0
    cases = [(64, 96, 0, 0, 64, 96), (173, 264, 165, 0, 8, 264), (45, 61, 44, 60, 1, 1), (1365, 2048, 0, 0, 1365, 2048), (512, 768, 0, 0, 512, 768)]
    for _ in range(300):
        H, W = int(rng.integers(9, 600)), int(rng.integers(9, 600))
        hb, wb = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        cases.append((H, W, int(rng.integers(0, H - hb + 1)), int(rng.integers(0, W - wb + 1)), hb, wb))
    for H, W, y0, x0, hb, wb in cases:
        for oh, ow in ((5, 7), (16, 16), (17, 33), (224, 224)):
            f = resized_level(hb, wb, oh, ow)
            assert lib.lrf_test_resized_footprint(H, W, y0, x0, hb, wb, oh, ow, ctypes.byref(mh), ctypes.byref(mw)) == 0, (H, W, y0, x0, hb, wb, oh, ow)
            # the bound the rule is built on holds for every tile
            assert mh.value <= lib.lrf_test_resized_span_bound(int(dims[2]), oh, hb, f) and mw.value <= lib.lrf_test_resized_span_bound(int(dims[3]), ow, wb, f)
            if lib.lrf_test_resized_staged(hb, wb, oh, ow, f):
                assert mh.value <= FH and mw.value <= FW, (H, W, y0, x0, hb, wb, oh, ow)
                staged += 1
            else:
                direct += 1
    assert staged > 100 and direct > 100


def test_the_path_rule(lib):
    # 8x264 to 17x33: level 1, 33 output columns read 264 level columns, more than the LDS tile holds
    assert resized_level(8, 264, 17, 33) == 1 and not lib.lrf_test_resized_staged(8, 264, 17, 33, 1)
    # 64x96 to 16x16: level 4, a 16x24 footprint
    assert resized_level(64, 96, 16, 16) == 4 and lib.lrf_test_resized_staged(64, 96, 16, 16, 4)
    # what RandomResizedCrop(224) draws from 512x768 (area 8 % .. 100 %, aspect 3/4 .. 4/3) is staged
    for hb, wb in ((512, 768), (512, 683), (153, 205), (205, 153), (224, 224), (480, 360)):
        assert lib.lrf_test_resized_staged(hb, wb, 224, 224, resized_level(hb, wb, 224, 224))
    # its worst case: the longer side 4/3 of the shorter, the shorter one pixel short of the next level (2.67 level pixels per output)
    for f in (1, 2, 4):
        short = 2 * f * 224 - 1
        for hb, wb in ((short * 4 // 3, short), (short, short * 4 // 3)):
            assert resized_level(hb, wb, 224, 224) == f and lib.lrf_test_resized_staged(hb, wb, 224, 224, f)
    # a box beyond 16 times the output on both axes stays at level 8 and leaves the staged path once its footprint outgrows the tile
    assert resized_level(400, 400, 16, 16) == 8 and not lib.lrf_test_resized_staged(400, 400, 16, 16, 8)


def plan(lib, r8, crops, size):
    im = np.ascontiguousarray(r8, dtype=np.int32)
    cr = np.ascontiguousarray(crops, dtype=np.int32).reshape(-1, 6)
    launches = np.zeros((MAX_LAUNCHES, 6), dtype=np.int64)
    table = np.full((len(cr), 8), -7, dtype=np.int64)
    too_many = ctypes.c_long()
    nl = lib.lrf_test_plan_decode_resized(len(im), im.ctypes.data, len(cr), cr.ctypes.data, size[0], size[1], launches.ctypes.data, MAX_LAUNCHES,
                                          table.ctypes.data, ctypes.byref(too_many))
    assert nl >= 0  # never more than MAX_LAUNCHES
    L = [dict(zip(("direct", "f", "r8", "item0", "nitems", "wgs"), (int(v) for v in launches[j]))) for j in range(nl)]
    return L, table, too_many.value


def check_plan(lib, r8, crops, size):
    L, table, too_many = plan(lib, r8, crops, size)
    assert too_many == 0 and 1 <= len(L) <= MAX_LAUNCHES
    want = {}
    for j, (i, y0, x0, hb, wb, flip) in enumerate(crops):
        f = resized_level(hb, wb, *size)
        key = (0 if lib.lrf_test_resized_staged(hb, wb, size[0], size[1], f) else 1, f, 0 if r8[i] else 1)
        want.setdefault(key, []).append((i, f, y0, x0, hb, wb, int(flip != 0), j))
    keys = [(l["direct"], l["f"], 0 if l["r8"] else 1) for l in L]
    assert keys == sorted(want)  # one launch per group present, in the documented order
    at = 0
    for l, key in zip(L, keys):
        rows = [tuple(int(v) for v in row) for row in table[at:at + l["nitems"]]]
        assert l["item0"] == at and rows == want[key]  # call order inside the launch, the place in the call carried
        assert l["wgs"] == lib.lrf_test_resized_wgs(key[0], *size) and l["nitems"] * l["wgs"] < 2 ** 31
        at += l["nitems"]
    assert at == len(crops) and sorted(int(v) for v in table[:, 7]) == list(range(len(crops)))  # every box once
    return L


def test_grouping_places_and_launch_order(lib):
    rng = np.random.default_rng(3)
    r8 = [1, 0, 1, 0, 1]
    crops = []
    for _ in range(400):
        hb, wb = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        crops.append((int(rng.integers(0, 5)), int(rng.integers(0, 9)), int(rng.integers(0, 9)), hb, wb, int(rng.integers(0, 3))))
    L = check_plan(lib, r8, crops, (16, 16))
    assert len({(l["direct"], l["f"], l["r8"]) for l in L}) == len(L) >= 10
    check_plan(lib, r8, crops, (5, 7))
    check_plan(lib, [1], [(0, 0, 0, 16, 16, 0)], (16, 16))
    check_plan(lib, [1, 0], [(0, 3, 4, 20, 30, 1), (1, 0, 0, 2, 2, 0), (0, 3, 4, 20, 30, 1)], (5, 7))  # a box listed twice


def test_at_most_sixteen_launches(lib):
    # every (path, level, rank class): staged boxes of f x the output, direct boxes 40 times as wide as their level needs
    crops = [(i, 0, 0, f * 16, f * 16, 0) for f in (1, 2, 4, 8) for i in (0, 1)] + [(i, 0, 0, f * 16, f * 16 * 40, 0) for f in (1, 2, 4, 8) for i in (0, 1)]
    L = check_plan(lib, [1, 0], crops * 2, (16, 16))
    assert len(L) == MAX_LAUNCHES


def test_a_launch_of_2_to_the_31_workgroups_is_refused(lib):
    # 16384x16384 outputs: 2^18 tiles a box on the staged path, 2^20 workgroups a box on the direct path
    assert lib.lrf_test_resized_wgs(0, 16384, 16384) == 2 ** 18 and lib.lrf_test_resized_wgs(1, 16384, 16384) == 2 ** 20
    L, table, too_many = plan(lib, [1], [(0, 0, 0, 1, 1, 0)] * 8192, (16384, 16384))
    assert too_many == 2 ** 31 and L == []
    L, table, too_many = plan(lib, [1], [(0, 0, 0, 1, 1, 0)] * 8191, (16384, 16384))
    assert too_many == 0 and len(L) == 1 and L[0]["nitems"] * L[0]["wgs"] == 2 ** 31 - 2 ** 18
    wide = (0, 0, 0, 1, 2 ** 17, 0)  # level 1, 8 level columns per output column: direct
    assert not lib.lrf_test_resized_staged(1, 2 ** 17, 16384, 16384, 1)
    L, table, too_many = plan(lib, [1], [wide] * 2048, (16384, 16384))
    assert too_many == 2 ** 31 and L == []
    L, table, too_many = plan(lib, [1], [wide] * 2047, (16384, 16384))
    assert too_many == 0 and len(L) == 1 and L[0]["direct"] == 1
