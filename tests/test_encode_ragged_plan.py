"""CPU suite: the tables of a ragged encode (plan_encode_ragged, lrf_amd/csrc/lrf_plan.cpp).  The plan source needs no device: it
is built here with g++ together with tests/encode_ragged_plan_shim.cpp and called through ctypes.

What is expected is worked out below from the rules alone — never by the library:
  * geometry (lrf/compression/qmf.py:230-242): luma H x W, chroma floor(H/2) x floor(W/2), each reflect-padded to multiples of 8;
    M = patches of 8 x 8; X holds the three matrices of an image back to back, the images back to back
  * body: sides multiples of 16 and bytes at a multiple of 8 -> the 16-aligned body, one workgroup per (16-row strip, 32 luma
    patches); otherwise the strip body with pooling windows (KH, KW) = 2 or 3 by the parity of H and of W, one workgroup per
    (16 padded luma rows = 8 padded chroma rows, 32 luma patches' width)
  * launches: the 16-aligned images in one, the others one per (KH, KW) present; inside a launch images in call order, units ascending
  * plane table: by kernel family (rank <= 8, <= 16, <= 32) when the call splits, luma before Cb before Cr inside a family,
    images in call order; one block per 384 rows of a plane"""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
TILE16, S22, S23, S32, S33 = range(5)
SIZES = [(32, 272), (40, 272), (45, 61), (64, 96), (24, 48), (173, 264)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("encode_ragged_plan") / "libencode_ragged_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "encode_ragged_plan_shim.cpp")])
    return ctypes.CDLL(so)


def geom(H, W):
    """[(M, nh, nw)] of Y, Cb, Cr"""
    out = []
    for h, w in ((H, W), (H // 2, W // 2), (H // 2, W // 2)):
        nh, nw = -(-h // 8), -(-w // 8)
        out.append((nh * nw, nh, nw))
    return out


def classify(H, W, aligned8=True):
    """(body, per_strip, units) of an image"""
    (_, nhl, nwl), (_, nhc, nwc), _ = geom(H, W)
    if H % 16 == 0 and W % 16 == 0 and aligned8:
        per = (nwl + 31) // 32
        return TILE16, per, (H // 16) * per
    per = (max(nwl, 2 * nwc) + 31) // 32
    return S22 + 2 * (H & 1) + (W & 1), per, max((nhl + 1) // 2, nhc) * per


def make(items, rgb_offs=None, with_sign=None):
    """items: (H, W, ranks) -> the images as the entry point would hand them over: pixels 16-aligned back to back, factors back to back"""
    ims, ro, uo, vo, so = [], 0, 0, 0, 0
    for i, (H, W, R) in enumerate(items):
        sign = with_sign is not None and with_sign[i]
        r_off = ro if rgb_offs is None else rgb_offs[i]
        ims.append(dict(H=H, W=W, R=R, rgb_off=r_off, u_off=uo, v_off=vo, sign_off=so if sign else -1, aligned8=r_off % 8 == 0))
        ro = (ro + 3 * H * W + 15) // 16 * 16
        uo += sum(g[0] * r for g, r in zip(geom(H, W), R))
        vo += 64 * sum(R)
        so += sum(R) if sign else 0
    return ims


def plan(lib, ims, split_blocks=-1, cap=None):
    n = len(ims)
    cap = sum(classify(im["H"], im["W"], im["aligned8"])[2] for im in ims) + 16 if cap is None else cap
    L = ctypes.c_long
    launches, blocks = (L * (4 * 8))(), (ctypes.c_int * (2 * cap))()
    descs, planes, out = (L * (6 * n))(), (L * (10 * 3 * n))(), (L * 5)()
    arr = lambda key: (L * n)(*[im[key] for im in ims])
    nl = lib.lrf_test_plan_encode_ragged(n, arr("H"), arr("W"), (ctypes.c_int * (3 * n))(*[r for im in ims for r in im["R"]]), arr("rgb_off"),
                                         arr("u_off"), arr("v_off"), arr("sign_off"), (ctypes.c_int * n)(*[int(im["aligned8"]) for im in ims]),
                                         L(split_blocks), launches, 8, blocks, L(cap), descs, planes, out)
    assert nl >= 0, nl
    res = dict(zip(("nblocks", "bcd_blocks", "split", "x_floats", "too_many"), out))
    res["launches"] = [dict(zip(("body", "block0", "nblocks", "xcd_chunk"), launches[4 * j:4 * j + 4])) for j in range(nl)]
    if res["too_many"]:
        return res
    res["blocks"] = [(blocks[2 * j], blocks[2 * j + 1]) for j in range(res["nblocks"])]
    res["descs"] = [dict(zip(("body", "per_strip", "x_off", "rgb_off", "H", "W"), descs[6 * j:6 * j + 6])) for j in range(n)]
    keys = ("image", "ch", "x_off", "u_off", "v_off", "M", "R", "sign_off", "blk0", "nblk")
    res["planes"] = [dict(zip(keys, planes[10 * j:10 * j + 10])) for j in range(3 * n)]
    return res


def check(lib, ims, split_blocks=-1, expect_split=None):
    """the properties every plan must have; -> the plan"""
    p = plan(lib, ims, split_blocks)
    n = len(ims)
    assert p["too_many"] == 0
    cls = [classify(im["H"], im["W"], im["aligned8"]) for im in ims]
    # descriptors: body, per_strip, the X workspace as a running sum
    x = 0
    for im, d, (body, per, _) in zip(ims, p["descs"], cls):
        assert (d["body"], d["per_strip"], d["x_off"], d["rgb_off"], d["H"], d["W"]) == (body, per, x, im["rgb_off"], im["H"], im["W"])
        x += 64 * sum(g[0] for g in geom(im["H"], im["W"]))
    assert p["x_floats"] == x
    # launches: at most five, by body, tiling the workgroup table; images in call order, units ascending, each exactly once
    bodies = sorted({c[0] for c in cls})
    assert [l["body"] for l in p["launches"]] == bodies and len(bodies) <= 5
    at = 0
    for l in p["launches"]:
        mine = [i for i in range(n) if cls[i][0] == l["body"]]
        want = [(i, u) for i in mine for u in range(cls[i][2])]
        assert l["block0"] == at and p["blocks"][at:at + l["nblocks"]] == want
        assert l["xcd_chunk"] == (0 if l["body"] == TILE16 else -(-len(want) // 8))
        at += l["nblocks"]
    assert at == p["nblocks"] == len(p["blocks"])
    # the plane table
    rmax = max(max(im["R"]) for im in ims)
    nblk = lambda i, ch: -(-geom(ims[i]["H"], ims[i]["W"])[ch][0] // 384)
    total = sum(nblk(i, ch) for i in range(n) for ch in range(3))
    assert p["bcd_blocks"] == total
    split = total >= (split_blocks if split_blocks >= 0 else (256 if rmax > 16 else 1024))
    assert bool(p["split"]) == split
    if expect_split is not None:
        assert split == expect_split
    fam = lambda r: 0 if r <= 8 else (1 if r <= 16 else 2)
    order = [(i, ch) for f in range(3 if split else 1) for ch in range(3) for i in range(n) if not split or fam(ims[i]["R"][ch]) == f]
    assert [(pl["image"], pl["ch"]) for pl in p["planes"]] == order and sorted(order) == [(i, ch) for i in range(n) for ch in range(3)]
    blk0 = 0
    xs = [d["x_off"] for d in p["descs"]]
    for pl, (i, ch) in zip(p["planes"], order):
        im, g = ims[i], geom(ims[i]["H"], ims[i]["W"])
        assert (pl["M"], pl["R"]) == (g[ch][0], im["R"][ch])
        assert pl["x_off"] == xs[i] + 64 * sum(g[c][0] for c in range(ch))
        assert pl["u_off"] == im["u_off"] + sum(g[c][0] * im["R"][c] for c in range(ch))
        assert pl["v_off"] == im["v_off"] + 64 * sum(im["R"][:ch])
        assert pl["sign_off"] == (-1 if im["sign_off"] < 0 else im["sign_off"] + sum(im["R"][:ch]))
        assert (pl["blk0"], pl["nblk"]) == (blk0, nblk(i, ch))
        blk0 += pl["nblk"]
    return p


def test_the_rules_give_the_bodies_the_sizes_are_meant_to_hit():
    assert classify(32, 272) == (TILE16, 2, 4) and classify(64, 96) == (TILE16, 1, 4)
    assert classify(40, 272) == (S22, 2, 6) and classify(24, 48) == (S22, 1, 2)
    assert classify(45, 61) == (S33, 1, 3) and classify(173, 264) == (S32, 2, 22)
    assert classify(64, 96, aligned8=False) == (S22, 1, 4)
    assert classify(46, 61)[0] == S23


def test_six_sizes_take_their_bodies_and_four_launches(lib):
    p = check(lib, make([(H, W, (7, 3, 3)) for H, W in SIZES]), expect_split=False)
    assert [d["body"] for d in p["descs"]] == [TILE16, S22, S33, TILE16, S22, S32]
    assert [(l["body"], l["nblocks"]) for l in p["launches"]] == [(TILE16, 8), (S22, 8), (S32, 22), (S33, 3)]
    assert p["blocks"][:8] == [(0, 0), (0, 1), (0, 2), (0, 3), (3, 0), (3, 1), (3, 2), (3, 3)]


def test_all_five_launches(lib):
    p = check(lib, make([(H, W, (7, 3, 3)) for H, W in SIZES + [(46, 61)]]))
    assert [l["body"] for l in p["launches"]] == [TILE16, S22, S23, S32, S33]


def test_an_aligned_image_at_an_odd_offset_goes_to_a_strip_launch(lib):
    items = [(64, 96, (7, 3, 3))] * 3
    ims = make(items, rgb_offs=[0, 3 * 64 * 96 + 3, 2 * 3 * 64 * 96 + 8])
    assert [im["aligned8"] for im in ims] == [True, False, True]
    p = check(lib, ims)
    assert [d["body"] for d in p["descs"]] == [TILE16, S22, TILE16]
    assert [(l["body"], l["nblocks"]) for l in p["launches"]] == [(TILE16, 8), (S22, 4)]


def test_planes_are_ordered_by_family_when_the_call_splits_luma_first(lib):
    triples = [(7, 3, 3), (12, 6, 6), (26, 13, 13), (16, 9, 16), (1, 1, 1), (32, 16, 16)]
    items = [(H, W, triples[(i + j) % 6]) for j in range(3) for i, (H, W) in enumerate(SIZES)]
    small = check(lib, make(items), expect_split=False)  # a small call: one run, channel-major
    assert [pl["ch"] for pl in small["planes"]] == [0] * 18 + [1] * 18 + [2] * 18
    p = check(lib, make(items, with_sign=[i % 2 == 0 for i in range(18)]), split_blocks=0, expect_split=True)
    fams = [0 if pl["R"] <= 8 else (1 if pl["R"] <= 16 else 2) for pl in p["planes"]]
    assert fams == sorted(fams) and set(fams) == {0, 1, 2}
    for f in range(3):
        chs = [pl["ch"] for pl, g in zip(p["planes"], fams) if g == f]
        assert chs == sorted(chs)
    # the default threshold: a call with a rank above 16 splits from 256 blocks, one without from 1024
    big = [(512, 768, (20, 10, 10))] * 26  # 16 + 4 + 4 blocks... per image: ceil(6144 / 384) + 2 ceil(1536 / 384) = 24
    assert check(lib, make(big), expect_split=True)["bcd_blocks"] == 624
    assert check(lib, make([(512, 768, (7, 3, 3))] * 26), expect_split=False)["bcd_blocks"] == 624
    assert check(lib, make([(512, 768, (7, 3, 3))] * 43), expect_split=True)["bcd_blocks"] == 1032


def test_offsets_follow_the_images_own_offsets(lib):
    ims = make([(45, 61, (8, 8, 5)), (24, 48, (16, 9, 16)), (64, 96, (1, 1, 1))], with_sign=[True, False, True])
    ims[0]["u_off"], ims[2]["u_off"] = ims[2]["u_off"], ims[0]["u_off"]  # factors need not stand in call order
    ims[1]["v_off"] += 1000
    p = check(lib, ims)
    assert [pl["sign_off"] for pl in p["planes"] if pl["image"] == 1] == [-1, -1, -1]
    assert [pl["sign_off"] for pl in p["planes"] if pl["image"] == 2] == [21, 22, 23]


def test_one_image(lib):
    for H, W in SIZES:
        p = check(lib, make([(H, W, (12, 6, 6))]))
        assert len(p["launches"]) == 1 and len(p["planes"]) == 3


def test_a_total_of_2_to_the_31_blocks_is_refused(lib):
    """65535 images of 26000 x 26000 (3 H W < 2^31 each): 27507 + 2 x 6877 = 41261 blocks per image, 2.7e9 in all"""
    per = sum(-(-g[0] // 384) for g in geom(26000, 26000))
    assert per == 41261 and 65535 * per >= 2 ** 31 and 3 * 26000 * 26000 < 2 ** 31
    im = dict(H=26000, W=26000, R=(7, 3, 3), rgb_off=0, u_off=0, v_off=0, sign_off=-1, aligned8=True)
    p = plan(lib, [im] * 65535, cap=16)
    # (reported: the larger of the BCD block count and the planes stage's workgroup count, 1625 strips x 102 column groups per image)
    assert p["too_many"] == 65535 * max(per, classify(26000, 26000)[2]) >= 2 ** 31 and p["launches"] == [] and p["nblocks"] == 0 and p["bcd_blocks"] == 0 and p["x_floats"] == 0
    assert check(lib, [im])["too_many"] == 0
