"""CPU suite: the tables of a ragged sweep encode (plan_encode_ragged_sweep, lrf_amd/csrc/lrf_plan.cpp).  The plan source needs no
device: it is built here with g++ together with tests/ragged_sweep_plan_shim.cpp and called through ctypes.

What is expected is worked out below from the rules alone — never by the library:
  * geometry (lrf/compression/qmf.py:230-242): luma H x W, chroma floor(H/2) x floor(W/2), each reflect-padded to multiples of 8;
    M = patches of 8 x 8; X holds the three matrices of an IMAGE back to back, the images back to back — once per image, however
    many candidates it has
  * one plane per (candidate, channel), one block per 384 rows; its factors start at the candidate's offsets plus the planes
    before it at the candidate's ranks; its signs at the image's offset plus the image's LARGEST ranks of the channels before it
  * init_src: the plane of the same image and channel whose candidate has the image's largest rank there, the first of equals
  * order: by kernel family (rank <= 8, <= 16, <= 32) when the call splits, inside a family the self-initialising planes first,
    then luma before Cb before Cr, candidates in list order"""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
L = ctypes.c_long


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ragged_sweep_plan") / "libragged_sweep_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "ragged_sweep_plan_shim.cpp")])
    return ctypes.CDLL(so)


def geom(H, W):
    """[M] of Y, Cb, Cr"""
    return [-(-h // 8) * -(-w // 8) for h, w in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]


def fam(r):
    return 0 if r <= 8 else (1 if r <= 16 else 2)


def make(sizes, cand_lists, with_sign=None, interleave=True):
    """sizes: (H, W) per image; cand_lists: per image its rank triples -> (images, candidates) as the entry point would hand them
    over: pixels 16-aligned back to back, the candidates of the images interleaved round-robin, factors back to back in list order,
    signs (where asked for) back to back at the image's largest ranks"""
    rmax = [[max(t[ch] for t in ts) for ch in range(3)] for ts in cand_lists]
    ims, ro, so = [], 0, 0
    for i, (H, W) in enumerate(sizes):
        sign = with_sign is not None and with_sign[i]
        ims.append(dict(H=H, W=W, rgb_off=ro, sign_off=so if sign else -1, aligned8=ro % 8 == 0))
        ro = (ro + 3 * H * W + 15) // 16 * 16
        so += sum(rmax[i]) if sign else 0
    if interleave:
        order = [(i, k) for k in range(max(len(ts) for ts in cand_lists)) for i in range(len(sizes)) if k < len(cand_lists[i])]
    else:
        order = [(i, k) for i in range(len(sizes)) for k in range(len(cand_lists[i]))]
    cands, uo, vo = [], 0, 0
    for i, k in order:
        R = cand_lists[i][k]
        cands.append(dict(image=i, R=R, u_off=uo, v_off=vo))
        uo += sum(m * r for m, r in zip(geom(*sizes[i]), R))
        vo += 64 * sum(R)
    return ims, cands


def plan(lib, ims, cands, split_blocks=-1):
    n, m = len(ims), len(cands)
    planes, x_offs, runs, out = (L * (11 * 3 * m))(), (L * n)(), (L * (4 * 8))(), (L * 7)()
    arr = lambda xs, key: (L * len(xs))(*[x[key] for x in xs])
    rc = lib.lrf_test_plan_ragged_sweep(n, arr(ims, "H"), arr(ims, "W"), arr(ims, "rgb_off"), arr(ims, "sign_off"),
                                        (ctypes.c_int * n)(*[int(im["aligned8"]) for im in ims]), m, (ctypes.c_int * m)(*[c["image"] for c in cands]),
                                        (ctypes.c_int * (3 * m))(*[r for c in cands for r in c["R"]]), arr(cands, "u_off"), arr(cands, "v_off"),
                                        L(split_blocks), planes, x_offs, runs, 8, out)
    assert rc == 0, rc
    res = dict(zip(("nblocks", "bcd_blocks", "split", "x_floats", "too_many", "launches", "nruns"), out))
    if res["too_many"]:
        return res
    keys = ("cand", "ch", "x_off", "u_off", "v_off", "M", "R", "sign_off", "blk0", "nblk", "init_src")
    res["planes"] = [dict(zip(keys, planes[11 * j:11 * j + 11])) for j in range(3 * m)]
    res["x_offs"] = list(x_offs)
    res["runs"] = [dict(zip(("plane0", "nplanes", "nbase", "fam"), runs[4 * r:4 * r + 4])) for r in range(res["nruns"])]
    return res


def check(lib, ims, cands, split_blocks=-1, expect_split=None):
    """the properties every plan must have; -> the plan"""
    p = plan(lib, ims, cands, split_blocks)
    n, m = len(ims), len(cands)
    assert p["too_many"] == 0
    g = [geom(im["H"], im["W"]) for im in ims]
    # X: once per image
    xs, x = [], 0
    for i in range(n):
        xs.append(x)
        x += 64 * sum(g[i])
    assert p["x_floats"] == x and p["x_offs"] == xs
    rmax = [[max(c["R"][ch] for c in cands if c["image"] == i) for ch in range(3)] for i in range(n)]
    base = {(i, ch): min(j for j, c in enumerate(cands) if c["image"] == i and c["R"][ch] == rmax[i][ch]) for i in range(n) for ch in range(3)}
    total = sum(-(-g[c["image"]][ch] // 384) for c in cands for ch in range(3))
    assert p["bcd_blocks"] == total
    rmax_t = max(max(c["R"]) for c in cands)
    split = total >= (split_blocks if split_blocks >= 0 else (256 if rmax_t > 16 else 1024))
    assert bool(p["split"]) == split
    if expect_split is not None:
        assert split == expect_split
    # every (candidate, channel) exactly once, in the documented order
    order = [(j, ch) for f in range(3 if split else 1) for self_init in (True, False) for ch in range(3) for j, c in enumerate(cands)
             if (not split or fam(c["R"][ch]) == f) and ((base[(c["image"], ch)] == j) == self_init)]
    assert [(pl["cand"], pl["ch"]) for pl in p["planes"]] == order
    assert sorted(order) == [(j, ch) for j in range(m) for ch in range(3)]
    where = {jc: k for k, jc in enumerate(order)}
    blk0 = 0
    for k, (pl, (j, ch)) in enumerate(zip(p["planes"], order)):
        c = cands[j]
        i = c["image"]
        assert (pl["M"], pl["R"]) == (g[i][ch], c["R"][ch])
        assert pl["x_off"] == xs[i] + 64 * sum(g[i][:ch])
        assert pl["u_off"] == c["u_off"] + sum(g[i][c2] * c["R"][c2] for c2 in range(ch))
        assert pl["v_off"] == c["v_off"] + 64 * sum(c["R"][:ch])
        assert pl["sign_off"] == (-1 if ims[i]["sign_off"] < 0 else ims[i]["sign_off"] + sum(rmax[i][:ch]))
        assert (pl["blk0"], pl["nblk"]) == (blk0, -(-g[i][ch] // 384))
        blk0 += pl["nblk"]
        # the initialising plane: same image, same channel, the image's largest rank, the first of equals
        assert pl["init_src"] == where[(base[(i, ch)], ch)]
        src = p["planes"][pl["init_src"]]
        assert cands[src["cand"]]["image"] == i and src["ch"] == ch and src["R"] == rmax[i][ch] >= pl["R"] and src["init_src"] == pl["init_src"]
    # the runs plan_bcd finds: at most three, tiling the table, each with its self-initialising planes first
    at = 0
    for r in p["runs"]:
        assert r["plane0"] == at
        mine = range(at, at + r["nplanes"])
        self_init = [p["planes"][k]["init_src"] == k for k in mine]
        assert self_init == sorted(self_init, reverse=True) and r["nbase"] == sum(self_init)
        if split:
            assert {fam(p["planes"][k]["R"]) for k in mine} == {r["fam"]}
        at += r["nplanes"]
    assert at == 3 * m and 1 <= len(p["runs"]) <= 3
    assert len(p["runs"]) == (len({fam(c["R"][ch]) for c in cands for ch in range(3)}) if split else 1)
    return p


SIZES = [(64, 96), (40, 272), (45, 61), (32, 272), (173, 264), (24, 48)]  # 16-aligned, even, odd x odd, 16-aligned, odd x even, even
CANDS = [[(4, 2, 2), (12, 6, 6), (20, 10, 10)],                                     # one image across the three families
         [(7, 3, 3)],                                                               # a single candidate
         [(4, 2, 2), (6, 2, 2)],                                                    # a channel rank shared: the first of equals initialises
         [(8, 8, 5), (16, 9, 16), (26, 13, 13), (32, 16, 16), (1, 1, 1), (9, 4, 4)],  # six candidates
         [(12, 6, 6), (7, 3, 3)],                                                   # the largest rank first
         [(5, 5, 5), (5, 5, 5), (3, 9, 1), (17, 1, 8)]]                             # equal triples; maxima of the channels in different candidates


def test_mixed_list_small_call_keeps_one_run(lib):
    ims, cands = make(SIZES, CANDS, with_sign=[True, False, True, True, False, True])
    assert {len(c) for c in CANDS} >= {1, 2, 3, 6} and len(cands) == 18
    p = check(lib, ims, cands, expect_split=False)
    assert len(p["runs"]) == 1 and p["runs"][0]["nbase"] == 3 * len(SIZES) and p["runs"][0]["fam"] == 2
    assert p["launches"] == 4  # 16-aligned, (2,2), (3,2), (3,3) windows


def test_mixed_list_split_by_family(lib):
    ims, cands = make(SIZES, CANDS, with_sign=[False, True, True, False, True, True])
    p = check(lib, ims, cands, split_blocks=0, expect_split=True)
    assert [r["fam"] for r in p["runs"]] == [0, 1, 2]
    assert sum(r["nbase"] for r in p["runs"]) == 3 * len(SIZES)
    # image 0 at (4,2,2), (12,6,6), (20,10,10): its luma initialisation sits in family 2, the lower ranks point across families
    luma0 = [pl for pl in p["planes"] if cands[pl["cand"]]["image"] == 0 and pl["ch"] == 0]
    assert sorted(pl["R"] for pl in luma0) == [4, 12, 20] and len({pl["init_src"] for pl in luma0}) == 1
    assert p["planes"][luma0[0]["init_src"]]["R"] == 20


def test_equal_ranks_take_the_first_of_them(lib):
    ims, cands = make([(45, 61)], [[(4, 2, 2), (6, 2, 2), (6, 1, 2)]], interleave=False)
    p = check(lib, ims, cands)
    by = {(pl["cand"], pl["ch"]): k for k, pl in enumerate(p["planes"])}
    assert [p["planes"][by[(j, 0)]]["init_src"] for j in range(3)] == [by[(1, 0)]] * 3   # luma: the first rank 6
    assert [p["planes"][by[(j, 1)]]["init_src"] for j in range(3)] == [by[(0, 1)]] * 3   # Cb: the first rank 2
    assert [p["planes"][by[(j, 2)]]["init_src"] for j in range(3)] == [by[(0, 2)]] * 3


def test_candidates_may_lie_anywhere(lib):
    a = check(lib, *make(SIZES, CANDS, interleave=True), split_blocks=0)
    b = check(lib, *make(SIZES, CANDS, interleave=False), split_blocks=0)
    assert a["x_floats"] == b["x_floats"] and a["bcd_blocks"] == b["bcd_blocks"]
    ims, cands = make(SIZES, CANDS)
    cands = cands[::-1]  # offsets no longer ascend with the list
    check(lib, ims, cands)


@pytest.mark.parametrize("split_blocks", [-1, 0])
def test_one_candidate_per_image_is_the_ragged_encoders_table(lib, split_blocks):
    triples = [(7, 3, 3), (12, 6, 6), (26, 13, 13), (16, 9, 16), (1, 1, 1), (32, 16, 16)]
    sizes = [SIZES[i % 6] for i in range(18)]
    ims, cands = make(sizes, [[triples[(i + i // 6) % 6]] for i in range(18)], with_sign=[i % 2 == 0 for i in range(18)], interleave=False)
    assert [c["image"] for c in cands] == list(range(18))
    p = check(lib, ims, cands, split_blocks)
    assert all(pl["init_src"] == k for k, pl in enumerate(p["planes"]))
    n = len(ims)
    arr = lambda xs, key: (L * len(xs))(*[x[key] for x in xs])
    rc = lib.lrf_test_ragged_sweep_equals_ragged(n, arr(ims, "H"), arr(ims, "W"), arr(ims, "rgb_off"), arr(ims, "sign_off"),
                                                 (ctypes.c_int * n)(*[int(im["aligned8"]) for im in ims]),
                                                 (ctypes.c_int * (3 * n))(*[r for c in cands for r in c["R"]]), arr(cands, "u_off"), arr(cands, "v_off"),
                                                 L(split_blocks))
    assert rc == 0, f"field group {rc} differs from plan_encode_ragged's"


def test_default_thresholds_count_candidates_not_images(lib):
    """512x768: 16 + 4 + 4 = 24 blocks per candidate.  One image at 43 candidates within rank 8 reaches 1024 blocks, the count at
    which a call without a rank above 16 splits; 42 do not.  X stays one image's."""
    for k, want in ((42, False), (43, True)):
        ims, cands = make([(512, 768)], [[(1 + j % 8, 1, 1) for j in range(k)]])
        p = check(lib, ims, cands, expect_split=want)
        assert p["bcd_blocks"] == 24 * k and p["x_floats"] == 64 * sum(geom(512, 768))


def test_a_total_of_2_to_the_31_blocks_is_refused(lib):
    """one image of 26000 x 26000 (3 H W < 2^31): 41261 blocks per candidate; 52047 candidates pass 2^31, 52046 do not reach it"""
    per = sum(-(-m // 384) for m in geom(26000, 26000))
    assert per == 41261 and 52047 * per >= 2 ** 31 > 52046 * per
    im = dict(H=26000, W=26000, rgb_off=0, sign_off=-1, aligned8=True)
    cand = dict(image=0, R=(7, 3, 3), u_off=0, v_off=0)
    p = plan(lib, [im], [cand] * 52047)
    assert p["too_many"] == 52047 * per and p["x_floats"] == 0 and p["bcd_blocks"] == 0 and p["nblocks"] == 0 and p["launches"] == 0
