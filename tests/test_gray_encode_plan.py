"""CPU suite: the list check and the tables of a ragged gray encode (describe_gray_encode, plan_encode_gray_ragged_sweep,
lrf_amd/csrc/lrf_plan.cpp).  The plan source needs no device: it is built here with g++ together with
tests/gray_encode_plan_shim.cpp and called through ctypes.

What is expected is worked out below from the rules alone — never by the library:
  * geometry (lrf_chan_dims(H, W, 1, 8, 8)): reflect padding to multiples of 8, top = pad // 2, left = pad // 2; M = patches of
    8 x 8; X holds one matrix [M][64] per IMAGE, the images back to back — once per image, however many candidates it has
  * the planes stage: an image with W % 16 == 0 whose bytes start at a multiple of 16 takes the 16-byte body, (hp / 8)(W / 16) 8
    items; every other image the general body, 16 M items; 256 items to a workgroup; one launch per body present, the 16-byte
    body first; inside a launch the images in call order, an image's workgroups ascending
  * one plane per candidate, one block per 384 rows, its factors at the candidate's offsets, its signs at the image's
  * init_src: the plane of the image's first candidate of largest rank
  * order: by kernel family (rank <= 8, <= 16, <= 32) when the call splits, inside a family the self-initialising planes first,
    candidates in list order"""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
L = ctypes.c_long
SIZES = [(8, 8), (16, 24), (37, 53), (64, 96), (56, 440), (173, 264), (48, 400)]
(GENC_OK, GENC_N, GENC_M, GENC_SIZE, GENC_GEOM, GENC_PIXELS, GENC_NEGATIVE, GENC_GRAY, GENC_K, GENC_BOUNDS, GENC_IMAGE, GENC_RANK_LOW, GENC_RANK_BIG, GENC_U,
 GENC_V, GENC_NO_CAND, GENC_SIGN, GENC_OVERLAP_U, GENC_OVERLAP_V) = range(19)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gray_encode_plan") / "libgray_encode_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "gray_encode_plan_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_describe_gray_encode.restype = None
    return lib


def geom(H, W):
    """(M, top, left, nh, nw)"""
    ph, pw = (-H) % 8, (-W) % 8
    nh, nw = (H + ph) // 8, (W + pw) // 8
    return nh * nw, ph // 2, pw // 2, nh, nw


def fam(r):
    return 0 if r <= 8 else (1 if r <= 16 else 2)


def make(sizes, cand_lists, with_sign=None, interleave=True, base=0):
    """sizes: (H, W) per image; cand_lists: per image its ranks -> (images, candidates) as the entry point would hand them over:
    pixels 16-aligned back to back behind a buffer `base` bytes past alignment, the candidates of the images interleaved
    round-robin, factors back to back in list order, signs (where asked for) back to back at the image's largest rank"""
    ims, go, so = [], 0, 0
    for i, (H, W) in enumerate(sizes):
        sign = with_sign is not None and with_sign[i]
        ims.append(dict(H=H, W=W, gray_off=go, sign_off=so if sign else -1, aligned16=(base + go) % 16 == 0))
        go = (go + H * W + 15) // 16 * 16
        so += max(cand_lists[i]) if sign else 0
    if interleave:
        order = [(i, k) for k in range(max(len(ts) for ts in cand_lists)) for i in range(len(sizes)) if k < len(cand_lists[i])]
    else:
        order = [(i, k) for i in range(len(sizes)) for k in range(len(cand_lists[i]))]
    cands, uo, vo = [], 0, 0
    for i, k in order:
        R = cand_lists[i][k]
        cands.append(dict(image=i, R=R, u_off=uo, v_off=vo))
        uo += geom(*sizes[i])[0] * R
        vo += 64 * R
    return ims, cands


def arr(xs, key, t=L):
    return (t * max(len(xs), 1))(*[int(x[key]) for x in xs])


def plan(lib, ims, cands, split_blocks=-1, max_blocks=1 << 16):
    n, m = len(ims), len(cands)
    planes, descs, launches, blocks, runs, out = (L * (10 * m))(), (L * (8 * n))(), (L * 6)(), (L * (2 * max_blocks))(), (L * (4 * 8))(), (L * 7)()
    rc = lib.lrf_test_plan_gray_encode(n, arr(ims, "H"), arr(ims, "W"), arr(ims, "gray_off"), arr(ims, "sign_off"), arr(ims, "aligned16", ctypes.c_int), m,
                                       arr(cands, "image", ctypes.c_int), arr(cands, "R", ctypes.c_int), arr(cands, "u_off"), arr(cands, "v_off"),
                                       L(split_blocks), planes, descs, launches, blocks, L(max_blocks), runs, 8, out)
    assert rc == 0, rc
    res = dict(zip(("nblocks", "bcd_blocks", "split", "x_floats", "too_many", "launches", "nruns"), out))
    if res["too_many"]:
        return res
    res["planes"] = [dict(zip(("cand", "x_off", "u_off", "v_off", "M", "R", "sign_off", "blk0", "nblk", "init_src"), planes[10 * j:10 * j + 10])) for j in range(m)]
    res["descs"] = [dict(zip(("gray_off", "x_off", "H", "W", "top", "left", "nw", "items"), descs[8 * i:8 * i + 8])) for i in range(n)]
    res["launch_list"] = [tuple(launches[3 * k:3 * k + 3]) for k in range(res["launches"])]
    res["blocks"] = [(blocks[2 * b], blocks[2 * b + 1]) for b in range(res["nblocks"])]
    res["runs"] = [dict(zip(("plane0", "nplanes", "nbase", "fam"), runs[4 * r:4 * r + 4])) for r in range(res["nruns"])]
    return res


def check(lib, ims, cands, split_blocks=-1, expect_split=None):
    """the properties every plan must have; -> the plan"""
    p = plan(lib, ims, cands, split_blocks)
    n, m = len(ims), len(cands)
    assert p["too_many"] == 0
    g = [geom(im["H"], im["W"]) for im in ims]
    # X and the descriptors: once per image
    x, body, units = 0, [], []
    for i, (im, d) in enumerate(zip(ims, p["descs"])):
        M, top, left, nh, nw = g[i]
        b16 = im["W"] % 16 == 0 and im["aligned16"]
        items = nh * (im["W"] // 16) * 8 if b16 else 16 * M
        assert d == dict(gray_off=im["gray_off"], x_off=x, H=im["H"], W=im["W"], top=top, left=left, nw=nw, items=items), i
        x += 64 * M
        body.append(0 if b16 else 1)
        units.append(-(-items // 256))
    assert p["x_floats"] == x
    # the planes stage: one launch per body present, the 16-byte body first; the workgroup table
    want_launches, want_blocks = [], []
    for b in (0, 1):
        mine = [(i, u) for i in range(n) if body[i] == b for u in range(units[i])]
        if mine:
            want_launches.append((b, len(want_blocks), len(mine)))
            want_blocks += mine
    assert p["launch_list"] == want_launches and p["blocks"] == want_blocks and p["nblocks"] == sum(units)
    for i in range(n):  # (every item of every image is some workgroup's)
        assert 256 * (units[i] - 1) < p["descs"][i]["items"] <= 256 * units[i]
    rmax = [max(c["R"] for c in cands if c["image"] == i) for i in range(n)]
    base = [min(j for j, c in enumerate(cands) if c["image"] == i and c["R"] == rmax[i]) for i in range(n)]
    total = sum(-(-g[c["image"]][0] // 384) for c in cands)
    assert p["bcd_blocks"] == total
    rmax_t = max(c["R"] for c in cands)
    split = total >= (split_blocks if split_blocks >= 0 else (256 if rmax_t > 16 else 1024))
    assert bool(p["split"]) == split
    if expect_split is not None:
        assert split == expect_split
    order = [j for f in range(3 if split else 1) for self_init in (True, False) for j, c in enumerate(cands)
             if (not split or fam(c["R"]) == f) and ((base[c["image"]] == j) == self_init)]
    assert [pl["cand"] for pl in p["planes"]] == order and sorted(order) == list(range(m))
    where = {j: k for k, j in enumerate(order)}
    blk0 = 0
    for pl, j in zip(p["planes"], order):
        c = cands[j]
        i = c["image"]
        assert (pl["M"], pl["R"]) == (g[i][0], c["R"])
        assert (pl["x_off"], pl["u_off"], pl["v_off"]) == (p["descs"][i]["x_off"], c["u_off"], c["v_off"])
        assert pl["sign_off"] == ims[i]["sign_off"]  # (-1: the default signs; a candidate reads the leading R of the image's)
        assert (pl["blk0"], pl["nblk"]) == (blk0, -(-g[i][0] // 384))
        blk0 += pl["nblk"]
        assert pl["init_src"] == where[base[i]]
        src = p["planes"][pl["init_src"]]
        assert cands[src["cand"]]["image"] == i and src["R"] == rmax[i] >= pl["R"] and src["init_src"] == pl["init_src"]
    # the runs plan_bcd finds: at most three, tiling the table, each with its self-initialising planes first
    at = 0
    for r in p["runs"]:
        assert r["plane0"] == at
        mine = list(range(at, at + r["nplanes"]))
        selfs = [k for k in mine if p["planes"][k]["init_src"] == k]
        assert selfs == mine[:len(selfs)] and r["nbase"] == len(selfs)
        if split:
            assert all(fam(p["planes"][k]["R"]) == r["fam"] for k in mine)
        at += r["nplanes"]
    assert at == m and len(p["runs"]) <= 3
    return p


LISTS = [
    ("in order", list(range(len(SIZES)))),
    ("reversed", list(range(len(SIZES)))[::-1]),
    ("shuffled with duplicates", [3, 0, 6, 3, 5, 1, 4, 2, 6, 0]),
]


@pytest.mark.parametrize("name, picks", LISTS, ids=[n for n, _ in LISTS])
@pytest.mark.parametrize("base", [0, 1], ids=["aligned", "base+1"])
def test_plain_lists(lib, name, picks, base):
    """one candidate per image (the plain ragged encode): bodies by alignment, workgroup counts, X offsets, the table"""
    ranks = [1, 4, 7, 8, 9, 16, 17, 32]
    sizes = [SIZES[k] for k in picks]
    ims, cands = make(sizes, [[ranks[(3 * i + k) % 8]] for i, k in enumerate(picks)], with_sign=[i % 2 == 0 for i in range(len(picks))], base=base)
    p = check(lib, ims, cands, expect_split=False)
    n16 = sum(1 for (H, W) in sizes if W % 16 == 0) if base == 0 else 0
    assert [b for b, _, _ in p["launch_list"]] == ([0, 1] if n16 else [1])
    assert all(pl["init_src"] == k for k, pl in enumerate(p["planes"]))  # every plane initialises itself
    assert [pl["cand"] for pl in p["planes"]] == list(range(len(picks)))  # no split: call order


def test_an_unaligned_offset_inside_an_aligned_buffer(lib):
    """the body is per image: the same 48x400 image at a multiple of 16 and one byte past it"""
    ims, cands = make([(48, 400), (48, 400)], [[7], [7]])
    ims[1]["gray_off"] += 1
    ims[1]["aligned16"] = False
    p = check(lib, ims, cands)
    assert p["launch_list"] == [(0, 0, 5), (1, 5, 19)]  # 6 x 25 x 8 = 1200 items, 16 x 300 = 4800 items


@pytest.mark.parametrize("split_blocks, expect", [(-1, False), (1, True), (10 ** 9, False)])
def test_sweep_order_with_and_without_a_family_split(lib, split_blocks, expect):
    """every image at ranks {1, 3, 8, 9, 20, 32} and one with its largest rank twice, interleaved and image by image"""
    sizes = [SIZES[k] for k in [4, 0, 6, 3, 5, 2]]
    lists = [[1, 3, 8, 9, 20, 32], [32, 20, 9, 8, 3, 1], [8, 32, 1, 32, 3], [3, 1], [16, 9, 12], [7]]
    for interleave in (True, False):
        ims, cands = make(sizes, lists, with_sign=[True, False, True, True, False, True], interleave=interleave)
        p = check(lib, ims, cands, split_blocks, expect_split=expect)
        if expect:
            assert [r["fam"] for r in p["runs"]] == [0, 1, 2]
            # the family of ranks <= 8 holds no self-initialising plane of the images whose largest rank lies above it
            assert p["runs"][0]["nbase"] == 2  # images 3 (ranks 3, 1) and 5 (rank 7)
        else:
            assert len(p["runs"]) == 1 and p["runs"][0]["nbase"] == len(sizes)


def test_default_split_threshold(lib):
    """a list of 256 blocks at rank 17 or more splits, one of 255 does not; below rank 17 the threshold is 1024"""
    for n, R, expect in [(128, 17, True), (127, 17, False), (128, 16, False), (512, 16, True)]:
        ims, cands = make([(56, 440)] * n, [[R]] * n)  # M = 385: two blocks a plane
        check(lib, ims, cands, expect_split=expect)


def test_too_many_builds_nothing(lib):
    """2^31 or more BCD blocks (one 32768 x 32768 image at 65536 candidates: 43691 blocks each) or planes workgroups (4096 such
    images on the general body: 2^20 each): too_many, and no table (the shim checks that every vector is empty)"""
    big = dict(H=32768, W=32768, gray_off=0, sign_off=-1, aligned16=False)
    p = plan(lib, [big], [dict(image=0, R=4, u_off=0, v_off=0)] * 65536)
    assert p["too_many"] == 65536 * 43691 and p["nblocks"] == 0 and p["bcd_blocks"] == 0
    n = 4096
    p = plan(lib, [big] * n, [dict(image=i, R=4, u_off=0, v_off=0) for i in range(n)])
    assert p["too_many"] == n * (1 << 20) and p["nblocks"] == 0


# ---------------------------------------------------------------- the list check
def describe(lib, ims, cands, gray_len, sign_len, u_len, v_len, base=0, K=10, lo=-16, hi=15, n=None, m=None):
    out = (L * (7 + 2 * max(len(ims), 1)))()
    lib.lrf_test_describe_gray_encode(L(len(ims) if n is None else n), L(len(ims)), arr(ims, "H"), arr(ims, "W"), arr(ims, "gray_off"), arr(ims, "sign_off"),
                                      L(len(cands) if m is None else m), L(len(cands)), arr(cands, "image", ctypes.c_int), arr(cands, "R", ctypes.c_int), arr(cands, "u_off"),
                                      arr(cands, "v_off"), L(gray_len), L(sign_len), L(u_len), L(v_len), L(base), K, lo, hi, out)
    return list(out)


def good():
    ims, cands = make([(37, 53), (64, 96), (48, 400)], [[4, 9], [32], [7, 3]], with_sign=[True, False, True])
    lens = dict(gray_len=ims[-1]["gray_off"] + 48 * 400, sign_len=9 + 7, u_len=cands[-1]["u_off"] + 300 * 3, v_len=cands[-1]["v_off"] + 64 * 3)
    return ims, cands, lens


def test_describe_accepts_and_marks_alignment(lib):
    ims, cands, lens = good()
    out = describe(lib, ims, cands, **lens)
    assert out[:7] == [GENC_OK, 0, 0, 0, 0, 3, 5]
    assert out[7:13] == [1, 0, 1, -1, 1, 9]  # (aligned16, sign_off) per image
    assert describe(lib, ims, cands, base=8, **lens)[7:13:2] == [0, 0, 0]
    out = describe(lib, ims, cands, **dict(lens, sign_len=0))  # no sign buffer: every image on the default signs
    assert out[0] == GENC_OK and out[8:13:2] == [-1, -1, -1]


def refusals():
    """(name, a change to the good list, the refusal expected: (check, candidate, index))"""
    def im(i, **kw):
        return lambda ims, cands, lens: ims[i].update(kw)

    def cd(j, **kw):
        return lambda ims, cands, lens: cands[j].update(kw)

    def ln(**kw):
        return lambda ims, cands, lens: lens.update(kw)
    return [
        ("a zero side", im(1, H=0), (GENC_SIZE, 0, 1)),
        ("a side above 2^20", im(2, W=(1 << 20) + 1), (GENC_SIZE, 0, 2)),
        ("reflect padding larger than the image", im(0, H=9, W=2), (GENC_GEOM, 0, 0)),
        ("2^31 pixels", im(1, H=1 << 16, W=1 << 15), (GENC_PIXELS, 0, 1)),
        ("a negative pixel offset", im(2, gray_off=-1), (GENC_NEGATIVE, 0, 2)),
        ("a sign offset below -1", im(0, sign_off=-2), (GENC_NEGATIVE, 0, 0)),
        ("pixels that leave the buffer", ln(gray_len=10000), (GENC_GRAY, 0, 2)),
        ("K = 0", ln(K=0), (GENC_K, 0, 0)),
        ("bounds outside int8", ln(lo=-129), (GENC_BOUNDS, 0, 0)),
        ("bounds in the wrong order", ln(lo=3, hi=2), (GENC_BOUNDS, 0, 0)),
        ("a candidate naming no image", cd(3, image=3), (GENC_IMAGE, 1, 3)),
        ("a negative image index", cd(0, image=-1), (GENC_IMAGE, 1, 0)),
        ("rank 0", cd(1, R=0), (GENC_RANK_LOW, 1, 1)),
        ("rank 33", cd(2, R=33), (GENC_RANK_BIG, 1, 2)),
        ("a negative factor offset", cd(4, v_off=-1), (GENC_NEGATIVE, 1, 4)),
        ("U that leaves the buffer", ln(u_len=1000), (GENC_U, 1, 1)),
        ("V that leaves the buffer", ln(v_len=64 * 4 + 64 * 32 + 1), (GENC_V, 1, 2)),
        ("an image without a candidate", cd(1, image=0, R=4), (GENC_NO_CAND, 0, 1)),
        ("signs that leave the buffer", ln(sign_len=15), (GENC_SIGN, 0, 2)),
        ("overlapping U ranges", cd(1, u_off=35 * 4 - 1), (GENC_OVERLAP_U, 1, 0)),
        ("overlapping V ranges", cd(4, v_off=0), (GENC_OVERLAP_V, 1, 0)),
    ]


@pytest.mark.parametrize("name, change, want", refusals(), ids=[r[0] for r in refusals()])
def test_describe_refuses_and_builds_nothing(lib, name, change, want):
    ims, cands, lens = good()
    change(ims, cands, lens)
    out = describe(lib, ims, cands, **lens)
    assert tuple(out[:3]) == want
    assert out[5:7] == [0, 0]  # neither images nor candidates were built


def test_describe_refuses_the_counts(lib):
    ims, cands, lens = good()
    assert describe(lib, ims, cands, n=0, **lens)[:3] == [GENC_N, 0, 0]
    assert describe(lib, ims, cands, n=65536, **lens)[:3] == [GENC_N, 0, 65536]
    assert describe(lib, ims, cands[:2], **lens)[:3] == [GENC_M, 0, 2]  # fewer candidates than images
    assert describe(lib, ims, cands, m=(1 << 20) + 1, **lens)[:3] == [GENC_M, 0, (1 << 20) + 1]
