"""CPU suite: the launches of a ragged decode (plan_decode_ragged, lrf_amd/csrc/lrf_plan.cpp).  The plan source needs no device:
it is built here with g++ together with tests/decode_ragged_plan_shim.cpp and called through ctypes.

An image enters the planner as (kind, class, units), the way describe_images hands it over after decode_plan (both in
lrf_plan.cpp) has classified it.  Here the classification is done by `classify` below, written from the rule in decode_plan's
comment and the geometry of lrf/compression/qmf.py:230-242 — independently of the library, and compared with the library's
decode_plan over a grid (test_classify_is_the_librarys_decode_plan) — and the expected groups follow from it:
  * every 16-aligned image within ranks (32,16,16) (DEC_TILE16), whatever its class      -> one launch
  * the other images the tiled body covers (DEC_STRIP)                                    -> one launch per class present
  * ranks <= 8 elsewhere (DEC_R8), everything else (DEC_ANY)                              -> one launch each
and every (image, tile) of an image must appear exactly once, in the launch of its group."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
TILE16, STRIP, R8, ANY = range(4)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ragged_plan") / "libragged_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "decode_ragged_plan_shim.cpp")])
    return ctypes.CDLL(so)


def classify(H, W, ranks, aligned8=True, no_tiled=False):
    """(kind, cls, units) of an image: the rule of decode_plan's comment.  Planes: luma H x W, chroma floor(H/2) x floor(W/2),
    reflect-padded to multiples of 8 with the smaller half of the padding on the left / top.  no_tiled: the developer switch
    LRF_DECODE_NO_TILED (no image takes a tiled body)."""
    w = [W, W // 2]
    wp = [-(-x // 8) * 8 for x in w]
    left = [(p - x) // 2 for p, x in zip(wp, w)]
    nw, nh = wp[0] // 8, -(-H // 8)
    rcm = max(ranks[1], ranks[2])
    tiled_ranks = ranks[0] <= 32 and rcm <= 16 and not no_tiled
    sides16 = H % 16 == 0 and W % 16 == 0 and aligned8
    strip_ok = W % 2 == 0 and left[0] % 2 == 0 and (left[1] - left[0] // 2) % 4 == 0
    per_strip = (nw + 31) // 32
    if tiled_ranks and (sides16 or strip_ok):
        rl = 8 if ranks[0] <= 8 else (16 if ranks[0] <= 16 else 32)
        rc = 4 if rcm <= 4 else (8 if rcm <= 8 else 16)
        cls = {(8, 4): 0, (8, 8): 1, (16, 4): 2, (16, 8): 2, (8, 16): 3, (16, 16): 3}.get((rl, rc), 4)
        return (TILE16, cls, (H // 16) * per_strip) if sides16 else (STRIP, cls, ((nh + 1) // 2) * per_strip)
    return (R8 if max(ranks) <= 8 else ANY), 0, H * ((W + 3) // 4)


def plan(lib, work, cap=None):
    n = len(work)
    cap = sum(u for _, _, u in work) + 16 if cap is None else cap
    launches = (ctypes.c_long * (5 * 16))()
    blocks = (ctypes.c_int * (2 * cap))()
    nblocks, too_many = ctypes.c_long(), ctypes.c_long()
    nl = lib.lrf_test_plan_decode_ragged(n, (ctypes.c_int * n)(*[w[0] for w in work]), (ctypes.c_int * n)(*[w[1] for w in work]),
                                         (ctypes.c_long * n)(*[w[2] for w in work]), launches, 16, blocks, cap, ctypes.byref(nblocks),
                                         ctypes.byref(too_many))
    assert nl >= 0
    L = [dict(zip(("kind", "cls", "block0", "nblocks", "reps"), launches[5 * j:5 * j + 5])) for j in range(nl)]
    B = [(blocks[2 * j], blocks[2 * j + 1]) for j in range(nblocks.value)]
    return L, B, too_many.value


def check(lib, work):
    """the properties every plan must have; -> its launches"""
    L, B, too_many = plan(lib, work)
    assert too_many == 0
    assert 1 <= len(L) <= 8
    # the launches tile the block table, in the documented order
    at = 0
    for l in L:
        assert l["block0"] == at and l["nblocks"] > 0
        at += l["nblocks"]
    assert at == len(B)
    keys = [(l["kind"], l["cls"] if l["kind"] == STRIP else 0) for l in L]
    assert keys == sorted(set(keys))
    # expected groups, from the classification alone
    want = {}
    for i, (kind, cls, _) in enumerate(work):
        want.setdefault((kind, cls if kind == STRIP else 0), []).append(i)
    assert sorted(want) == keys
    seen = set()
    for l, key in zip(L, keys):
        reps = l["reps"]
        assert reps == 1 or l["kind"] == R8
        assert l["cls"] == (-1 if l["kind"] == TILE16 else (key[1] if l["kind"] == STRIP else 0))
        mine = B[l["block0"]:l["block0"] + l["nblocks"]]
        assert sorted({i for i, _ in mine}) == want[key]
        for i, t in mine:
            assert (i, t) not in seen
            seen.add((i, t))
        assert mine == sorted(mine)  # images in call order, tiles ascending
        for i in want[key]:
            kind, _, units = work[i]
            nb = units if kind in (TILE16, STRIP) else -(-units // (256 * reps))
            assert [t for j, t in mine if j == i] == list(range(nb)), (i, nb)
    return L


CLASS_TRIPLES = [(7, 3, 3), (8, 8, 5), (12, 6, 6), (16, 9, 16), (26, 13, 13)]  # classes 0..4


def test_classes_are_what_the_triples_are_meant_to_hit():
    assert [classify(64, 96, r)[1] for r in CLASS_TRIPLES] == [0, 1, 2, 3, 4]
    assert classify(64, 96, (1, 1, 1))[:2] == (TILE16, 0) and classify(64, 96, (32, 16, 16))[:2] == (TILE16, 4)
    assert classify(32, 272, (7, 3, 3)) == (TILE16, 0, 2 * 2)        # 34 luma patches per row: two tiles per strip
    assert classify(40, 272, (7, 3, 3)) == (STRIP, 0, 3 * 2) and classify(24, 48, (12, 6, 6)) == (STRIP, 2, 2)
    assert classify(45, 61, (7, 3, 3))[0] == R8 and classify(173, 264, (7, 3, 3))[0] == R8
    assert classify(173, 264, (12, 6, 6))[0] == ANY
    for r in ((33, 4, 4), (5, 17, 2), (64, 64, 64)):
        assert classify(64, 96, r)[0] == ANY and classify(40, 272, r)[0] == ANY


GRID_SIDES = list(range(8, 41)) + [45, 61, 64, 96, 173, 264, 272]
GRID_RANKS = [(1, 1, 1), (8, 4, 4), (8, 5, 4), (8, 8, 8), (9, 8, 8), (16, 8, 8), (16, 9, 8), (8, 16, 16), (17, 16, 16), (32, 16, 16), (33, 16, 16),
              (32, 17, 1), (64, 64, 64)]


def test_classify_is_the_librarys_decode_plan(lib):
    """the rule restated above against decode_plan itself, at every point of the grid: every side is at least 8, which geom_of
    accepts for both planes (asserted: the library answers a plan, never a refusal), so the restated rule covers all of it"""
    points = 0
    for no_tiled in (False, True):
        for H in GRID_SIDES:
            for W in GRID_SIDES:
                for r in GRID_RANKS:
                    for aligned8 in (True, False):
                        got = lib.lrf_test_decode_plan(H, W, r[0], r[1], r[2], aligned8, no_tiled)
                        assert got >= 0, (H, W, got)
                        assert divmod(got, 8) == classify(H, W, r, aligned8, no_tiled)[:2], (H, W, r, aligned8, no_tiled)
                        points += 1
    assert points == 2 * len(GRID_SIDES) ** 2 * len(GRID_RANKS) * 2
    assert not any(classify(H, 64, r, True, True)[0] in (TILE16, STRIP) for H in GRID_SIDES for r in GRID_RANKS)


def test_aligned_images_of_all_five_classes_share_one_launch(lib):
    work = [classify(H, W, r) for r in CLASS_TRIPLES for H, W in ((64, 96), (32, 272))]
    assert {w[0] for w in work} == {TILE16} and {w[1] for w in work} == set(range(5))
    L = check(lib, work)
    assert len(L) == 1 and L[0]["kind"] == TILE16 and L[0]["cls"] == -1


def test_strip_images_of_three_classes_take_three_launches(lib):
    work = [classify(H, W, r) for H, W in ((40, 272), (24, 48)) for r in ((7, 3, 3), (12, 6, 6), (26, 13, 13), (1, 1, 1))]
    assert {w[0] for w in work} == {STRIP}
    L = check(lib, work)
    assert [(l["kind"], l["cls"]) for l in L] == [(STRIP, 0), (STRIP, 2), (STRIP, 4)]


def test_mix_of_all_four_kinds(lib):
    sizes = [(32, 272), (45, 61), (40, 272), (173, 264), (64, 96), (24, 48)]
    triples = CLASS_TRIPLES + [(33, 4, 4), (1, 1, 1), (64, 64, 64)]
    work = [classify(*sizes[i % len(sizes)], triples[(i * 3) % len(triples)]) for i in range(31)]
    assert {w[0] for w in work} == {TILE16, STRIP, R8, ANY}
    L = check(lib, work)
    assert [l["kind"] for l in L][0] == TILE16 and [l["kind"] for l in L][-2:] == [R8, ANY]


def test_all_eight_launches(lib):
    work = [classify(64, 96, (7, 3, 3))] + [classify(40, 272, r) for r in CLASS_TRIPLES] + [classify(45, 61, (7, 3, 3)), classify(45, 61, (9, 3, 3))]
    assert len(check(lib, work)) == 8


def test_unaligned_output_turns_an_aligned_image_into_a_strip_image(lib):
    a, b = classify(64, 96, (7, 3, 3), aligned8=True), classify(64, 96, (7, 3, 3), aligned8=False)
    assert a == (TILE16, 0, 4) and b == (STRIP, 0, 4)
    L = check(lib, [a, b, a])
    assert [(l["kind"], l["nblocks"]) for l in L] == [(TILE16, 8), (STRIP, 4)]


def test_one_image(lib):
    for im in (classify(64, 96, (7, 3, 3)), classify(24, 48, (16, 9, 16)), classify(45, 61, (1, 1, 1)), classify(45, 61, (64, 64, 64))):
        L = check(lib, [im])
        assert len(L) == 1 and L[0]["kind"] == im[0]


def test_reps_of_the_rank8_launch_follow_its_total(lib):
    """decode8_reps: total groups of 256 pixel quads / 2048, between 1 and 16.  173x264: 173 * 66 = 11418 quads = 45 groups"""
    im = classify(173, 264, (7, 3, 3))
    assert im == (R8, 0, 11418)
    for n, reps in ((1, 1), (91, 1), (92, 2), (400, 8), (2000, 16)):  # 91 * 45 = 4095 < 4096 <= 92 * 45
        L = check(lib, [im] * n)
        assert L[0]["reps"] == reps and L[0]["nblocks"] == n * -(-11418 // (256 * reps))


def test_a_launch_of_2_to_the_31_workgroups_is_refused(lib):
    L, B, too_many = plan(lib, [(ANY, 0, 256 * 2 ** 30)] * 2 + [(TILE16, 0, 4)], cap=16)
    assert too_many == 2 ** 31 and L == [] and B == []
    L, B, too_many = plan(lib, [(TILE16, 0, 4)])
    assert too_many == 0 and len(B) == 4
