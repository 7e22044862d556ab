"""CPU suite: the tables of the ragged metrics (plan_metrics_ragged, plan_metrics_chunks: lrf_amd/csrc/lrf_plan.cpp).  The plan
source needs no device: it is built here with g++ together with tests/metrics_ragged_plan_shim.cpp and called through ctypes.

The expectations are a Python restatement of the uniform entry's tiling — tiles of 24 x 64 window positions over the
(H - 6) x (W - 6) positions of a plane — and of the workgroup map of k_ragged_ssim_tiles: workgroup w belongs to the last pair
whose wg0 <= w, and inside it to channel (w - wg0) // nt, tile (w - wg0) % nt."""
import bisect
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
OK, BAD_N, BAD_C, BAD_SIZE, NEGATIVE, BAD_A, BAD_B, TOO_MANY = range(8)
PRE_BYTES = 256 * 16 * 8
SIZES = [(7, 7), (7, 70), (30, 7), (30, 70), (31, 71), (54, 134), (55, 135)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("metrics_plan") / "libmetrics_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "metrics_ragged_plan_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_plan_metrics_chunks.restype = ctypes.c_long
    return lib


def tiles(H, W):
    return -(-(H - 6) // 24), -(-(W - 6) // 64)


def vec_of(bits):
    return 16 if bits % 16 == 0 else (4 if bits % 4 == 0 else 1)


def plan(lib, pairs, C=3, a_len=1 << 40, b_len=1 << 40, a_base=0, b_base=0, want_ssim=True):
    n = len(pairs)
    flat = (ctypes.c_long * (4 * max(n, 1)))(*[v for p in pairs for v in p])
    out_pairs = (ctypes.c_long * (10 * max(n, 1)))()
    out_spans = (ctypes.c_long * (5 * max(n, 1)))()
    counts, refusal = (ctypes.c_long * 4)(), (ctypes.c_long * 4)()
    rc = lib.lrf_test_plan_metrics_ragged(ctypes.c_long(n), flat, C, ctypes.c_long(a_len), ctypes.c_long(b_len), ctypes.c_long(a_base),
                                          ctypes.c_long(b_base), int(want_ssim), out_pairs, out_spans, ctypes.c_long(max(n, 1)), counts, refusal)
    assert rc >= 0
    P = [dict(zip(("a_off", "b_off", "H", "W", "ntx", "nt", "wg0", "src", "vec", "pad"), out_pairs[10 * i:10 * i + 10])) for i in range(counts[0])]
    S = [dict(zip(("a_off", "b_off", "n", "wg0", "vec"), out_spans[5 * i:5 * i + 5])) for i in range(counts[1])]
    return rc, P, S, list(counts), list(refusal)


def back_to_back(sizes, C=3, step=16):
    """pairs (H, W, a_off, b_off) of images laid back to back in steps of `step` bytes"""
    pairs, off = [], 0
    for H, W in sizes:
        pairs.append((H, W, off, off))
        off = -(-(off + C * H * W) // step) * step
    return pairs, off


def test_tile_counts_and_slot_offsets():
    assert [tiles(*s) for s in SIZES] == [(1, 1), (1, 1), (1, 1), (1, 1), (2, 2), (2, 2), (3, 3)]


@pytest.mark.parametrize("C", [1, 3])
def test_pairs_follow_the_uniform_tiling(lib, C):
    pairs, total = back_to_back(SIZES, C)
    rc, P, S, counts, _ = plan(lib, pairs, C=C, a_len=total, b_len=total)
    assert rc == OK and len(P) == len(SIZES)
    wg = 0
    for d, (H, W, a_off, b_off) in zip(P, pairs):
        nty, ntx = tiles(H, W)
        assert (d["H"], d["W"], d["a_off"], d["b_off"], d["pad"]) == (H, W, a_off, b_off, 0)
        assert (d["ntx"], d["nt"], d["wg0"]) == (ntx, ntx * nty, wg)
        wg += C * ntx * nty
    assert counts[2] == wg


def test_every_pair_channel_tile_exactly_once(lib):
    C = 3
    pairs, total = back_to_back(SIZES + SIZES[::-1])
    rc, P, _, counts, _ = plan(lib, pairs, C=C, a_len=total, b_len=total)
    assert rc == OK
    starts = [d["wg0"] for d in P]
    assert starts == sorted(starts) and starts[0] == 0
    seen = set()
    for w in range(counts[2]):
        i = bisect.bisect_right(starts, w) - 1  # the kernel's search: the last pair whose wg0 <= w
        d = P[i]
        local = w - d["wg0"]
        ch, tile = divmod(local, d["nt"])
        ty, tx = divmod(tile, d["ntx"])
        nty, ntx = tiles(d["H"], d["W"])
        assert ch < C and ty < nty and tx < ntx
        seen.add((i, ch, ty, tx))
    assert len(seen) == counts[2] == sum(C * tiles(H, W)[0] * tiles(H, W)[1] for H, W, _, _ in pairs)


def test_load_width_from_offsets_and_row_length(lib):
    # (W, a_off, b_off, a_base, b_base) -> the widest of 16, 4, 1 that divides every one of them
    cases = [(64, 0, 0, 0, 0, 16), (64, 16, 32, 256, 512, 16), (64, 4, 0, 0, 0, 4), (64, 0, 0, 8, 0, 4), (68, 0, 0, 0, 0, 4),
             (64, 1, 0, 0, 0, 1), (70, 0, 0, 0, 0, 1), (64, 0, 0, 0, 3, 1), (64, 12, 4, 4, 12, 16)]
    for W, a_off, b_off, a_base, b_base, want in cases:
        rc, P, S, _, _ = plan(lib, [(16, W, a_off, b_off)], a_base=a_base, b_base=b_base)
        assert rc == OK and P[0]["vec"] == want == vec_of((a_base + a_off) | (b_base + b_off) | W), (W, a_off, b_off, a_base, b_base)
        assert S[0]["vec"] == vec_of((a_base + a_off) | (3 * 16 * W))  # the flat read of a alone


def test_shared_sources_are_deduplicated(lib):
    # pairs 0, 2, 4 read one a image; pair 3 starts where they do but is of another size: a source of its own
    pairs = [(30, 70, 0, 0), (31, 71, 6400, 6400), (30, 70, 0, 13200), (35, 60, 0, 19600), (30, 70, 0, 26000)]
    rc, P, S, counts, _ = plan(lib, pairs)
    assert rc == OK
    assert [d["src"] for d in P] == [0, 1, 0, 2, 0]
    assert [(s["a_off"], s["n"]) for s in S] == [(0, 3 * 30 * 70), (6400, 3 * 31 * 71), (0, 3 * 35 * 60)]
    wg = 0
    for s in S:
        assert s["wg0"] == wg
        wg += -(-s["n"] // PRE_BYTES)
    assert counts[3] == wg
    # a large source takes several workgroups of the flat read
    rc, _, S, counts, _ = plan(lib, [(200, 300, 0, 0), (200, 300, 0, 180000), (7, 7, 16, 0)])
    assert rc == OK and [s["wg0"] for s in S] == [0, -(-3 * 200 * 300 // PRE_BYTES)] and counts[3] == S[1]["wg0"] + 1


def test_squared_error_alone_reads_the_pairs(lib):
    pairs = [(3, 5, 0, 1), (30, 70, 64, 64), (3, 5, 0, 128)]
    rc, P, S, counts, _ = plan(lib, pairs, want_ssim=False)
    assert rc == OK and counts[2] == 0
    assert [(s["a_off"], s["b_off"], s["n"], s["vec"]) for s in S] == [(0, 1, 45, 1), (64, 64, 6300, 4), (0, 128, 45, 1)]
    assert plan(lib, pairs, want_ssim=True)[0] == BAD_SIZE  # 3x5 is below the window


def chunks(lib, sizes, cap):
    n = len(sizes)
    out, off, mx = (ctypes.c_long * (3 * n))(), (ctypes.c_long * n)(), ctypes.c_long()
    k = lib.lrf_test_plan_metrics_chunks(ctypes.c_long(n), (ctypes.c_long * (2 * n))(*[v for s in sizes for v in s]), ctypes.c_long(cap), out, off,
                                         ctypes.byref(mx))
    return [tuple(out[3 * j:3 * j + 3]) for j in range(k)], list(off), mx.value


def test_chunking(lib):
    sizes = [(7, 7), (30, 70), (31, 71), (7, 70), (54, 134)]
    b = [-(-3 * H * W // 16) * 16 for H, W in sizes]
    assert b[0] == 160 and b[1] == 6304
    # a cap of one byte: every item is larger than the cap and gets a chunk of its own
    ch, off, mx = chunks(lib, sizes, 1)
    assert ch == [(i, 1, b[i]) for i in range(5)] and off == [0] * 5 and mx == max(b)
    # exactly one item: items 0 and 1 would fit together only with b[0] + b[1]
    ch, off, mx = chunks(lib, sizes, b[1])
    assert ch == [(0, 1, b[0]), (1, 1, b[1]), (2, 1, b[2]), (3, 1, b[3]), (4, 1, b[4])]
    ch, off, mx = chunks(lib, sizes, b[0] + b[1])
    assert ch[0] == (0, 2, b[0] + b[1]) and off[:2] == [0, b[0]]
    # everything
    ch, off, mx = chunks(lib, sizes, sum(b))
    assert ch == [(0, 5, sum(b))] and mx == sum(b)
    assert off == [sum(b[:i]) for i in range(5)] and all(o % 16 == 0 for o in off)
    ch, _, _ = chunks(lib, sizes, sum(b) - 1)
    assert ch == [(0, 4, sum(b[:4])), (4, 1, b[4])]


@pytest.mark.parametrize("pairs, kw, check, who", [
    ([], {}, BAD_N, 0),
    ([(8, 8, 0, 0)] * 65536, {}, BAD_N, 0),
    ([(8, 8, 0, 0)], dict(C=0), BAD_C, 0),
    ([(8, 8, 0, 0)], dict(C=65536), BAD_C, 0),
    ([(8, 8, 0, 0), (6, 8, 0, 0)], {}, BAD_SIZE, 1),
    ([(8, 8, 0, 0), (8, 6, 0, 0)], {}, BAD_SIZE, 1),
    ([(0, 8, 0, 0)], dict(want_ssim=False), BAD_SIZE, 0),
    ([((1 << 20) + 1, 8, 0, 0)], {}, BAD_SIZE, 0),
    ([(1 << 20, 1 << 20, 0, 0)], {}, BAD_SIZE, 0),
    ([(8, 8, 0, 0), (8, 8, -1, 0)], {}, NEGATIVE, 1),
    ([(8, 8, 0, -16)], {}, NEGATIVE, 0),
    ([(8, 8, 0, 0), (8, 8, 9, 0)], dict(a_len=200), BAD_A, 1),
    ([(8, 8, 0, 0)], dict(a_len=191), BAD_A, 0),
    ([(8, 8, 0, 9)], dict(b_len=200), BAD_B, 0),
    ([(8, 8, (1 << 62), 0)], dict(a_len=(1 << 62) + 10), BAD_A, 0),
    ([(1 << 19, 1 << 19, 0, 0)] * 5, {}, TOO_MANY, 3),
])
def test_refusals_build_nothing(lib, pairs, kw, check, who):
    rc, P, S, counts, refusal = plan(lib, pairs, **kw)
    assert rc == check and refusal[0] == check and refusal[1] == who
    assert P == [] and S == [] and counts == [0, 0, 0, 0]


def test_exact_fit_is_accepted(lib):
    rc, P, S, _, _ = plan(lib, [(8, 8, 8, 0)], a_len=200, b_len=192)
    assert rc == OK and len(P) == 1 and len(S) == 1
