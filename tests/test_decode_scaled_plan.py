"""CPU suite: the footprint arithmetic, the thread maps and the launch plan of the decode at 1/2, 1/4, 1/8 scale (lrf_plan.h,
plan_decode_scaled in lrf_amd/csrc/lrf_plan.cpp; the kernels of lrf_decode_scaled_kernel.hip call the same functions).  Built
here with g++ together with tests/decode_scaled_plan_shim.cpp and called through ctypes: no device.

  * for every output row and column of a set of geometries at each scale, the image pixels covered are the block of the
    definition exactly, and the chroma rows under them with their multiplicities are those of nearest_idx (scaled_decode.py);
  * for windows at every origin, the pixel sets of the threads of both bodies are the window exactly: each pixel once, nothing
    outside;
  * the items are grouped by (path, scale, class) in that order, call order kept inside a launch, every item in exactly one
    launch with its place in the call; the tiled items of one (image, scale) share one pooled table; 2^31 workgroups are refused."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from scaled_decode import SCALES, nearest_idx, scaled_dims

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
GEOMETRIES = [(16, 16), (24, 48), (45, 61), (173, 264), (2, 2), (9, 7)]
MAX_LAUNCHES = 18


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scaled_plan") / "libscaled_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "decode_scaled_plan_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_scaled_dim.restype = ctypes.c_long
    lib.lrf_test_scaled_dim.argtypes = [ctypes.c_long, ctypes.c_int]
    lib.lrf_test_scaled_footprint.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    lib.lrf_test_scaled_wgs.restype = ctypes.c_long
    lib.lrf_test_scaled_wgs.argtypes = [ctypes.c_int] * 6
    lib.lrf_test_scaled_cover.restype = ctypes.c_long
    lib.lrf_test_scaled_cover.argtypes = [ctypes.c_int] * 8 + [ctypes.c_long, ctypes.c_void_p]
    lib.lrf_test_plan_decode_scaled.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_scales_and_sizes(lib):
    assert [f for f in range(-1, 20) if lib.lrf_test_scaled_f_ok(f)] == list(SCALES)
    for n in (1, 2, 7, 8, 9, 16, 173, 1365, 2 ** 31 - 1):
        for f in SCALES:
            assert lib.lrf_test_scaled_dim(n, f) == -(-n // f)


@pytest.mark.parametrize("f", SCALES)
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_footprint_is_the_block_and_its_chroma_rows_are_nearest_idx(lib, H, W, f):
    span, rows, mult = np.zeros(2, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
    for n in (H, W):
        nc = n // 2
        idx = nearest_idx(n, nc)
        covered = np.zeros(n, np.int64)
        for i in range(-(-n // f)):
            k = lib.lrf_test_scaled_footprint(i, f, n, nc, span.ctypes.data, rows.ctypes.data, mult.ctypes.data)
            lo, hi = int(span[0]), int(span[1])
            assert (lo, hi) == (f * i, min(f * i + f, n)), (n, f, i)
            covered[lo:hi] += 1
            want_rows, want_mult = np.unique(idx[lo:hi], return_counts=True)
            assert 1 <= k <= 8 and rows[:k].tolist() == want_rows.tolist() and mult[:k].tolist() == want_mult.tolist(), (n, f, i)
        assert covered.min() == 1 and covered.max() == 1  # the blocks tile the image's rows


@pytest.mark.parametrize("f", SCALES)
@pytest.mark.parametrize("tiled,H,W", [(1, 32, 272), (1, 64, 96), (0, 45, 61), (0, 24, 48)])
def test_the_threads_of_a_window_keep_the_window_exactly_at_every_origin(lib, tiled, H, W, f):
    Hs, Ws = scaled_dims(H, W, f)
    count = np.zeros((Hs, Ws), dtype=np.int32)
    for h, w in ((1, 1), (5, 7), (Hs, Ws)):
        if h > Hs or w > Ws:
            continue
        for y0 in range(Hs - h + 1):
            for x0 in range(Ws - w + 1):
                count[:] = 0
                wgs = lib.lrf_test_scaled_wgs(tiled, f, y0, x0, h, w)
                assert lib.lrf_test_scaled_cover(tiled, f, Hs, Ws, y0, x0, h, w, wgs, count.ctypes.data) == 0, (h, w, y0, x0)
                window = count[y0:y0 + h, x0:x0 + w]
                assert window.min() == 1 and window.max() == 1 and int(count.sum()) == h * w, (h, w, y0, x0)


def test_a_window_of_more_than_256_patches_takes_several_workgroups(lib):
    # 512x768 at f = 2: 256x384 output pixels, 32 x 48 chroma patches of 8x8 outputs -> 6 workgroups; the window covers each once
    assert lib.lrf_test_scaled_wgs(1, 2, 0, 0, 256, 384) == 6 and lib.lrf_test_scaled_wgs(1, 8, 0, 0, 64, 96) == 6
    assert lib.lrf_test_scaled_wgs(1, 2, 7, 7, 2, 2) == 1 and lib.lrf_test_scaled_wgs(0, 2, 0, 0, 16, 17) == 2
    count = np.zeros((256, 384), dtype=np.int32)
    assert lib.lrf_test_scaled_cover(1, 2, 256, 384, 3, 5, 224, 224, lib.lrf_test_scaled_wgs(1, 2, 3, 5, 224, 224), count.ctypes.data) == 0
    assert int(count.sum()) == 224 * 224 and count[3:227, 5:229].min() == 1 and count.max() == 1


def plan(lib, images, items):
    im = np.ascontiguousarray([(t, c) + tuple(r) for t, c, r in images], dtype=np.int32).reshape(-1, 5)
    it = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 6)
    launches = np.zeros((MAX_LAUNCHES, 6), dtype=np.int64)
    table = np.full((len(it), 9), -7, dtype=np.int64)
    jobs = np.zeros((3 * len(im), 3), dtype=np.int64)
    n_jobs, pool, too_many = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    nl = lib.lrf_test_plan_decode_scaled(len(im), im.ctypes.data, len(it), it.ctypes.data, launches.ctypes.data, MAX_LAUNCHES, table.ctypes.data,
                                         jobs.ctypes.data, len(jobs), ctypes.byref(n_jobs), ctypes.byref(pool), ctypes.byref(too_many))
    assert nl >= 0
    L = [dict(zip(("tiled", "f", "cls", "item0", "nitems", "wgs"), (int(v) for v in launches[j]))) for j in range(nl)]
    return L, table, jobs[:n_jobs.value], pool.value, too_many.value


def pool_elems(ranks, f):
    return ranks[0] * (8 // f) ** 2 + (ranks[1] + ranks[2]) * (16 // f) ** 2


def check_plan(lib, images, items):
    L, table, jobs, pool, too_many = plan(lib, images, items)
    assert too_many == 0 and 1 <= len(L) <= MAX_LAUNCHES
    key_of = lambda e: (0, e[1], images[e[0]][1]) if images[e[0]][0] else (1, e[1], 0)  # (path, f, class): tiled first
    want = {}
    for j, e in enumerate(items):
        want.setdefault(key_of(e), []).append(tuple(e) + (j, 1000 * j))
    keys = [(0 if l["tiled"] else 1, l["f"], l["cls"]) for l in L]
    assert keys == sorted(want)  # one launch per group present, in the documented order
    at = 0
    for l, key in zip(L, keys):
        rows = [tuple(int(v) for v in row[:8]) for row in table[at:at + l["nitems"]]]
        assert l["item0"] == at and rows == want[key]  # call order inside the launch, place and out_off carried
        assert l["wgs"] == max(lib.lrf_test_scaled_wgs(int(key[0] == 0), *e[1:6]) for e in want[key])
        assert l["nitems"] * l["wgs"] < 2 ** 31
        at += l["nitems"]
    assert at == len(items) and sorted(int(v) for v in table[:, 6]) == list(range(len(items)))  # every item once
    # pooled tables: one per (image, f) among the tiled items, back to back, each item pointing at its own
    tiled_pairs = []
    for row in table:
        if images[int(row[0])][0] and (int(row[0]), int(row[1])) not in tiled_pairs:
            tiled_pairs.append((int(row[0]), int(row[1])))
    assert [(int(j[0]), int(j[1])) for j in jobs] == tiled_pairs
    off = 0
    where = {}
    for (i, f), j in zip(tiled_pairs, jobs):
        assert int(j[2]) == off
        where[(i, f)] = off
        off += pool_elems(images[i][2], f)
    assert pool == off
    for row in table:
        assert int(row[8]) == where.get((int(row[0]), int(row[1])), 0)
    return L


def test_grouping_and_launch_order(lib):
    images = [(1, 0, (7, 3, 3)), (0, 0, (7, 3, 3)), (1, 4, (26, 13, 13)), (1, 0, (5, 2, 4)), (0, 0, (64, 64, 64)), (1, 2, (12, 6, 6))]
    rng = np.random.default_rng(5)
    items = [(int(i), int(f), int(rng.integers(0, 3)), int(rng.integers(0, 3)), 5, 7) for i, f in zip(rng.integers(0, len(images), 300), rng.choice(SCALES, 300))]
    L = check_plan(lib, images, items)
    assert [(l["tiled"], l["f"], l["cls"]) for l in L] == [(1, f, c) for f in SCALES for c in (0, 2, 4)] + [(0, f, 0) for f in SCALES]


def test_whole_images_of_one_scale(lib):
    images = [(1, 0, (7, 3, 3))] * 3 + [(0, 0, (7, 3, 3))] + [(1, 4, (26, 13, 13))]
    sizes = [(512, 768), (16, 16), (64, 96), (45, 61), (32, 272)]
    for f in SCALES:
        items = [(i, f, 0, 0) + scaled_dims(H, W, f) for i, (H, W) in enumerate(sizes)]
        L = check_plan(lib, images, items)
        assert len(L) == 3 and L[0]["wgs"] == 6  # the largest image of the launch sets its grid


def test_at_most_eighteen_launches(lib):
    images = [(1, c, (7, 3, 3)) for c in range(5)] + [(0, 0, (7, 3, 3))]
    items = [(i, f, 0, 0, 1, 1) for i in range(len(images)) for f in SCALES] * 2
    assert len(check_plan(lib, images, items)) == MAX_LAUNCHES


def test_one_item_and_an_item_listed_twice(lib):
    for im in ((1, 3, (16, 9, 16)), (0, 0, (33, 4, 4))):
        L = check_plan(lib, [im], [(0, 4, 0, 0, 1, 1)])
        assert len(L) == 1 and L[0]["nitems"] == 1
    check_plan(lib, [(1, 0, (7, 3, 3)), (0, 0, (7, 3, 3))], [(0, 2, 3, 4, 5, 7), (1, 8, 0, 0, 2, 2), (0, 2, 3, 4, 5, 7)])


def test_a_launch_of_2_to_the_31_workgroups_is_refused(lib):
    L, table, jobs, pool, too_many = plan(lib, [(0, 0, (7, 3, 3))], [(0, 2, 0, 0, 2 ** 20, 2 ** 20)] * 3)
    assert too_many >= 2 ** 31 and L == [] and len(jobs) == 0
    big = (0, 8, 0, 0, 2 ** 20, 2 ** 20)  # tiled at f = 8: 2^19 x 2^19 patches = 2^30 workgroups
    L, table, jobs, pool, too_many = plan(lib, [(1, 0, (7, 3, 3))], [big, big])
    assert too_many == 2 ** 31 and L == []
    L, table, jobs, pool, too_many = plan(lib, [(1, 0, (7, 3, 3))], [big])
    assert too_many == 0 and len(L) == 1 and L[0]["nitems"] * L[0]["wgs"] == 2 ** 30
