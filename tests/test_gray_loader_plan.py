"""CPU suite: the image list, the thread maps and the launch plans of the gray loader (describe_gray_images, plan_gray_windows,
plan_gray_resized in lrf_amd/csrc/lrf_plan.cpp; gray_tile_of and crop_quad_of of lrf_plan.h, which the kernels of
lrf_gray_loader_kernel.hip call too).  Built here with g++ together with tests/gray_loader_plan_shim.cpp and called through
ctypes: no device.

  * describe_gray_images refuses, term by term and in its documented order, what the kernels could not index safely, and
    describes the padding lrf_chan_dims gives;
  * the windows are grouped by level (at most 4 launches), the boxes by (path, level) with the staged path first (at most 8),
    call order kept inside a launch, every item in exactly one launch with its place in the call, a launch as wide as its
    largest item needs; 2^31 workgroups are refused;
  * for every origin of a set of window sizes on four geometries at levels 1, 2, 4, 8 the pixels the threads keep are the window
    exactly: each once, nothing outside."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from resized_decode import resized_level
from tensor_format import boxes_of, staged

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
OK, SIZE, GEOM, RANK, NEGATIVE, U, V, OUT = range(8)  # GDESC_* (lrf_plan.h)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gray_plan") / "libgray_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "gray_loader_plan_shim.cpp")])
    lib = ctypes.CDLL(so)
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.lrf_test_describe_gray.argtypes = [l, p, l, l, i, l, p, p]
    lib.lrf_test_gray_window_cover.restype = l
    lib.lrf_test_gray_window_cover.argtypes = [i] * 5
    lib.lrf_test_gray_window_wgs.restype = l
    lib.lrf_test_gray_window_wgs.argtypes = [i] * 7
    lib.lrf_test_plan_gray_windows.argtypes = [i, p, l, p, p, i, p, p]
    lib.lrf_test_plan_gray_resized.argtypes = [l, p, i, i, p, i, p, p]
    return lib


def describe(lib, images, u_len, v_len, scale=0, out_len=0):
    im = np.ascontiguousarray(images, dtype=np.int64).reshape(-1, 6)
    who, descs = np.zeros(1, np.int64), np.zeros((im.shape[0], 8), np.int64)
    rc = lib.lrf_test_describe_gray(im.shape[0], im.ctypes.data, u_len, v_len, scale, out_len, who.ctypes.data, descs.ctypes.data)
    return rc, int(who[0]), descs


def test_describe_gives_the_padding_of_the_geometry(lib):
    rc, _, d = describe(lib, [(37, 53, 7, 5, 9, 0), (64, 96, 64, 0, 0, 0), (8, 8, 1, 0, 0, 0), (173, 264, 9, 100, 200, 0)], 10 ** 6, 10 ** 6)
    assert rc == OK
    assert d.tolist() == [[5, 9, 37, 53, 7, 1, 1, 7], [0, 0, 64, 96, 64, 0, 0, 12], [0, 0, 8, 8, 1, 0, 0, 1], [100, 200, 173, 264, 9, 1, 0, 33]]


def test_describe_refuses_term_by_term(lib):
    good = (37, 53, 7, 0, 0, 0)  # M = 35: U 245 elements, V 448
    assert describe(lib, [good], 245, 448)[0] == OK
    cases = [((0, 53, 7, 0, 0, 0), SIZE), ((37, 0, 7, 0, 0, 0), SIZE), ((2 ** 20 + 1, 8, 7, 0, 0, 0), SIZE), ((8, 2 ** 20 + 1, 7, 0, 0, 0), SIZE),
             ((2 ** 16, 2 ** 15, 7, 0, 0, 0), SIZE),  # 2^31 pixels
             ((3, 53, 7, 0, 0, 0), GEOM), ((37, 2, 7, 0, 0, 0), GEOM),  # reflect padding of 5 and 6 on sides of 3 and 2
             ((37, 53, 0, 0, 0, 0), RANK), ((37, 53, 65, 0, 0, 0), RANK), ((37, 53, 7, -1, 0, 0), NEGATIVE), ((37, 53, 7, 0, -1, 0), NEGATIVE)]
    for im, want in cases:
        rc, who, _ = describe(lib, [good, im], 10 ** 6, 10 ** 6)
        assert (rc, who) == (want, 1), (im, rc)
    assert describe(lib, [good], 244, 448)[0] == U and describe(lib, [(37, 53, 7, 1, 0, 0)], 245, 448)[0] == U
    assert describe(lib, [good], 245, 447)[0] == V and describe(lib, [(37, 53, 7, 0, 1, 0)], 245, 448)[0] == V
    assert describe(lib, [(37, 53, 7, 2 ** 62, 0, 0)], 2 ** 62 + 10, 448)[0] == U  # (no sum wraps)
    # the order: the size before the rank before the offsets before the extents
    assert describe(lib, [(0, 53, 0, -1, 0, 0)], 0, 0)[0] == SIZE and describe(lib, [(37, 53, 0, -1, 0, 0)], 0, 0)[0] == RANK
    assert describe(lib, [(37, 53, 7, -1, 0, 0)], 0, 0)[0] == NEGATIVE and describe(lib, [good], 0, 0)[0] == U
    # the output of the whole-image entry: [Hs][Ws] at out_off, per level; a negative out_off only counts there
    for scale, px in ((1, 37 * 53), (2, 19 * 27), (4, 10 * 14), (8, 5 * 7)):
        assert describe(lib, [(37, 53, 7, 0, 0, 3)], 245, 448, scale, px + 3)[0] == OK
        assert describe(lib, [(37, 53, 7, 0, 0, 3)], 245, 448, scale, px + 2)[0] == OUT
        assert describe(lib, [(37, 53, 7, 0, 0, -1)], 245, 448, scale, 10 ** 6)[0] == NEGATIVE
    assert describe(lib, [(37, 53, 7, 0, 0, -1)], 245, 448)[0] == OK


def plan_windows(lib, sizes, items, max_launches=4):
    sz, it = np.ascontiguousarray(sizes, dtype=np.int64), np.ascontiguousarray(items, dtype=np.int64).reshape(-1, 8)
    launches, table, too_many = np.zeros((max_launches, 5), np.int64), np.zeros((it.shape[0], 10), np.int64), np.zeros(1, np.int64)
    n = lib.lrf_test_plan_gray_windows(len(sizes), sz.ctypes.data, it.shape[0], it.ctypes.data, launches.ctypes.data, max_launches, table.ctypes.data,
                                       too_many.ctypes.data)
    return n, launches[:max(n, 0)], table, int(too_many[0])


def test_windows_are_grouped_by_level(lib):
    sizes = [(64, 96), (37, 53), (173, 264)]
    rng = np.random.default_rng(3)
    items = []
    for j in range(200):
        im, f = int(rng.integers(0, 3)), int(rng.choice([1, 2, 4, 8]))
        Hs, Ws = -(-sizes[im][0] // f), -(-sizes[im][1] // f)
        h, w = int(rng.integers(1, Hs + 1)), int(rng.integers(1, Ws + 1))
        items.append((im, f, int(rng.integers(0, Hs - h + 1)), int(rng.integers(0, Ws - w + 1)), h, w, 1000 * j, w + j))
    n, launches, table, too_many = plan_windows(lib, sizes, items)
    assert n == 4 and too_many == 0 and launches[:, 0].tolist() == [1, 2, 4, 8] and not launches[:, 1].any()
    assert sorted(table[:, 7].tolist()) == list(range(200))  # every item once
    at = 0
    for f, _, item0, nitems, wgs in launches.tolist():
        assert item0 == at
        rows = table[item0:item0 + nitems]
        assert (rows[:, 1] == f).all() and (np.diff(rows[:, 7]) > 0).all()  # its level, call order kept
        need = [lib.lrf_test_gray_window_wgs(*sizes[r[0]], f, *r[2:6].tolist()) for r in rows]
        assert wgs == max(need) and min(need) >= 1
        at += nitems
    assert at == 200
    for row in table.tolist():  # the item itself travels unchanged
        src = items[row[7]]
        assert tuple(row[:6]) == src[:6] and row[6] == 0 and tuple(row[8:]) == src[6:]
    n, launches, _, _ = plan_windows(lib, sizes, [it for it in items if it[1] in (2, 8)])
    assert n == 2 and launches[:, 0].tolist() == [2, 8]
    # 2^31 workgroups in one launch are refused and no table is built: 2^20 windows of 1024 rows of 513 pixel quads, 2052 workgroups each
    big = [(0, 8, 0, 0, 1024, 2049, 0, 1)] * 4
    n, _, _, too_many = plan_windows(lib, [(8 * 1024, 8 * 2049)], big * 2 ** 18)
    assert n == 0 and too_many == 2 ** 20 * 2052


def plan_resized(lib, boxes, size, max_launches=8):
    b = np.ascontiguousarray(boxes, dtype=np.int64).reshape(-1, 6)
    launches, table, too_many = np.zeros((max_launches, 5), np.int64), np.zeros((b.shape[0], 10), np.int64), np.zeros(1, np.int64)
    n = lib.lrf_test_plan_gray_resized(b.shape[0], b.ctypes.data, size[0], size[1], launches.ctypes.data, max_launches, table.ctypes.data, too_many.ctypes.data)
    return n, launches[:max(n, 0)], table, int(too_many[0])


@pytest.mark.parametrize("size", [(5, 7), (17, 33), (224, 224)])
def test_boxes_are_grouped_by_path_and_level(lib, size):
    oh, ow = size
    geoms = [(173, 264), (64, 96), (512, 768), (40, 4000)]
    boxes = [(im, y0, x0, hb, wb, (j + im) & 1) for im, (H, W) in enumerate(geoms) for j, (y0, x0, hb, wb) in enumerate(boxes_of(H, W, size, 11 + im))]
    n, launches, table, too_many = plan_resized(lib, boxes, size)
    assert 1 <= n <= 8 and too_many == 0
    keys = [(int(d), int(f)) for f, d, *_ in launches.tolist()]
    assert keys == sorted(keys) and len(set(keys)) == n  # staged first, then by level
    assert {d for d, _ in keys} == {0, 1} or size == (224, 224)  # both paths occur
    assert sorted(table[:, 7].tolist()) == list(range(len(boxes)))
    at = 0
    for f, direct, item0, nitems, wgs in launches.tolist():
        assert item0 == at
        rows = table[item0:item0 + nitems]
        assert (np.diff(rows[:, 7]) > 0).all()
        for r in rows.tolist():
            im, y0, x0, hb, wb, flip = boxes[r[7]]
            assert r[:8] == [im, resized_level(hb, wb, oh, ow), y0, x0, hb, wb, flip, r[7]] and r[1] == f
            assert direct == (0 if staged(hb, wb, oh, ow) else 1)
            assert r[8:] == [r[7] * oh * ow, ow]  # box j is [oh][ow] at oh ow j
        assert wgs == (-(-oh * ow // 256) if direct else -(-oh // 16) * -(-ow // 64))
        at += nitems
    assert at == len(boxes)


WINDOWS = [(1, 1), (3, 5), (16, 16), (13, 37), (8, 8), (9, 17)]


@pytest.mark.parametrize("geom", [(16, 24), (37, 53), (40, 272), (173, 264)])
@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_the_threads_keep_every_window_exactly_at_every_origin(lib, geom, f):
    H, W = geom
    Hs, Ws = -(-H // f), -(-W // f)
    checked = 0
    for h, w in WINDOWS + [(Hs, Ws), (Hs, 1), (1, Ws), (Hs - 1, Ws - 1)]:
        if h < 1 or w < 1 or h > Hs or w > Ws:
            continue
        got = lib.lrf_test_gray_window_cover(H, W, f, h, w)
        assert got == (Hs - h + 1) * (Ws - w + 1), (geom, f, h, w, got)
        checked += got
    assert checked > 0
