"""CPU suite: the launches of a decode of windows (plan_decode_crops, lrf_amd/csrc/lrf_plan.cpp) and the functions of lrf_plan.h
that say which image pixels a thread of a crop kernel keeps (crop_tile_of, crop_quad_of: the kernels of
lrf_decode_crops_kernel.hip call the same functions).  Built here with g++ together with tests/decode_crops_plan_shim.cpp and
called through ctypes: no device.

  * the crops are grouped by their image's launch — the tiled body by rank-bound class, then rank <= 8, then the general kernel:
    at most seven — call order kept inside a group, every crop in exactly one launch with its place in the call as output index;
  * for every window of a set of geometries and sizes, at every origin, the pixel sets of the launch's workgroups are the
    window exactly: each pixel once, nothing outside."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
TILE16, STRIP, R8, ANY = range(4)
GEOMETRIES = [(24, 48), (32, 272), (40, 272), (45, 61), (173, 264)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("crops_plan") / "libcrops_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "decode_crops_plan_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_crop_wgs.restype = ctypes.c_long
    lib.lrf_test_crop_cover.restype = ctypes.c_long
    lib.lrf_test_crop_cover.argtypes = [ctypes.c_int] * 9 + [ctypes.c_long, ctypes.c_void_p]
    lib.lrf_test_plan_decode_crops.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def luma_pad(H, W):
    """(top, left) of the luma plane: reflect padding to multiples of 8, the smaller half first (lrf/compression/qmf.py:230-242)"""
    return (-H % 8) // 2, (-W % 8) // 2


def plan(lib, images, crops, size):
    kind = np.array([k for k, _ in images], dtype=np.int32)
    cls = np.array([c for _, c in images], dtype=np.int32)
    boxes = np.ascontiguousarray(crops, dtype=np.int32).reshape(-1, 3)
    launches = np.zeros((16, 5), dtype=np.int64)
    table = np.full((len(boxes), 4), -7, dtype=np.int32)
    too_many = ctypes.c_long()
    nl = lib.lrf_test_plan_decode_crops(len(images), kind.ctypes.data, cls.ctypes.data, len(boxes), boxes.ctypes.data, size[0], size[1],
                                        launches.ctypes.data, 16, table.ctypes.data, ctypes.byref(too_many))
    assert nl >= 0
    L = [dict(zip(("kind", "cls", "crop0", "ncrops", "wgs"), (int(v) for v in launches[j]))) for j in range(nl)]
    return L, table, too_many.value


def slot(image):
    kind, cls = image
    return (0, cls) if kind in (TILE16, STRIP) else (1 if kind == R8 else 2, 0)


def check_plan(lib, images, crops, size):
    L, table, too_many = plan(lib, images, crops, size)
    assert too_many == 0 and 1 <= len(L) <= 7
    want = {}
    for j, (i, y0, x0) in enumerate(crops):
        want.setdefault(slot(images[i]), []).append((i, y0, x0, j))
    keys = [(0, l["cls"]) if l["kind"] == STRIP else ((1, 0) if l["kind"] == R8 else (2, 0)) for l in L]
    assert keys == sorted(want)  # one launch per group present, in the documented order
    at = 0
    for l, key in zip(L, keys):
        assert l["kind"] in (STRIP, R8, ANY) and l["crop0"] == at and l["ncrops"] == len(want[key])
        assert l["wgs"] == lib.lrf_test_crop_wgs(int(l["kind"] == STRIP), size[0], size[1])
        assert [tuple(int(v) for v in row) for row in table[at:at + l["ncrops"]]] == want[key]  # call order inside the group
        at += l["ncrops"]
    assert at == len(crops) and sorted(int(v) for v in table[:, 3]) == list(range(len(crops)))  # every crop once
    return L


def test_grouping_and_launch_order(lib):
    images = [(TILE16, 0), (ANY, 0), (STRIP, 0), (R8, 0), (STRIP, 4), (TILE16, 4), (TILE16, 2)]
    rng = np.random.default_rng(3)
    crops = [(int(i), int(rng.integers(0, 9)), int(rng.integers(0, 9))) for i in rng.integers(0, len(images), 200)]
    L = check_plan(lib, images, crops, (9, 13))
    assert [(l["kind"], l["cls"]) for l in L] == [(STRIP, 0), (STRIP, 2), (STRIP, 4), (R8, 0), (ANY, 0)]
    # TILE16 and STRIP images of one class share the tiled launch of that class
    assert L[0]["ncrops"] == sum(1 for i, _, _ in crops if i in (0, 2))


def test_at_most_seven_launches(lib):
    images = [(STRIP, c) for c in range(5)] + [(TILE16, c) for c in range(5)] + [(R8, 0), (ANY, 0)]
    crops = [(i, 1, 2) for i in range(len(images))] * 2
    L = check_plan(lib, images, crops, (16, 16))
    assert len(L) == 7


def test_one_crop_and_a_crop_listed_twice(lib):
    for im in ((TILE16, 3), (STRIP, 1), (R8, 0), (ANY, 0)):
        L = check_plan(lib, [im], [(0, 0, 0)], (1, 1))
        assert len(L) == 1 and L[0]["ncrops"] == 1
    check_plan(lib, [(STRIP, 0), (ANY, 0)], [(0, 3, 4), (1, 0, 0), (0, 3, 4)], (7, 5))


def test_workgroups_per_window_are_the_worst_case_over_alignments(lib):
    assert lib.lrf_test_crop_wgs(1, 1, 1) == 1 and lib.lrf_test_crop_wgs(1, 2, 2) == 2  # rows 15, 16 of the padded plane: two strips
    assert lib.lrf_test_crop_wgs(1, 224, 224) == 15      # 15 strips x one group of 29 <= 32 patches
    assert lib.lrf_test_crop_wgs(1, 16, 250) == 2 * 2    # up to 33 patches: two groups
    assert lib.lrf_test_crop_wgs(0, 224, 224) == 49 and lib.lrf_test_crop_wgs(0, 9, 13) == 1


def test_a_launch_of_2_to_the_31_workgroups_is_refused(lib):
    L, table, too_many = plan(lib, [(ANY, 0)], [(0, 0, 0)] * 3, (2 ** 20, 2 ** 20))
    assert too_many >= 2 ** 31 and L == []


@pytest.mark.parametrize("H,W", GEOMETRIES)
@pytest.mark.parametrize("tiled", [1, 0])
def test_the_threads_of_a_window_keep_the_window_exactly_at_every_origin(lib, H, W, tiled):
    top, left = luma_pad(H, W)
    count = np.zeros((H, W), dtype=np.int32)
    for h, w in ((1, 1), (9, 13), (16, 16), (H, W)):
        wgs = lib.lrf_test_crop_wgs(tiled, h, w)
        for y0 in range(H - h + 1):
            for x0 in range(W - w + 1):
                count[:] = 0
                assert lib.lrf_test_crop_cover(tiled, H, W, top, left, y0, x0, h, w, wgs, count.ctypes.data) == 0, (h, w, y0, x0)
                window = count[y0:y0 + h, x0:x0 + w]
                assert window.min() == 1 and window.max() == 1 and int(count.sum()) == h * w, (h, w, y0, x0)
