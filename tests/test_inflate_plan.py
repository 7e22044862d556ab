"""CPU suite: plan_inflate (lrf_amd/csrc/lrf_plan.cpp), which says which lane of lrf_inflate_columns_i8's launch decodes which
column.  Built here with g++ together with tests/inflate_plan_shim.cpp and called through ctypes: no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("inflate_plan") / "libinflate_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "inflate_plan_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_plan_inflate.restype = ctypes.c_long
    lib.lrf_test_plan_inflate.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    return lib


def plan(lib, mats):
    rows = np.array([m[0] for m in mats], dtype=np.int64)
    cols = np.array([m[1] for m in mats], dtype=np.int32)
    total = int(cols.sum())
    slots = np.full((total + 1, 2), -7, dtype=np.int32)
    n = lib.lrf_test_plan_inflate(len(mats), rows.ctypes.data, cols.ctypes.data, slots.ctypes.data, total + 1)
    assert n == total and (slots[total] == -7).all()
    return [tuple(int(v) for v in s) for s in slots[:total]]


def image_mats(images):
    """the six matrices (rows, cols) per image of (M triple, R triple), in the container's order"""
    return [m for M, R in images for c in range(3) for m in ((M[c], R[c]), (64, R[c]))]


CALLS = [image_mats([((6144, 1536, 1536), (7, 3, 3))] * 5), image_mats([((6144, 1536, 1536), (26, 13, 13)), ((713, 187, 187), (9, 2, 64)), ((1, 1, 1), (1, 1, 1))]),
         [(64, 1)], [(5, 130), (5, 65), (9, 64), (9, 3)], [(100, 4096), (100, 4096), (7, 1)]]


@pytest.mark.parametrize("mats", CALLS)
def test_every_column_once_adjacent_columns_in_adjacent_lanes_long_columns_first(lib, mats):
    slots = plan(lib, mats)
    assert sorted(slots) == [(i, j) for i, (_, cols) in enumerate(mats) for j in range(cols)]  # each column exactly once
    at = 0
    order = []
    while at < len(slots):  # a matrix's columns are consecutive slots, ascending: lanes l, l + 1 hold adjacent bytes of every row
        i, cols = slots[at][0], mats[slots[at][0]][1]
        assert slots[at:at + cols] == [(i, j) for j in range(cols)]
        order.append(i)
        at += cols
    keys = [(-mats[i][0], -mats[i][1], i) for i in order]
    assert keys == sorted(keys)  # by rows, longest first; ties: more columns first, then call order
    # a wave (64 consecutive slots) mixes row counts only where two groups meet: at most (number of distinct rows - 1) waves do
    mixed = sum(len({mats[i][0] for i, _ in slots[w:w + 64]}) > 1 for w in range(0, len(slots), 64))
    assert mixed <= len({r for r, _ in mats}) - 1


def test_the_plan_does_not_depend_on_the_order_of_the_call(lib):
    mats = CALLS[1]
    base = [(mats[i], j) for i, j in plan(lib, mats)]
    rng = np.random.default_rng(3)
    for _ in range(5):
        perm = [int(p) for p in rng.permutation(len(mats))]
        shuffled = [mats[p] for p in perm]
        got = [(shuffled[i], j) for i, j in plan(lib, shuffled)]
        assert got == base  # the same (rows, cols, column) sequence: only matrices equal in rows and cols may trade places
        slots = plan(lib, shuffled)
        firsts = [i for i, j in slots if j == 0]
        for a, b in zip(firsts, firsts[1:]):
            if shuffled[a] == shuffled[b]:
                assert a < b  # the tie rule: call order
