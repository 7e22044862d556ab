"""CPU suite: lrf_pack_deflate_size_column_i8 (liblrf_pack.so), the host restatement of what lrf_deflate_sizes_i8 counts on the
device — the length of a column's stream from its byte counts alone — against the length of the stream the coder writes."""
import ctypes
import os
import re

import numpy as np
import pytest

import deflate_cases as dc
from conftest import ROOT


def size_fn():
    lib = dc.pack_lib()
    lib.lrf_pack_deflate_size_column_i8.restype = ctypes.c_int64
    lib.lrf_pack_deflate_size_column_i8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    return lib.lrf_pack_deflate_size_column_i8


def host_size(col, stride=1):
    col = np.asarray(col, dtype=np.int8)
    src = np.full((col.size, stride), 77, dtype=np.int8)
    src[:, 0] = col
    return size_fn()(src.ctypes.data, col.size, stride)


def btype(stream):
    """BTYPE of the first block of a zlib stream: 0 stored, 1 fixed, 2 dynamic"""
    return (stream[2] >> 1) & 3


@pytest.mark.parametrize("rows", dc.ROWS)
def test_size_equals_the_stream_length(rows):
    for content in dc.CONTENTS:
        if (rows, content) not in dc.pairs():
            continue
        col = dc.column(content, rows)
        want = len(dc.host_stream(col))
        assert host_size(col, 1) == want, (rows, content)
        assert host_size(col, 5) == want, (rows, content)


def test_size_of_every_golden_column():
    sets = dc.golden_factor_sets()
    assert len(sets) >= 30
    n = 0
    for name, fac in sets:
        for f in fac:
            f = np.ascontiguousarray(f)
            for j in range(f.shape[1]):
                # (the column where it lies in its row-major matrix: stride = the number of columns)
                got = size_fn()(f.ctypes.data + j, f.shape[0], f.shape[1])
                assert got == len(dc.host_stream(f[:, j])), (name, f.shape, j)
                n += 1
    assert n > 1000


def test_all_three_forms_and_the_length_limit():
    """the corpus holds columns of every block form, each sized right; the Fibonacci column (17 symbols and the end-of-block
    symbol: an unconstrained Huffman code deeper than the 15 bits deflate allows) goes through the length-limit fix-up"""
    seen = {}
    for rows, content in dc.pairs():
        col = dc.column(content, rows)
        s = dc.host_stream(col)
        assert host_size(col) == len(s)
        seen.setdefault(btype(s), (rows, content))
    tiny = np.array([3], dtype=np.int8)  # (a column of one byte: nothing beats the fixed block's 3 + 8 + 7 bits)
    s = dc.host_stream(tiny)
    assert host_size(tiny) == len(s)
    seen.setdefault(btype(s), (1, "tiny"))
    assert set(seen) == {0, 1, 2}, seen
    fib = dc.fibonacci_column()
    s = dc.host_stream(fib)
    assert btype(s) == 2 and host_size(fib) == len(s) and host_size(fib, 5) == len(s)


def test_bad_arguments():
    f = size_fn()
    col = dc.column("u32", 64)
    assert f(None, 64, 1) < 0
    assert f(col.ctypes.data, 0, 1) < 0
    assert f(col.ctypes.data, -3, 1) < 0
    assert f(col.ctypes.data, (1 << 30) + 1, 1) < 0
    assert f(col.ctypes.data, 64, 0) < 0
    assert f(col.ctypes.data, 64, 1) == len(dc.host_stream(col))


def test_declared_bound_and_grouped_as_the_header_says():
    from lrf_amd import _lib
    hip = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    pack = open(os.path.join(ROOT, "include", "lrf_pack_deflate.h")).read()
    assert "lrf_pack_deflate_size_column_i8(" in pack
    assert "lrf_deflate_sizes_i8(" in hip and "lrf_deflate_sizes_i8" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "lrf_deflate_sizes_i8")
    assert hasattr(_lib.Context, "deflate_sizes") and hasattr(_lib.Context, "deflate_sizes_into")
    cg = int(re.search(r"#define\s+LRF_DEFLATE_CG\s+(\d+)", hip).group(1))
    assert _lib.LRF_DEFLATE_CG == cg and cg >= 8


def test_binding_refuses_before_any_library_call():
    """deflate_sizes_into checks types and shapes first: a context whose library raises on any use shows that nothing was called"""
    import torch

    from lrf_amd import _lib

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached ({name})")

    ctx = object.__new__(_lib.Context)
    ctx._lib, ctx._h, ctx.device = Untouchable(), None, 0
    table = np.array([[0, 64, 3, 0, 0]], dtype=np.int64)
    src, lens = torch.zeros(192, dtype=torch.int8), torch.zeros(3, dtype=torch.int32)
    for bad_src, bad_lens in ((src.to(torch.uint8), lens), (src, lens.to(torch.int64)), (src.numpy(), lens), (src, None)):
        with pytest.raises(TypeError):
            ctx.deflate_sizes_into(bad_src, table, bad_lens)
    for bad_src, bad_lens in ((src.reshape(64, 3), lens), (src, lens.reshape(1, 3)), (torch.zeros(384, dtype=torch.int8)[::2], lens),
                              (src, lens)):  # (the last pair: flat and of the right types, but not on the context's device)
        with pytest.raises(ValueError):
            ctx.deflate_sizes_into(bad_src, table, bad_lens)
