"""CPU suite: the Huffman-only deflate coder of factor columns — the builder of lrf_amd/csrc/lrf_deflate_shared.h through a g++
shim, its host restatement lrf_pack_deflate_column_i8, and the stream assembly lrf_pack_qmf_streams_deflated (liblrf_pack.so)."""
import ctypes
import os
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import deflate_cases as dc
from conftest import ROOT, Case

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("deflate_shim") / "libdeflate_shim_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "deflate_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.shim_code_lengths.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def lengths(shim, freq, limit):
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.full(f.size, 99, dtype=np.uint8)
    assert shim.shim_code_lengths(f.ctypes.data, f.size, limit, out.ctypes.data) == 0
    return out


def fib(n):
    c = [1, 1]
    while len(c) < n:
        c.append(c[-1] + c[-2])
    return c[:n]


def builder_vectors():
    rng = np.random.default_rng(11)
    one = np.zeros(257, dtype=np.uint32)
    one[40] = 9
    two = np.zeros(257, dtype=np.uint32)
    two[[3, 256]] = [1000, 1]
    vs = [("one", one, 15), ("two", two, 15), ("equal257", np.full(257, 5), 15),
          ("fib18", np.array(fib(18) + [0] * 239), 15), ("fib10", np.array(fib(10) + [0] * 9), 7)]
    for i in range(12):
        n, limit = (257, 15) if i % 2 == 0 else (19, 7)
        f = rng.integers(0, [3, 50, 100000][i % 3], n) * (rng.random(n) < [0.2, 0.6, 1.0][(i // 3) % 3])
        vs.append((f"random{i}", f.astype(np.uint32), limit))
    skew = (2.0 ** np.arange(19)).astype(np.uint32)
    vs.append(("pow2_19", skew, 7))
    return vs


@pytest.mark.parametrize("name,freq,limit", builder_vectors(), ids=[v[0] for v in builder_vectors()])
def test_builder_lengths(shim, name, freq, limit):
    got = lengths(shim, freq, limit)
    used = np.asarray(freq) > 0
    assert (got[~used] == 0).all()
    assert (got[used] > 0).all() and (got <= limit).all()
    kraft = sum(Fraction(1, 2 ** int(l)) for l in got[used])
    assert kraft <= 1
    if used.sum() >= 2:
        assert kraft == 1
    if name == "fib18":  # unlimited Huffman depth is 17 here: the limit is what holds the lengths at 15
        assert got.max() == 15
    if name == "fib10":
        assert got.max() == 7


def test_tile_constant_is_the_headers(shim):
    assert shim.shim_tile() == dc.T


def check_stream(stream, col):
    assert zlib.decompress(stream) == col.tobytes()
    d = zlib.decompressobj()
    assert d.decompress(stream) == col.tobytes() and d.eof and d.unused_data == b""
    assert stream[:2] == b"\x78\x01"


@pytest.mark.parametrize("rows", dc.ROWS)
def test_column_round_trip(rows):
    for content in dc.CONTENTS:
        if content == "fib" and rows != 4180:
            continue
        col = dc.column(content, rows)
        streams = [dc.host_stream(col, stride) for stride in (1, 7, 32)]
        assert streams[0] == streams[1] == streams[2]
        check_stream(streams[0], col)
        assert len(streams[0]) <= dc.bound(rows)
        if content == "full" and rows >= 255:  # uniform over all of int8: nothing to gain, the stored form must win
            assert streams[0][2] & 6 == 0, "BTYPE 0 expected"
            assert len(streams[0]) == dc.bound(rows)
            if rows == 65537:
                assert streams[0][2] == 0 and streams[0][2 + 5 + 65535] == 1, "two stored blocks expected, the second one final"


def test_column_bad_arguments():
    lib = dc.pack_lib()
    col = dc.column("u32", 64)
    dst = np.full(200, 0xA5, dtype=np.uint8)
    assert lib.lrf_pack_deflate_column_i8(col.ctypes.data, 0, 1, dst.ctypes.data, 200) == -1
    assert lib.lrf_pack_deflate_column_i8(col.ctypes.data, 64, 0, dst.ctypes.data, 200) == -1
    assert lib.lrf_pack_deflate_column_i8(None, 64, 1, dst.ctypes.data, 200) == -1
    assert lib.lrf_pack_deflate_column_i8(col.ctypes.data, 64, 1, dst.ctypes.data, 10) == -7
    assert (dst == 0xA5).all()
    assert lib.lrf_pack_deflate_bound(0) == -1 and lib.lrf_pack_deflate_bound(65536) == 2 + 10 + 65536 + 4


def test_golden_columns_round_trip_and_size():
    """Every column of the golden factor sets round-trips, and over all of them the coder needs no more bytes than zlib level 9
    (zlib's own Huffman-only strategy reaches 0.935 of level 9 on these: a coder that loses that margin is mis-built)."""
    sets = dc.golden_factor_sets()
    assert len(sets) >= 30
    ours = z9 = 0
    for _, fac in sets:
        for f in fac:
            for j in range(f.shape[1]):
                col = np.ascontiguousarray(f[:, j])
                s = dc.host_stream(col)
                check_stream(s, col)
                ours += len(s)
                z9 += len(zlib.compress(col.tobytes(), 9))
    print(f"deflate restatement {ours} bytes, zlib-9 {z9} bytes, ratio {ours / z9:.4f} over {len(sets)} factor sets")
    assert ours <= z9


ASSEMBLY_CASES = ["nat_q7", "odd_q7", "tiny_rank1", "zero_q7"]


def assemble(cases, corrupt=None):
    """lrf_pack_qmf_streams_deflated over host-restated slots of the cases' reference factors, one ragged call"""
    from lrf_amd.codec import _pack_lib
    from lrf_amd.container import separate_bytes
    lib = _pack_lib()
    n = len(cases)
    metas = [bytes(separate_bytes(c.encoded, 2)[0]) for c in cases]
    M, R, chunks, col_off, col_len, at = [], [], [], [], [], 0
    for c in cases:
        fac = c.ref_factors()
        M += [fac[0].shape[0], fac[2].shape[0], fac[4].shape[0]]
        R += [fac[0].shape[1], fac[2].shape[1], fac[4].shape[1]]
        for f in fac:
            for j in range(f.shape[1]):
                s = dc.host_stream(np.ascontiguousarray(f[:, j]))
                slot = dc.bound(f.shape[0])
                chunks.append(s + b"\xA5" * (slot - len(s)))
                col_off.append(at)
                col_len.append(len(s))
                at += slot
    slots = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    col_off, col_len = np.array(col_off, dtype=np.int64), np.array(col_len, dtype=np.int32)
    slots_len = slots.size
    if corrupt == "length":
        col_len[-1] = slots.size - col_off[-1] + 1
    elif corrupt == "n":
        n = 0
    elif corrupt == "overlap":
        col_off[1] = col_off[0] + 1
    M, R = np.array(M, dtype=np.int64), np.array(R, dtype=np.int32)
    out = (ctypes.c_void_p * len(cases))(*[0xDEAD] * len(cases))
    out_len = (ctypes.c_int64 * len(cases))(*[-7] * len(cases))
    rc = lib.lrf_pack_qmf_streams_deflated(slots.ctypes.data, slots_len, n, M.ctypes.data, R.ctypes.data, col_off.ctypes.data, col_len.ctypes.data,
                                           col_off.size, (ctypes.c_char_p * len(cases))(*metas), np.array([len(m) for m in metas], dtype=np.int64).ctypes.data,
                                           2, out, out_len)
    if rc:
        assert [x for x in out] == [0xDEAD] * len(cases) and [x for x in out_len] == [-7] * len(cases), "an error must write nothing"
        return rc, None
    streams = []
    for b in range(len(cases)):
        streams.append(ctypes.string_at(out[b], out_len[b]))
        lib.lrf_pack_free(out[b])
    return 0, streams


def test_stream_assembly():
    from lrf_amd.container import bytes_to_dict, decode_matrix, decode_tensor, separate_bytes
    cases = [Case(n) for n in ASSEMBLY_CASES]
    rc, streams = assemble(cases)
    assert rc == 0
    for c, s in zip(cases, streams):
        meta, fac = separate_bytes(s, 2)
        assert bytes_to_dict(meta) == bytes_to_dict(separate_bytes(c.encoded, 2)[0])
        blobs = separate_bytes(fac, 6)
        for blob, ref in zip(blobs, c.ref_factors()):
            assert np.array_equal(decode_matrix(blob), ref)
            assert np.array_equal(decode_tensor(blob), ref)  # the generic reader of the container


@pytest.mark.parametrize("corrupt", ["length", "n", "overlap"])
def test_stream_assembly_refuses_corrupt_input(corrupt):
    rc, _ = assemble([Case(n) for n in ASSEMBLY_CASES], corrupt)
    assert rc == -6


def test_exports_are_declared_and_bound():
    from lrf_amd import _lib
    from lrf_amd.codec import _pack_lib
    hip = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    pack = open(os.path.join(ROOT, "include", "lrf_pack_deflate.h")).read()
    assert '#include "lrf_pack_deflate.h"' in open(os.path.join(ROOT, "include", "lrf_pack.h")).read()
    for name in ("lrf_deflate_bound", "lrf_deflate_columns_i8"):
        assert name + "(" in hip and name in _lib.EXPORTS
    assert "lrf_deflate_matrix" in hip and hasattr(_lib.Context, "deflate_columns")
    for name in ("lrf_pack_deflate_bound", "lrf_pack_deflate_column_i8", "lrf_pack_qmf_streams_deflated"):
        assert name + "(" in pack and hasattr(_pack_lib(), name)
    assert ctypes.CDLL(_lib.LIB_PATH).lrf_deflate_bound is not None
    assert [int(_lib.deflate_bound(n)) for n in (1, 65535, 65536)] == [dc.bound(n) for n in (1, 65535, 65536)]


@pytest.mark.parametrize("entry", ["qmf_encode_batch", "qmf_encode_ragged", "qmf_encode_target"])
def test_deflate_keyword_refusals_need_no_gpu(entry):
    import torch

    import lrf_amd
    img = torch.zeros((1, 3, 16, 16), dtype=torch.uint8)
    args = {"qmf_encode_batch": (img,), "qmf_encode_ragged": ([img[0]],), "qmf_encode_target": (img, 30.0)}[entry]
    kw = {} if entry == "qmf_encode_target" else {"quality": 7}
    with pytest.raises(ValueError):
        getattr(lrf_amd, entry)(*args, deflate="zlib", **kw)
    if entry == "qmf_encode_batch":
        with pytest.raises(NotImplementedError):
            lrf_amd.qmf_encode_batch(img, quality=7, patch=False, deflate="device")
        with pytest.raises(NotImplementedError):
            lrf_amd.qmf_encode_batch(img, quality=7, patch_size=(4, 4), deflate="device")
