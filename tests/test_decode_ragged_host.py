"""CPU suite: the host side of the ragged decode — what qmf_decode_ragged refuses before a GPU is asked for, and the ragged native
unpacker (lrf_pack_unpack_qmf_factors_ragged) against this package's Python container code on the reference's own streams."""
import numpy as np
import pytest

from conftest import Case

GOLDEN_MIX = ["tiny_q7", "tiny_r7", "tiny_q20", "odd_q7", "odd_r7", "nat_q7", "s2odd_q7"]  # mixed sizes and ranks


@pytest.fixture(scope="module")
def no_gpu(monkeypatch_module):
    """every refusal below must come before a context is asked for: asking for one fails the test"""
    from lrf_amd import _lib

    def refuse(device=None):
        raise AssertionError("a GPU context was asked for")
    monkeypatch_module.setattr(_lib, "context", refuse)


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def test_exported():
    import ctypes
    import os

    import lrf_amd
    from conftest import ROOT
    assert "qmf_decode_ragged" in lrf_amd.__all__ and callable(lrf_amd.qmf_decode_ragged)
    header = open(os.path.join(ROOT, "include", "lrf_pack_ragged.h")).read()
    assert "lrf_pack_unpack_qmf_factors_ragged(" in header and '#include "lrf_pack_ragged.h"' in open(os.path.join(ROOT, "include", "lrf_pack.h")).read()
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "lrf_amd", "liblrf_pack.so")), "lrf_pack_unpack_qmf_factors_ragged")


def test_empty_list_and_non_bytes_items_raise(no_gpu):
    from lrf_amd import qmf_decode_ragged
    good = Case("tiny_q7").encoded
    with pytest.raises(ValueError):
        qmf_decode_ragged([])
    with pytest.raises(ValueError):
        qmf_decode_ragged(good)  # a stream, not a list of streams
    with pytest.raises(TypeError):
        qmf_decode_ragged([good, "text"])
    with pytest.raises(TypeError):
        qmf_decode_ragged([good, None])
    with pytest.raises(TypeError):
        qmf_decode_ragged([np.frombuffer(good, dtype=np.uint8), good])


def test_streams_of_other_branches_raise_naming_the_branch(no_gpu):
    from lrf_amd import qmf_decode_ragged
    good = Case("tiny_q7").encoded
    for name, word in (("rgbsp_odd_q6", "RGB"), ("any_p16_q10", "patch size"), ("any_nopatch_q10", "patch=False")):
        with pytest.raises(NotImplementedError, match=word):
            qmf_decode_ragged([good, Case(name).encoded, good])


def test_crafted_streams_among_good_ones_are_rejected_before_any_kernel_runs(no_gpu):
    """the streams test_container_abi.py's test_crafted_streams_are_rejected_before_any_kernel_runs builds: rank 64 in the
    metadata over 2-column factors, a patch row missing, int16 factors"""
    from lrf_amd import qmf_decode_ragged
    from lrf_amd.codec import pack_image, parse_stream
    case = Case("tiny_q7")
    good = [case.encoded, Case("odd_r7").encoded, Case("tiny_q20").encoded]
    meta, fac = parse_stream(case.encoded)
    H, W = case.image.shape[-2:]
    lying = pack_image(fac, (H, W), [64, 64, 64], meta["bounds"], meta["patch size"], meta["dtype"])
    short = [f.copy() for f in fac]
    short[2] = short[2][:-1]
    short = pack_image(short, (H, W), meta["rank"], meta["bounds"], meta["patch size"], meta["dtype"])
    wide = pack_image([f.astype(np.int16) for f in fac], (H, W), meta["rank"], meta["bounds"], meta["patch size"], meta["dtype"])
    truncated = case.encoded[:-9]
    for bad in (lying, short, wide):
        for at in (0, 1, 3):
            with pytest.raises(ValueError, match="metadata describes"):
                qmf_decode_ragged(good[:at] + [bad] + good[at:])
    with pytest.raises(ValueError, match="metadata describes"):
        qmf_decode_ragged(good + [truncated])
    above = pack_image([np.zeros((f.shape[0], 65), dtype=np.int8) for f in fac], (H, W), [65, 65, 65], meta["bounds"], meta["patch size"], meta["dtype"])
    with pytest.raises(ValueError, match="above 64"):
        qmf_decode_ragged(good + [above])


def _layout(cases):
    """M, R, offsets of the streams back to back, and their factor payloads"""
    from lrf_amd import _lib
    from lrf_amd.container import separate_bytes
    Ms, Rs, uo, vo, blobs, u, v = [], [], [], [], [], 0, 0
    for c in cases:
        H, W = c.image.shape[-2:]
        M = [d[4] for d in _lib.plane_dims(H, W)]
        Ms.append(M)
        Rs.append(c.ranks)
        uo.append(u)
        vo.append(v)
        u += sum(m * r for m, r in zip(M, c.ranks))
        v += 64 * sum(c.ranks)
        blobs.append(separate_bytes(c.encoded, 2)[1])
    return blobs, Ms, Rs, uo, vo, u, v


@pytest.mark.parametrize("threads", [1, 5])
def test_ragged_unpacker_equals_the_python_parser(threads):
    from lrf_amd.codec import parse_stream, unpack_ragged_native
    cases = [Case(n) for n in GOLDEN_MIX]
    assert len({tuple(c.image.shape) for c in cases}) >= 3 and len({tuple(c.ranks) for c in cases}) >= 3
    blobs, Ms, Rs, uo, vo, ul, vl = _layout(cases)
    U, V, rc = unpack_ragged_native(blobs, Ms, Rs, uo, vo, ul, vl, threads=threads)
    assert rc == 0 and U.shape == (ul,) and V.shape == (vl,)
    for c, M, R, u, v in zip(cases, Ms, Rs, uo, vo):
        _, fac = parse_stream(c.encoded)
        for ch in range(3):
            assert fac[2 * ch].shape == (M[ch], R[ch])
            assert np.array_equal(U[u:u + M[ch] * R[ch]].reshape(M[ch], R[ch]), fac[2 * ch]), (c.name, ch)
            assert np.array_equal(V[v:v + 64 * R[ch]].reshape(64, R[ch]), fac[2 * ch + 1]), (c.name, ch)
            u += M[ch] * R[ch]
            v += 64 * R[ch]


def test_ragged_unpacker_refuses_what_is_not_the_layout():
    from lrf_amd.codec import unpack_ragged_native
    cases = [Case(n) for n in GOLDEN_MIX[:4]]
    blobs, Ms, Rs, uo, vo, ul, vl = _layout(cases)
    for at in (0, 2, 3):
        cut = list(blobs)
        cut[at] = cut[at][:-7]  # truncated
        assert unpack_ragged_native(cut, Ms, Rs, uo, vo, ul, vl)[2] == -6
        broken = bytearray(blobs[at])
        broken[len(broken) // 2] ^= 0x55  # corrupt deflate data, or a length field
        flipped = list(blobs)
        flipped[at] = bytes(broken)
        assert unpack_ragged_native(flipped, Ms, Rs, uo, vo, ul, vl)[2] == -6
    wrong_r = [list(r) for r in Rs]
    wrong_r[1][0] += 1  # another rank than the stream holds
    assert unpack_ragged_native(blobs, Ms, wrong_r, uo, vo, ul + 64 * 64, vl + 64)[2] == -6
    wrong_m = [list(m) for m in Ms]
    wrong_m[2][1] += 1  # another row count
    assert unpack_ragged_native(blobs, wrong_m, Rs, uo, vo, ul + 64 * 64, vl)[2] == -6
    # ranges that leave the buffers: refused as bad arguments, nothing written past them
    assert unpack_ragged_native(blobs, Ms, Rs, uo, vo, ul - 1, vl)[2] == -1
    assert unpack_ragged_native(blobs, Ms, Rs, uo, vo, ul, vl - 1)[2] == -1
    assert unpack_ragged_native(blobs, Ms, Rs, [-1] + uo[1:], vo, ul, vl)[2] == -1
    assert unpack_ragged_native(blobs, Ms, Rs, uo, vo[:-1] + [vl], ul, vl)[2] == -1


def test_factors_ragged_lays_the_streams_out_back_to_back():
    """the host half of qmf_decode_ragged: descriptors and flat factors, equal to the per-stream parser's"""
    from lrf_amd.codec import _factors_python, _factors_ragged
    cases = [Case(n) for n in GOLDEN_MIX]
    images, U, V = _factors_ragged([c.encoded for c in cases])
    for c, (H, W, ranks, u_off, v_off) in zip(cases, images):
        assert (H, W) == tuple(c.image.shape[-2:]) and ranks == c.ranks
        _, pu, pv = _factors_python([c.encoded])
        assert np.array_equal(U[u_off:u_off + pu.shape[1]], pu[0]) and np.array_equal(V[v_off:v_off + pv.shape[1]], pv[0])
    assert images[-1][3] + pu.shape[1] == U.size and images[-1][4] + pv.shape[1] == V.size
