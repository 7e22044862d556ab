"""CPU suite: the host side of the ragged encode — the ragged native packer (lrf_pack_qmf_streams_ragged) against this package's
Python container code, and what qmf_encode_ragged refuses before a GPU is asked for."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

# seven images of mixed sizes and rank triples (sizes: the bodies of tests/test_encode_ragged_plan.py)
ITEMS = [((32, 272), (7, 3, 3)), ((40, 272), (12, 6, 6)), ((45, 61), (1, 1, 1)), ((64, 96), (26, 13, 13)), ((24, 48), (16, 9, 16)),
         ((173, 264), (8, 8, 5)), ((64, 96), (32, 16, 16))]
BOUNDS = (-16, 15)


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def no_gpu(monkeypatch_module):
    """every refusal below must come before a context is asked for: asking for one fails the test"""
    from lrf_amd import _lib

    def refuse(device=None):
        raise AssertionError("a GPU context was asked for")
    monkeypatch_module.setattr(_lib, "context", refuse)


def _factors(seed=3, gap=5):
    """random int8 factors of ITEMS in two flat buffers, `gap` unused elements between images -> (U, V, u_off, v_off)"""
    from lrf_amd import _lib
    rng = np.random.default_rng(seed)
    u_off, v_off, uo, vo = [], [], gap, 0
    for hw, t in ITEMS:
        u_off.append(uo)
        v_off.append(vo)
        uo += sum(d[4] * r for d, r in zip(_lib.plane_dims(*hw), t)) + gap
        vo += 64 * sum(t) + gap
    return rng.integers(-16, 16, uo, dtype=np.int8), rng.integers(-16, 16, vo, dtype=np.int8), u_off, v_off


def test_exported():
    import lrf_amd
    assert "qmf_encode_ragged" in lrf_amd.__all__ and callable(lrf_amd.qmf_encode_ragged)
    assert "lrf_pack_qmf_streams_ragged(" in open(os.path.join(ROOT, "include", "lrf_pack_ragged.h")).read()
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "lrf_amd", "liblrf_pack.so")), "lrf_pack_qmf_streams_ragged")
    assert "lrf_qmf_encode_ragged_rgb_u8(" in open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    from lrf_amd import _lib
    assert "lrf_qmf_encode_ragged_rgb_u8" in _lib.EXPORTS and hasattr(_lib.Context, "encode_ragged")


@pytest.mark.parametrize("threads", [1, 4])
def test_ragged_packer_equals_pack_image_per_image(threads):
    from lrf_amd import _lib
    from lrf_amd.codec import pack_image, pack_streams_ragged_native, split_factors
    U, V, u_off, v_off = _factors()
    sizes, triples = [hw for hw, _ in ITEMS], [list(t) for _, t in ITEMS]
    streams, rc = pack_streams_ragged_native(U, V, sizes, triples, u_off, v_off, BOUNDS, threads=threads)
    assert rc == 0 and len(streams) == len(ITEMS)
    for s, hw, t, uo, vo in zip(streams, sizes, triples, u_off, v_off):
        nu, nv = sum(d[4] * r for d, r in zip(_lib.plane_dims(*hw), t)), 64 * sum(t)
        assert s == pack_image(split_factors(U[uo:uo + nu], V[vo:vo + nv], hw, t), hw, t, BOUNDS), (hw, t)


def test_ragged_packer_streams_unpack_to_the_factors():
    """and the ragged unpacker reads them back: the two ends of the container agree"""
    from lrf_amd import _lib
    from lrf_amd.codec import pack_streams_ragged_native, unpack_ragged_native
    from lrf_amd.container import separate_bytes
    U, V, u_off, v_off = _factors(seed=4, gap=0)
    sizes, triples = [hw for hw, _ in ITEMS], [list(t) for _, t in ITEMS]
    streams, rc = pack_streams_ragged_native(U, V, sizes, triples, u_off, v_off, BOUNDS, threads=2)
    assert rc == 0
    Ms = [[d[4] for d in _lib.plane_dims(*hw)] for hw in sizes]
    U2, V2, rc = unpack_ragged_native([separate_bytes(s, 2)[1] for s in streams], Ms, triples, u_off, v_off, U.size, V.size)
    assert rc == 0 and np.array_equal(U2, U) and np.array_equal(V2, V)


def test_ragged_packer_refuses_what_is_inconsistent():
    """straight at the C entry: every inconsistency is -6 and no stream is handed out"""
    from lrf_amd import _lib
    from lrf_amd.codec import _pack_lib
    lib = _pack_lib()
    U, V, u_off, v_off = _factors(gap=0)
    n = len(ITEMS)
    Ms = [[d[4] for d in _lib.plane_dims(*hw)] for hw, _ in ITEMS]
    Rs = [list(t) for _, t in ITEMS]
    meta = [b"{}"] * n

    def call(n=n, Ms=Ms, Rs=Rs, u_off=u_off, v_off=v_off, u_len=U.size, v_len=V.size):
        k = max(n, 1)
        out, lens = (ctypes.c_void_p * k)(), (ctypes.c_int64 * k)()
        rc = lib.lrf_pack_qmf_streams_ragged(
            U.ctypes.data_as(ctypes.c_void_p), u_len, V.ctypes.data_as(ctypes.c_void_p), v_len, n,
            (ctypes.c_int64 * (3 * k))(*[m for M in Ms for m in M][:3 * k]), (ctypes.c_int * (3 * k))(*[r for R in Rs for r in R][:3 * k]),
            (ctypes.c_int64 * k)(*u_off[:k]), (ctypes.c_int64 * k)(*v_off[:k]), (ctypes.c_char_p * k)(*meta[:k]),
            (ctypes.c_int64 * k)(*[len(m) for m in meta[:k]]), 2, out, lens)
        if rc == 0:
            for b in range(n):
                lib.lrf_pack_free(out[b])
        else:
            assert all(not out[b] for b in range(k))
        return rc

    assert call() == 0
    big_m = [list(m) for m in Ms]
    big_m[3][0] = 2 ** 62  # M x R would wrap
    wrong_r = [list(r) for r in Rs]
    wrong_r[-1][0] += 1  # the last image then needs more than the buffer holds
    refused = {
        "U one element short": call(u_len=U.size - 1),
        "V one element short": call(v_len=V.size - 1),
        "a rank the buffer has no room for": call(Rs=wrong_r),
        "u offset past the end": call(u_off=u_off[:-1] + [U.size]),
        "v offset past the end": call(v_off=v_off[:-1] + [V.size - 1]),
        "negative offset": call(u_off=[-1] + u_off[1:]),
        "M x R overflow": call(Ms=big_m),
        "M = 0": call(Ms=[[0, 1, 1]] + Ms[1:]),
        "R = 0": call(Rs=[[7, 0, 3]] + Rs[1:]),
        "n = 0": call(n=0),
        "n = -1": call(n=-1),
    }
    assert all(rc == -6 for rc in refused.values()), refused


def _images():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for (H, W), _ in ITEMS[:3]]


def test_argument_errors_raise_before_a_gpu_is_asked_for(no_gpu):
    from lrf_amd import qmf_encode_ragged
    ims = _images()
    for kw in (dict(rank=[7, 5]), dict(quality=[7, 5, 3, 1]), dict(ranks=[(7, 3, 3), (7, 3, 3)]), dict(rank=7, init_sign=[None, None])):
        with pytest.raises(ValueError, match="one per image"):
            qmf_encode_ragged(ims, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        qmf_encode_ragged(ims)
    with pytest.raises(ValueError, match="exactly one"):
        qmf_encode_ragged(ims, rank=7, quality=7)
    with pytest.raises(ValueError, match="init_sign holds"):
        qmf_encode_ragged(ims, rank=7, init_sign=np.ones(12, dtype=np.int8))
    with pytest.raises(ValueError):
        qmf_encode_ragged([], rank=7)
    with pytest.raises(ValueError):
        qmf_encode_ragged(ims + [ims[0][0]], rank=7)  # [H,W], not [3,H,W]
    with pytest.raises(ValueError, match=">= 1"):
        qmf_encode_ragged(ims, ranks=(7, 0, 3))
    with pytest.raises(NotImplementedError, match="uint8"):
        qmf_encode_ragged(ims[:2] + [ims[2].float()], rank=7)
    with pytest.raises(TypeError):
        qmf_encode_ragged(ims[:2] + [ims[2].numpy()], rank=7)
    with pytest.raises(NotImplementedError, match="num_iters"):
        qmf_encode_ragged(ims, rank=7, num_iters=0)


def test_per_image_parameters_go_through_qmf_ranks(no_gpu):
    from lrf_amd import qmf_ranks
    from lrf_amd.codec import _check_encode_ragged_args
    ims = _images()
    sizes, triples, signs = _check_encode_ragged_args(ims, None, [7, 20, 3], None, 10, None)
    assert sizes == [hw for hw, _ in ITEMS[:3]] and triples == [qmf_ranks(hw, quality=q) for hw, q in zip(sizes, (7, 20, 3))] and signs == [None] * 3
    assert _check_encode_ragged_args(ims, 7, None, None, 10, None)[1] == [[7, 3, 3]] * 3
    assert _check_encode_ragged_args(ims, [7, 1, 12], None, None, 10, None)[1] == [[7, 3, 3], [1, 1, 1], [12, 6, 6]]
    assert _check_encode_ragged_args(ims, None, None, (8, 8, 5), 10, None)[1] == [[8, 8, 5]] * 3
    assert _check_encode_ragged_args(ims, None, None, [(8, 8, 5), (1, 2, 3), (4, 4, 4)], 10, None)[1] == [[8, 8, 5], [1, 2, 3], [4, 4, 4]]
    one = np.array([1, -1, 1, 1, -1], dtype=np.int8)
    signs = _check_encode_ragged_args(ims, None, None, (3, 1, 1), 10, one)[2]
    assert all(np.array_equal(s, one) for s in signs)
    signs = _check_encode_ragged_args(ims, None, None, (3, 1, 1), 10, [one, None, -one])[2]
    assert np.array_equal(signs[0], one) and signs[1] is None and np.array_equal(signs[2], -one)


def test_context_encode_ragged_checks_its_arguments_without_a_device():
    from lrf_amd._lib import check_encode_ragged_args
    rgb = torch.zeros(3 * 64 * 96 + 16, dtype=torch.uint8)
    assert check_encode_ragged_args(rgb, [(64, 96, (7, 3, 3), 16)]) == [(64, 96, [7, 3, 3], 16, -1)]
    for bad in ([(64, 96, (7, 3, 3), 17)], [(64, 96, (7, 3, 3), -1)], [(64, 96, (33, 3, 3), 0)], [(64, 96, (7, 0, 3), 0)], [],
                [(64, 96, (7, 3, 3), 0, 0)], [(64, 96, (7, 3), 0)], [(0, 96, (7, 3, 3), 0)]):
        with pytest.raises(ValueError):
            check_encode_ragged_args(rgb, bad)
    sign = torch.ones(13, dtype=torch.int8)
    assert check_encode_ragged_args(rgb, [(64, 96, (7, 3, 3), 0, 0)], sign)[0][4] == 0
    with pytest.raises(ValueError):
        check_encode_ragged_args(rgb, [(64, 96, (7, 3, 3), 0, 1)], sign)
    with pytest.raises(TypeError):
        check_encode_ragged_args(rgb.float(), [(64, 96, (7, 3, 3), 0)])
    with pytest.raises(TypeError):
        check_encode_ragged_args(rgb, [(64, 96, (7, 3, 3), 0, 0)], sign.float())
