"""CPU suite: the definition of the decode at 1/2, 1/4, 1/8 scale (tests/scaled_decode.py) against block-averaging the oracle's
full decode, its nearest-neighbour index against the oracle's up-sampling, the sizes, what check_scaled_args and
qmf_decode_scaled refuse before a GPU is asked for, and how the crop functions split a list with per-crop scales between the
two kernel calls (the calls stubbed)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import QMF_CASES, Case
from scaled_decode import SCALES, block_average_u8, nearest_idx, reference_scaled, scaled_dims

RANKS = (7, 3, 3)
GEOMETRIES = [(16, 16), (32, 272), (64, 96), (24, 48), (40, 272), (45, 61), (173, 264), (2, 2), (9, 7)]


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


def _two_images():
    """64x96 and 45x61 at (7,3,3), zero factors on the host"""
    from lrf_amd import _lib
    images, uo, vo = [], 0, 0
    for H, W in ((64, 96), (45, 61)):
        images.append((H, W, RANKS, uo, vo))
        uo += sum(d[4] * r for d, r in zip(_lib.plane_dims(H, W), RANKS))
        vo += 64 * sum(RANKS)
    return torch.zeros(uo, dtype=torch.int8), torch.zeros(vo, dtype=torch.int8), images


def test_exported():
    import os

    import lrf_amd
    from conftest import ROOT
    from lrf_amd import _lib
    assert "qmf_decode_scaled" in lrf_amd.__all__ and callable(lrf_amd.qmf_decode_scaled)
    header = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    for name in ("lrf_scaled_dims", "lrf_qmf_decode_scaled_rgb_u8", "lrf_qmf_decode_scaled_crops_rgb_u8"):
        assert name in _lib.EXPORTS and name + "(" in header


@pytest.mark.parametrize("name", QMF_CASES)
def test_reference_against_the_block_averaged_full_decode(oracle, name):
    """the definition pools before the colour conversion, a caller of the full decoder after its truncation and clamp: half a
    level of truncation bias, and more than one level only where the full decoder clamped (the reference alone: 0.33, 0.35 %)"""
    c = Case(name)
    f6 = c.ref_factors()
    H, W = c.image.shape[-2:]
    full = oracle.planes_to_rgb(f6[0::2], f6[1::2], H, W)
    for f in SCALES:
        ref = reference_scaled(f6, H, W, f, oracle)
        assert ref.dtype == np.uint8 and ref.shape == (3,) + scaled_dims(H, W, f)
        d = np.abs(ref.astype(np.float64) - block_average_u8(full, f))
        print(f"{name} f={f}: mean |d| {d.mean():.4f}, more than one level away {100 * (d > 1).mean():.4f} %")
        assert d.mean() <= 0.5, (name, f, d.mean())
        assert (d > 1).mean() <= 0.01, (name, f, (d > 1).mean())


@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_nearest_idx_is_the_oracles_upsampling(oracle, H, W):
    hc, wc = H // 2, W // 2
    ramp = np.arange(hc * wc, dtype=np.float32).reshape(hc, wc)
    up = np.empty((H, W), dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    oracle.lib().lrf_oracle_nearest_upsample(ramp.ctypes.data_as(fp), ctypes.c_long(hc), ctypes.c_long(wc), ctypes.c_long(H), ctypes.c_long(W),
                                             up.ctypes.data_as(fp))
    iy, ix = nearest_idx(H, hc), nearest_idx(W, wc)
    assert np.array_equal(up, ramp[iy][:, ix])


def test_scaled_dims_and_scaled_sizes():
    from lrf_amd import _lib
    from lrf_amd.codec import ResidentFactors
    lib = _lib.load()
    for H, W in GEOMETRIES + [(1365, 2048), (2 ** 31 - 1, 1)]:
        for f in SCALES:
            hs, ws = ctypes.c_int64(), ctypes.c_int64()
            assert lib.lrf_scaled_dims(H, W, f, ctypes.byref(hs), ctypes.byref(ws)) == 0
            assert (hs.value, ws.value) == (-(-H // f), -(-W // f)) == _lib.scaled_dims(H, W, f) == scaled_dims(H, W, f)
    hs, ws = ctypes.c_int64(-5), ctypes.c_int64(-5)
    for H, W, f in ((64, 96, 1), (64, 96, 3), (64, 96, 16), (64, 96, 0), (64, 96, -2), (0, 96, 2), (64, -1, 2), (2 ** 31, 4, 2)):
        assert lib.lrf_scaled_dims(H, W, f, ctypes.byref(hs), ctypes.byref(ws)) == -1 and (hs.value, ws.value) == (-5, -5)
    assert lib.lrf_scaled_dims(64, 96, 2, None, ctypes.byref(ws)) == -1 and lib.lrf_scaled_dims(64, 96, 2, ctypes.byref(hs), None) == -1
    for f in (1, 3, 16, 0, True, 2.5):
        with pytest.raises(ValueError):
            _lib.scaled_dims(64, 96, f)
    U, V, images = _two_images()
    res = ResidentFactors(None, U, V, images)
    assert res.scaled_sizes(1) == res.sizes == [(64, 96), (45, 61)]
    assert res.scaled_sizes(2) == [(32, 48), (23, 31)] and res.scaled_sizes(4) == [(16, 24), (12, 16)] and res.scaled_sizes(8) == [(8, 12), (6, 8)]
    with pytest.raises(ValueError):
        res.scaled_sizes(3)


def test_good_arguments_come_back():
    from lrf_amd._lib import check_scaled_args
    U, V, images = _two_images()
    for f in SCALES:
        ims, scale = check_scaled_args(U, V, images, f)
        assert scale == f and type(scale) is int and len(ims) == 2
    assert check_scaled_args(U, V, images, np.int64(4))[1] == 4
    # the far corners: 64x96 at 1/2 is 32x48, 45x61 at 1/8 is 6x8
    ims, boxes, size = check_scaled_args(U, V, images, crops=[(0, 2, 0, 0), (0, 2, 27, 41), (1, 8, 1, 1)], size=(5, 7))
    assert boxes.dtype == np.int32 and boxes.tolist() == [[0, 2, 0, 0], [0, 2, 27, 41], [1, 8, 1, 1]] and size == (5, 7) and len(ims) == 2
    assert check_scaled_args(U, V, images, crops=torch.tensor([[1, 4, 0, 0]]), size=(12, 16))[1].tolist() == [[1, 4, 0, 0]]  # the whole scaled image


@pytest.mark.parametrize("kw", [
    dict(scale=1), dict(scale=3), dict(scale=16), dict(scale=0), dict(scale=-2),
    dict(crops=[(0, 2, 28, 0)], size=(5, 7)),       # 28 + 5 > 32
    dict(crops=[(0, 2, 0, 42)], size=(5, 7)),       # 42 + 7 > 48
    dict(crops=[(0, 2, 0, 0), (1, 8, 2, 0)], size=(5, 7)),  # 2 + 5 > 6
    dict(crops=[(0, 4, 0, 0)], size=(17, 7)),       # taller than the scaled image (16x24)
    dict(crops=[(1, 2, 0, 0)], size=(5, 32)),       # wider than it (23x31)
    dict(crops=[(0, 2, -1, 0)], size=(5, 7)), dict(crops=[(0, 2, 0, -1)], size=(5, 7)),
    dict(crops=[(2, 2, 0, 0)], size=(5, 7)), dict(crops=[(-1, 2, 0, 0)], size=(5, 7)),
    dict(crops=[(0, 1, 0, 0)], size=(5, 7)), dict(crops=[(0, 3, 0, 0)], size=(5, 7)), dict(crops=[(0, 16, 0, 0)], size=(1, 1)),
    dict(crops=[], size=(5, 7)), dict(crops=np.zeros((0, 4), dtype=np.int32), size=(5, 7)),
    dict(crops=[(0, 2, 0, 0)], size=(0, 7)), dict(crops=[(0, 2, 0, 0)], size=(5, -2)), dict(crops=[(0, 2, 0, 0)], size=(5,)),
    dict(crops=[(0, 0, 0)], size=(5, 7)),           # not [n, 4]
    dict(crops=[0, 2, 0, 0], size=(5, 7)),
    dict(crops=[(0, 2, 2 ** 40, 0)], size=(5, 7)),  # no wrap on the way to int32
    dict(crops=[(0, 2, 0, 0)]), dict(size=(5, 7)), dict(scale=2, crops=[(0, 2, 0, 0)], size=(5, 7)),
])
def test_check_scaled_args_raises_value_error(kw):
    from lrf_amd._lib import check_scaled_args
    U, V, images = _two_images()
    with pytest.raises(ValueError):
        check_scaled_args(U, V, images, **kw)


@pytest.mark.parametrize("kw", [
    dict(scale=2.0), dict(scale=True), dict(scale="2"), dict(scale=None),
    dict(crops=[(0.0, 2.0, 0.0, 0.0)], size=(5, 7)), dict(crops=np.zeros((2, 4), dtype=np.float32), size=(5, 7)), dict(crops=torch.zeros((2, 4)), size=(5, 7)),
    dict(crops=[(0, 2, 0, 0)], size=(5.0, 7)), dict(crops=[(0, 2, 0, 0)], size=(True, 7)),
])
def test_check_scaled_args_raises_type_error(kw):
    from lrf_amd._lib import check_scaled_args
    U, V, images = _two_images()
    with pytest.raises(TypeError):
        check_scaled_args(U, V, images, **kw)


def test_factors_are_checked_as_the_ragged_decode_checks_them():
    from lrf_amd._lib import check_scaled_args
    U, V, images = _two_images()
    with pytest.raises(TypeError):
        check_scaled_args(U.float(), V, images, 2)
    with pytest.raises(ValueError):
        check_scaled_args(U[:-1], V, images, 2)
    with pytest.raises(ValueError):
        check_scaled_args(U, V, [(64, 96, (7, 3, 65), 0, 0)], 2)
    with pytest.raises(ValueError):
        check_scaled_args(U, V, [], 2)


class StubContext:
    """records the two kernel calls and answers with tensors that name the call and the box"""

    def __init__(self):
        self.calls = []

    def decode_crops(self, U, V, images, crops, size):
        b = np.asarray(crops)
        self.calls.append(("full", b.tolist(), size))
        return torch.stack([torch.full((3,) + tuple(size), 10 + j, dtype=torch.uint8) for j in range(len(b))])

    def decode_scaled_crops(self, U, V, images, crops, size):
        b = np.asarray(crops)
        self.calls.append(("scaled", b.tolist(), size))
        return torch.stack([torch.full((3,) + tuple(size), 100 + j, dtype=torch.uint8) for j in range(len(b))])


def test_per_crop_scales_are_split_between_the_two_calls_and_merged_in_call_order():
    from lrf_amd.codec import ResidentFactors, qmf_decode_crops
    U, V, images = _two_images()
    ctx = StubContext()
    res = ResidentFactors(ctx, U, V, images)
    crops = [(0, 1, 2), (1, 0, 0), (0, 3, 4), (0, 5, 6), (1, 1, 1), (0, 0, 0)]
    got = res.decode_crops(crops, (2, 3), scale=[1, 8, 2, 1, 4, 2])
    assert ctx.calls == [("full", [[0, 1, 2], [0, 5, 6]], (2, 3)), ("scaled", [[1, 8, 0, 0], [0, 2, 3, 4], [1, 4, 1, 1], [0, 2, 0, 0]], (2, 3))]
    assert tuple(got.shape) == (6, 3, 2, 3) and got[:, 0, 0, 0].tolist() == [10, 100, 101, 11, 102, 103]
    ctx.calls.clear()
    assert res.decode_crops(crops, (2, 3))[:, 0, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]  # the default: the existing call, untouched
    assert res.decode_crops(crops, (2, 3), scale=1)[:, 0, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]
    assert [c[0] for c in ctx.calls] == ["full", "full"] and ctx.calls[0][1] == [list(c) for c in crops]
    ctx.calls.clear()
    assert res.decode_crops(crops, (2, 3), scale=4)[:, 0, 0, 0].tolist() == [100, 101, 102, 103, 104, 105]  # one scale for all
    assert ctx.calls == [("scaled", [[i, 4, y, x] for i, y, x in crops], (2, 3))]
    ctx.calls.clear()
    assert qmf_decode_crops(res, crops, (2, 3), scale=np.array([1, 1, 1, 1, 1, 1]))[:, 0, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]
    assert [c[0] for c in ctx.calls] == ["full"]
    ctx.calls.clear()
    # refusals come before either call: a window inside the image but outside its scaled size, a scale per crop too few, 3, floats
    for bad, exc in (([1, 8, 2, 1, 4, 8], ValueError), ([1, 2, 4], ValueError), ([1, 8, 2, 1, 4, 3], ValueError), (2.0, TypeError), ([1.0] * 6, TypeError),
                     (True, TypeError)):
        with pytest.raises(exc):
            res.decode_crops(crops[:5] + [(0, 7, 0)], (2, 3), scale=bad)
    with pytest.raises(ValueError):
        res.decode_crops([(0, 63, 0)], (2, 3), scale=[1])  # the full-scale part is checked as before
    assert ctx.calls == []


def test_qmf_decode_scaled_refuses_before_a_gpu_is_asked_for(no_gpu):
    from lrf_amd import qmf_decode_crops, qmf_decode_scaled
    tiny, odd = Case("tiny_q7"), Case("odd_q7")
    streams = [tiny.encoded, odd.encoded]
    for scale in (1, 3, 16, 0):
        with pytest.raises(ValueError):
            qmf_decode_scaled(streams, scale)
    for scale in (2.0, "2", None, True):
        with pytest.raises(TypeError):
            qmf_decode_scaled(streams, scale)
    with pytest.raises(ValueError):
        qmf_decode_scaled([], 2)
    with pytest.raises(ValueError):
        qmf_decode_scaled(streams, 2, inflate="gpu")
    with pytest.raises(ValueError):
        qmf_decode_crops(streams, [(0, 30, 0)], (4, 4), scale=2)  # 64x96 at 1/2 is 32x48
    with pytest.raises(ValueError):
        qmf_decode_crops(streams, [(0, 0, 0)], (4, 4), scale=[3])


def test_streams_of_other_branches_raise_naming_the_branch(no_gpu):
    from lrf_amd import qmf_decode_scaled
    good = Case("tiny_q7").encoded
    for name, word in (("rgbsp_odd_q6", "RGB"), ("any_p16_q10", "patch size"), ("any_nopatch_q10", "patch=False")):
        with pytest.raises(NotImplementedError, match=word):
            qmf_decode_scaled([good, Case(name).encoded], 2)


class OnDevice:
    """stands for a CUDA tensor of boxes: the refusal must come before its values are asked for"""
    is_cuda = True

    def detach(self):
        raise AssertionError("the boxes were read")


# one bad input per check of check_scaled_args, in the order of the checks, with the text it raises
MESSAGES = [
    (dict(scale=2.0), TypeError, 'scale must be an integer, got 2.0'),
    (dict(scale=3), ValueError, 'scale 3: 2, 4 or 8 expected'),
    (dict(scale=2, crops=[(0, 2, 0, 0)], size=(4, 4)), ValueError, 'give either a scale (whole images) or crops of (image, scale, y0, x0) and a size'),
    (dict(crops=[(0, 2, 0, 0)], size=4), ValueError, 'size must be (h, w), got 4'),
    (dict(crops=[(0, 2, 0, 0)], size=(4.0, 4)), TypeError, 'size must hold two integers, got (4.0, 4)'),
    (dict(crops=[(0, 2, 0, 0)], size=(4, 0)), ValueError, 'crop size 4x0: both sides must be >= 1'),
    (dict(crops=OnDevice(), size=(4, 4)), ValueError, 'crops live on the host: the call validates every box before it launches'),
    (dict(crops=[], size=(4, 4)), ValueError, 'decode_scaled_crops needs 1 to 2^20 crops'),
    (dict(crops=[(0.0, 2.0, 0.0, 0.0)], size=(4, 4)), TypeError, 'crops must be integers (image, scale, y0, x0), got float64'),
    (dict(crops=[(0, 0, 0)], size=(4, 4)), ValueError, 'crops must be [n, 4] (image, scale, y0, x0), got shape (1, 3)'),
    (dict(crops=np.zeros((2 ** 20 + 1, 4), dtype=np.int8), size=(4, 4)), ValueError, 'decode_scaled_crops needs 1 to 2^20 crops'),
    (dict(crops=[(0, 2, 0, 0), (-1, 2, 0, 0)], size=(4, 4)), ValueError, 'crop 1: image -1 out of range [0, 2)'),
    (dict(crops=[(0, 2, 0, 0), (1, 3, 0, 0)], size=(4, 4)), ValueError, 'crop 1: scale 3: 2, 4 or 8 expected'),
    (dict(crops=[(0, 2, 0, 0), (1, 4, 9, 0)], size=(4, 4)), ValueError, 'crop 1: 4x4 at (9, 0) leaves image 1 of 12x16 at scale 1/4'),
]


@pytest.mark.parametrize("case", range(len(MESSAGES)))
def test_check_scaled_args_messages(case):
    from lrf_amd._lib import check_scaled_args
    kw, kind, text = MESSAGES[case]
    U, V, images = _two_images()
    with pytest.raises(kind) as e:
        check_scaled_args(U, V, images, **kw)
    assert type(e.value) is kind and str(e.value) == text
