"""CPU suite: the definition of the resized crops (tests/resized_decode.py) — its two identities with the plain and the scaled
crop, its distance from real-valued bilinear interpolation — what check_resized_args and qmf_decode_resized_crops refuse before
a GPU is asked for, and the exports."""
import numpy as np
import pytest
import torch

from conftest import Case
from resized_decode import float_bilinear, reference_resized, resized_level

RANKS = (7, 3, 3)


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
    """64x96 and 32x48 at (7,3,3), zero factors on the host: the sizes of the golden streams tiny_q7 and zero_q7"""
    from lrf_amd import _lib
    images, uo, vo = [], 0, 0
    for H, W in ((64, 96), (32, 48)):
        images.append((H, W, RANKS, uo, vo))
        uo += sum(d[4] * r for d, r in zip(_lib.plane_dims(H, W), RANKS))
        vo += 64 * sum(RANKS)
    return torch.zeros(uo, dtype=torch.int8), torch.zeros(vo, dtype=torch.int8), images


def test_exported():
    import os

    import lrf_amd
    from conftest import ROOT
    from lrf_amd import _lib
    assert "qmf_decode_resized_crops" in lrf_amd.__all__ and callable(lrf_amd.qmf_decode_resized_crops)
    assert callable(lrf_amd.ResidentFactors.decode_resized_crops) and callable(_lib.Context.decode_resized_crops) and callable(_lib.check_resized_args)
    header = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    assert "lrf_qmf_decode_resized_crops_rgb_u8" in _lib.EXPORTS and "lrf_qmf_decode_resized_crops_rgb_u8(" in header and "} lrf_resized_crop;" in header
    assert "torchvision" in lrf_amd.qmf_decode_resized_crops.__doc__  # the docstring says whose bytes these are not


@pytest.mark.parametrize("H,W", [(64, 96), (45, 61)])
def test_the_two_identities_at_every_origin(H, W):
    """a box of the output's size is the plain crop; a box of f x the output at an origin that is a multiple of f is the crop of
    the level at (y0 / f, x0 / f): every origin, byte for byte (the level images are random bytes: the identities are the taps')"""
    oh, ow = 5, 7
    rng = np.random.default_rng(H * 1000 + W)
    for f in (1, 2, 4, 8):
        Hs, Ws = -(-H // f), -(-W // f)
        L = rng.integers(0, 256, (3, Hs, Ws), dtype=np.uint8)
        hb, wb = f * oh, f * ow
        if hb > H or wb > W:
            continue
        assert resized_level(hb, wb, oh, ow) == f
        n = 0
        for y in range(0, H - hb + 1, f):
            for x in range(0, W - wb + 1, f):
                for flip in (False, True):
                    want = L[:, y // f:y // f + oh, x // f:x // f + ow]
                    got = reference_resized(L, (y, x, hb, wb), (oh, ow), flip)
                    assert np.array_equal(got, want[:, :, ::-1] if flip else want), (f, y, x, flip)
                n += 1
        assert n == ((H - hb) // f + 1) * ((W - wb) // f + 1)


@pytest.mark.parametrize("binary", [False, True], ids=["random", "0_255"])
def test_within_two_and_a_half_levels_of_real_valued_bilinear(binary):
    """the tap position is floored to 1/256 per axis (under one level each), the rounding adds half a level: 2.5"""
    rng = np.random.default_rng(7 + binary)
    worst = 0.0
    for k in range(600):
        H, W = int(rng.integers(9, 300)), int(rng.integers(9, 300))
        oh, ow = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        hb, wb = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        y0, x0 = int(rng.integers(0, H - hb + 1)), int(rng.integers(0, W - wb + 1))
        f = resized_level(hb, wb, oh, ow)
        Hs, Ws = -(-H // f), -(-W // f)
        L = (rng.integers(0, 2, (3, Hs, Ws)) * 255).astype(np.uint8) if binary else rng.integers(0, 256, (3, Hs, Ws), dtype=np.uint8)
        box = (y0, x0, hb, wb)
        d = float(np.abs(reference_resized(L, box, (oh, ow)).astype(np.float64) - float_bilinear(L, box, (oh, ow))).max())
        worst = max(worst, d)
        assert d <= 2.5, (k, H, W, box, oh, ow, d)
    print("largest distance from float64 bilinear:", worst)


def test_good_arguments_come_back():
    from lrf_amd import _lib
    from lrf_amd.codec import _resized_boxes
    U, V, images = _two_images()
    rows = _resized_boxes([(0, 0, 0, 64, 96), (1, 31, 47, 1, 1), (1, 3, 4, 20, 30)], [False, True, False])
    ims, boxes, size = _lib.check_resized_args(U, V, images, rows, (5, 7))
    assert boxes.dtype == np.int32 and boxes.tolist() == [[0, 0, 0, 64, 96, 0], [1, 31, 47, 1, 1, 1], [1, 3, 4, 20, 30, 0]] and size == (5, 7)
    assert boxes.flags.c_contiguous and len(ims) == 2
    assert _resized_boxes(np.array([(0, 0, 0, 1, 1)]), True)[:, 5].tolist() == [1] and _resized_boxes(torch.tensor([(0, 0, 0, 1, 1)]), None)[:, 5].tolist() == [0]
    assert _lib.check_resized_args(U, V, images, [(0, 0, 0, 1, 1, 7)], (16384, 1))[1][0, 5] == 1  # flip: any value but 0


BAD_VALUE = {
    "box past the bottom": dict(boxes=[(0, 1, 0, 64, 96)]), "box past the right": dict(boxes=[(1, 0, 20, 32, 30)]),
    "negative y0": dict(boxes=[(0, -1, 0, 5, 5)]), "negative x0": dict(boxes=[(0, 0, -1, 5, 5)]),
    "taller than the image": dict(boxes=[(1, 0, 0, 33, 48)]), "h = 0": dict(boxes=[(0, 0, 0, 0, 5)]), "w = 0": dict(boxes=[(0, 0, 0, 5, 0)]),
    "h < 0": dict(boxes=[(0, 5, 5, -2, 5)]), "image 2": dict(boxes=[(2, 0, 0, 5, 5)]), "image -1": dict(boxes=[(-1, 0, 0, 5, 5)]),
    "no boxes": dict(boxes=np.zeros((0, 5), np.int64)), "four columns": dict(boxes=[(0, 0, 0, 5)]), "one box, flat": dict(boxes=(0, 0, 0, 5, 5)),
    "flip of the wrong length": dict(flip=[True]), "flip of the wrong rank": dict(flip=[[True, False]]),
    "size 0": dict(size=(0, 7)), "size (5, 0)": dict(size=(5, 0)), "negative size": dict(size=(-5, 7)), "size past 16384": dict(size=(16385, 7)),
    "size of three": dict(size=(5, 7, 1)), "size not a pair": dict(size=5),
}
BAD_TYPE = {
    "float boxes": dict(boxes=[(0.0, 0.0, 0.0, 5.0, 5.0)]), "float size": dict(size=(5.0, 7)), "bool size": dict(size=(True, 7)),
    "flip as integers": dict(flip=[0, 1]), "flip as a string": dict(flip="yes"),
}
GOOD = dict(boxes=[(0, 0, 0, 64, 96), (1, 3, 4, 20, 30)], size=(5, 7), flip=[False, True])


def _checked(kw):
    from lrf_amd import _lib
    from lrf_amd.codec import _resized_boxes
    U, V, images = _two_images()
    a = dict(GOOD, **kw)
    return _lib.check_resized_args(U, V, images, _resized_boxes(a["boxes"], a["flip"]), a["size"])


@pytest.mark.parametrize("why", sorted(BAD_VALUE))
def test_check_resized_args_raises_value_error(why):
    _checked({})
    with pytest.raises(ValueError):
        _checked(BAD_VALUE[why])


@pytest.mark.parametrize("why", sorted(BAD_TYPE))
def test_check_resized_args_raises_type_error(why):
    with pytest.raises(TypeError):
        _checked(BAD_TYPE[why])


def test_check_resized_args_itself_refuses_rows_that_are_not_six_integers():
    from lrf_amd import _lib
    U, V, images = _two_images()
    with pytest.raises(ValueError):
        _lib.check_resized_args(U, V, images, [(0, 0, 0, 5, 5)], (5, 7))
    with pytest.raises(TypeError):
        _lib.check_resized_args(U, V, images, [(0, 0, 0, 5, 5, 0.5)], (5, 7))
    with pytest.raises(TypeError):
        _lib.check_resized_args(U.float(), V, images, [(0, 0, 0, 5, 5, 0)], (5, 7))
    with pytest.raises(ValueError):
        _lib.check_resized_args(U[:-1], V, images, [(0, 0, 0, 5, 5, 0)], (5, 7))


@pytest.mark.parametrize("why", sorted(BAD_VALUE) + sorted(BAD_TYPE))
def test_qmf_decode_resized_crops_refuses_before_a_gpu_is_asked_for(no_gpu, why):
    from lrf_amd import qmf_decode_resized_crops
    streams = [Case("tiny_q7").encoded, Case("zero_q7").encoded]
    sizes = [tuple(Case(n).image.shape[-2:]) for n in ("tiny_q7", "zero_q7")]
    assert sizes == [(64, 96), (32, 48)]  # the boxes above are written for these
    a = dict(GOOD, **(BAD_VALUE[why] if why in BAD_VALUE else BAD_TYPE[why]))
    with pytest.raises(ValueError if why in BAD_VALUE else TypeError):
        qmf_decode_resized_crops(streams, a["boxes"], a["size"], a["flip"])


def test_other_refusals_before_a_gpu_is_asked_for(no_gpu):
    from lrf_amd import qmf_decode_resized_crops
    streams = [Case("tiny_q7").encoded, Case("zero_q7").encoded]
    with pytest.raises(ValueError):
        qmf_decode_resized_crops([], GOOD["boxes"], GOOD["size"])
    with pytest.raises(ValueError):
        qmf_decode_resized_crops(streams, GOOD["boxes"], GOOD["size"], inflate="gpu")
    with pytest.raises(AssertionError, match="a GPU context was asked for"):
        qmf_decode_resized_crops(streams, GOOD["boxes"], GOOD["size"], GOOD["flip"])  # and good arguments do reach the GPU


def test_streams_of_other_branches_raise_naming_the_branch(no_gpu):
    from lrf_amd import qmf_decode_resized_crops
    good = Case("tiny_q7").encoded
    for name, word in (("rgbsp_odd_q6", "RGB"), ("any_p16_q10", "patch size"), ("any_nopatch_q10", "patch=False")):
        with pytest.raises(NotImplementedError, match=word):
            qmf_decode_resized_crops([good, Case(name).encoded], [(0, 0, 0, 5, 5)], (5, 7))


class OnDevice:
    """stands for a CUDA tensor of boxes: the refusal must come before its values are asked for"""
    is_cuda = True

    def detach(self):
        raise AssertionError("the boxes were read")


# one bad input per check of check_resized_args, in the order of the checks, with the text it raises
MESSAGES = [
    ([(0, 0, 0, 8, 8, 0)], 9, ValueError, 'size must be (oh, ow), got 9'),
    ([(0, 0, 0, 8, 8, 0)], (9, True), TypeError, 'size must hold two integers, got (9, True)'),
    ([(0, 0, 0, 8, 8, 0)], (9, 16385), ValueError, 'output size 9x16385: both sides must be in [1, 16384]'),
    (OnDevice(), (9, 13), ValueError, 'crops live on the host: the call validates every box before it launches'),
    ([], (9, 13), ValueError, 'decode_resized_crops needs 1 to 2^20 crops'),
    (np.zeros((1, 6), dtype=np.float32), (9, 13), TypeError, 'crops must be integers (image, y0, x0, h, w, flip), got float32'),
    ([(0, 0, 0, 8, 8)], (9, 13), ValueError, 'crops must be [n, 6] (image, y0, x0, h, w, flip), got shape (1, 5)'),
    (np.zeros((2 ** 20 + 1, 6), dtype=np.int8), (9, 13), ValueError, 'decode_resized_crops needs 1 to 2^20 crops'),
    ([(0, 0, 0, 8, 8, 0), (2, 0, 0, 8, 8, 1)], (9, 13), ValueError, 'crop 1: image 2 out of range [0, 2)'),
    ([(0, 0, 0, 8, 8, 0), (1, 0, 0, 0, 8, 1)], (9, 13), ValueError, 'crop 1: box of 0x8: both sides must be >= 1'),
    ([(0, 0, 0, 8, 8, 0), (1, 40, 0, 6, 8, 1)], (9, 13), ValueError, 'crop 1: 6x8 at (40, 0) leaves image 1 of 32x48'),
]


@pytest.mark.parametrize("case", range(len(MESSAGES)))
def test_check_resized_args_messages(case):
    from lrf_amd._lib import check_resized_args
    crops, size, kind, text = MESSAGES[case]
    U, V, images = _two_images()
    with pytest.raises(kind) as e:
        check_resized_args(U, V, images, crops, size)
    assert type(e.value) is kind and str(e.value) == text
