"""CPU suite: what check_crop_args and qmf_decode_crops refuse before a GPU is asked for — boxes that leave their image, negative
origins, image indices out of range, an empty list, sizes below 1, boxes that are not integers, streams of another branch."""
import numpy as np
import pytest
import torch

from conftest import Case

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
    """24x48 and 45x61 at (7,3,3), zero factors on the host"""
    from lrf_amd import _lib
    images, uo, vo = [], 0, 0
    for H, W in ((24, 48), (45, 61)):
        images.append((H, W, RANKS, uo, vo))
        uo += sum(d[4] * r for d, r in zip(_lib.plane_dims(H, W), RANKS))
        vo += 64 * sum(RANKS)
    return torch.zeros(uo, dtype=torch.int8), torch.zeros(vo, dtype=torch.int8), images


def test_exported():
    import os

    import lrf_amd
    from conftest import ROOT
    from lrf_amd import _lib
    for name in ("qmf_decode_crops", "qmf_load_factors"):
        assert name in lrf_amd.__all__ and callable(getattr(lrf_amd, name))
    assert "lrf_qmf_decode_crops_rgb_u8" in _lib.EXPORTS
    assert "lrf_qmf_decode_crops_rgb_u8(" in open(os.path.join(ROOT, "include", "lrf_hip.h")).read()


def test_good_boxes_come_back_as_int32():
    from lrf_amd._lib import check_crop_args
    U, V, images = _two_images()
    ims, boxes, size = check_crop_args(U, V, images, [(0, 0, 0), (0, 15, 35), (1, 36, 48)], (9, 13))  # the far corners: 15 + 9 = 24, 48 + 13 = 61
    assert boxes.dtype == np.int32 and boxes.tolist() == [[0, 0, 0], [0, 15, 35], [1, 36, 48]] and size == (9, 13) and len(ims) == 2
    assert check_crop_args(U, V, images, torch.tensor([[1, 0, 0]]), (45, 61))[1].tolist() == [[1, 0, 0]]  # the whole image; a host tensor
    assert check_crop_args(U, V, images, np.array([[0, 23, 47]], dtype=np.uint16), (np.int64(1), 1))[2] == (1, 1)


@pytest.mark.parametrize("crops,size", [
    ([(0, 16, 0)], (9, 13)),        # 16 + 9 > 24
    ([(0, 0, 36)], (9, 13)),        # 36 + 13 > 48
    ([(0, 0, 0), (1, 37, 0)], (9, 13)),
    ([(0, 0, 0)], (25, 13)),        # taller than its image
    ([(1, 0, 0)], (24, 62)),        # wider than its image
    ([(0, -1, 0)], (9, 13)),
    ([(0, 0, -1)], (9, 13)),
    ([(2, 0, 0)], (9, 13)),
    ([(-1, 0, 0)], (9, 13)),
    ([], (9, 13)),
    (np.zeros((0, 3), dtype=np.int32), (9, 13)),
    ([(0, 0, 0)], (0, 13)),
    ([(0, 0, 0)], (9, -2)),
    ([(0, 0)], (9, 13)),            # not [n, 3]
    ([0, 0, 0], (9, 13)),
    ([(0, 0, 0)], (9,)),
    ([(0, 2 ** 40, 0)], (9, 13)),   # no wrap on the way to int32
])
def test_check_crop_args_raises_value_error(crops, size):
    from lrf_amd._lib import check_crop_args
    U, V, images = _two_images()
    with pytest.raises(ValueError):
        check_crop_args(U, V, images, crops, size)


@pytest.mark.parametrize("crops,size", [
    ([(0.0, 0.0, 0.0)], (9, 13)),
    (np.zeros((2, 3), dtype=np.float32), (9, 13)),
    (torch.zeros((2, 3)), (9, 13)),
    ([(0, 0, 0)], (9.0, 13)),
    ([(0, 0, 0)], (True, 13)),
])
def test_check_crop_args_raises_type_error(crops, size):
    from lrf_amd._lib import check_crop_args
    U, V, images = _two_images()
    with pytest.raises(TypeError):
        check_crop_args(U, V, images, crops, size)


def test_factors_are_checked_as_the_ragged_decode_checks_them():
    from lrf_amd._lib import check_crop_args
    U, V, images = _two_images()
    with pytest.raises(TypeError):
        check_crop_args(U.float(), V, images, [(0, 0, 0)], (1, 1))
    with pytest.raises(ValueError):
        check_crop_args(U[:-1], V, images, [(0, 0, 0)], (1, 1))
    with pytest.raises(ValueError):
        check_crop_args(U, V, [(24, 48, (7, 3, 65), 0, 0)], [(0, 0, 0)], (1, 1))
    with pytest.raises(ValueError):
        check_crop_args(U, V, [], [(0, 0, 0)], (1, 1))


def test_qmf_decode_crops_refuses_before_a_gpu_is_asked_for(no_gpu):
    from lrf_amd import qmf_decode_crops
    tiny, odd = Case("tiny_q7"), Case("odd_q7")
    streams = [tiny.encoded, odd.encoded]
    (H0, W0), (H1, W1) = tiny.image.shape[-2:], odd.image.shape[-2:]
    for crops, size in (([(0, H0 - 3, 0)], (4, 4)), ([(1, 0, W1 - 3)], (4, 4)), ([(0, -1, 0)], (4, 4)), ([(2, 0, 0)], (4, 4)), ([], (4, 4)),
                        ([(0, 0, 0)], (0, 4)), ([(0, 0, 0)], (H0 + 1, 1))):
        with pytest.raises(ValueError):
            qmf_decode_crops(streams, crops, size)
    with pytest.raises(TypeError):
        qmf_decode_crops(streams, [(0.5, 0.0, 0.0)], (4, 4))
    with pytest.raises(ValueError):
        qmf_decode_crops([], [(0, 0, 0)], (4, 4))
    with pytest.raises(TypeError):
        qmf_decode_crops([tiny.encoded, "text"], [(0, 0, 0)], (4, 4))


def test_streams_of_other_branches_raise_naming_the_branch(no_gpu):
    from lrf_amd import qmf_decode_crops, qmf_load_factors
    good = Case("tiny_q7").encoded
    for name, word in (("rgbsp_odd_q6", "RGB"), ("any_p16_q10", "patch size"), ("any_nopatch_q10", "patch=False")):
        with pytest.raises(NotImplementedError, match=word):
            qmf_decode_crops([good, Case(name).encoded], [(0, 0, 0)], (4, 4))
        with pytest.raises(NotImplementedError, match=word):
            qmf_load_factors([Case(name).encoded, good])


class OnDevice:
    """stands for a CUDA tensor of boxes: the refusal must come before its values are asked for"""
    is_cuda = True

    def detach(self):
        raise AssertionError("the boxes were read")


# one bad input per check of check_crop_args, in the order of the checks, with the text it raises
MESSAGES = [
    ([(0, 0, 0)], 9, ValueError, 'size must be (h, w), got 9'),
    ([(0, 0, 0)], (9.0, 13), TypeError, 'size must hold two integers, got (9.0, 13)'),
    ([(0, 0, 0)], (0, 13), ValueError, 'crop size 0x13: both sides must be >= 1'),
    (OnDevice(), (9, 13), ValueError, 'crops live on the host: the call validates every box before it launches'),
    ([], (9, 13), ValueError, 'decode_crops needs 1 to 2^20 crops'),
    ([(0.0, 0.0, 0.0)], (9, 13), TypeError, 'crops must be integers (image, y0, x0), got float64'),
    ([(0, 0)], (9, 13), ValueError, 'crops must be [n, 3] (image, y0, x0), got shape (1, 2)'),
    (np.zeros((2 ** 20 + 1, 3), dtype=np.int8), (9, 13), ValueError, 'decode_crops needs 1 to 2^20 crops'),
    ([(0, 0, 0), (2, 0, 0)], (9, 13), ValueError, 'crop 1: image 2 out of range [0, 2)'),
    ([(0, 0, 0), (1, 37, 0)], (9, 13), ValueError, 'crop 1: 9x13 at (37, 0) leaves image 1 of 45x61'),
]


@pytest.mark.parametrize("case", range(len(MESSAGES)))
def test_check_crop_args_messages(case):
    from lrf_amd._lib import check_crop_args
    crops, size, kind, text = MESSAGES[case]
    U, V, images = _two_images()
    with pytest.raises(kind) as e:
        check_crop_args(U, V, images, crops, size)
    assert type(e.value) is kind and str(e.value) == text
