"""CPU suite: the choice qmf_encode_target(ssim=...) makes (select_target_ssim, pure torch) on hand-made tables, and what
qmf_encode_target(ssim=...) and image_metrics_ragged refuse before a context exists — none of it needs a GPU."""
import math

import pytest
import torch

import lrf_amd
from lrf_amd import _lib, select_target_ssim

NAN = float("nan")


def t64(rows):
    return torch.tensor(rows, dtype=torch.float64)


def pick(ssim, psnr, target):
    index, reached = select_target_ssim(t64(ssim), t64(psnr), t64(target))
    assert index.dtype == torch.int64 and reached.dtype == torch.bool
    return index.tolist(), reached.tolist()


def by_hand(ssim, psnr, target):
    """the rule written out per image"""
    Q, B = len(ssim), len(ssim[0])
    index, reached = [], []
    for b in range(B):
        col, tgt = [ssim[q][b] for q in range(Q)], target[b] if len(target) > 1 else target[0]
        ok = [q for q in range(Q) if not math.isnan(col[q]) and col[q] >= tgt]
        if ok:
            index.append(ok[0])
            reached.append(True)
            continue
        reached.append(False)
        real = [q for q in range(Q) if not math.isnan(col[q])]
        if real:
            index.append(max(real, key=lambda q: (col[q], -q)))
        else:
            index.append(max(range(Q), key=lambda q: (psnr[q][b], -q)))
    return index, reached


PSNR = [[20.0, 21.0, 22.0, 30.0], [25.0, 21.0, 30.0, 30.0], [24.0, 35.0, 30.0, 29.0], [30.0, 35.0, math.inf, 29.5]]


def test_first_candidate_that_reaches_even_when_ssim_is_not_monotone():
    ssim = [[0.50, 0.90, 0.10, 0.70],
            [0.95, 0.80, 0.40, 0.60],
            [0.70, 0.99, 0.30, 0.65],
            [0.96, 0.85, 0.35, 0.69]]
    got = pick(ssim, PSNR, [0.9])
    assert got == ([1, 0, 1, 0], [True, True, False, False]) == by_hand(ssim, PSNR, [0.9])
    # image 2 never reaches 0.9: the highest SSIM (0.40, candidate 1); image 3: 0.70, candidate 0


def test_ties_take_the_first():
    ssim = [[0.8, 0.5, 0.5], [0.8, 0.7, 0.5], [0.9, 0.7, 0.5], [0.9, 0.6, 0.5]]
    psnr = [row[:3] for row in PSNR]
    assert pick(ssim, psnr, [0.8]) == ([0, 1, 0], [True, False, False]) == by_hand(ssim, psnr, [0.8])
    assert pick(ssim, psnr, [0.9]) == ([2, 1, 0], [True, False, False])
    assert pick(ssim, psnr, [0.5]) == ([0, 0, 0], [True, True, True])  # equality reaches


def test_nan_never_reaches_and_never_wins():
    ssim = [[NAN, 0.2, NAN], [0.6, NAN, NAN], [NAN, 0.9, 0.3], [0.5, NAN, NAN]]
    psnr = [row[:3] for row in PSNR]
    assert pick(ssim, psnr, [0.55]) == ([1, 2, 2], [True, True, False]) == by_hand(ssim, psnr, [0.55])
    assert pick(ssim, psnr, [0.95]) == ([1, 2, 2], [False, False, False]) == by_hand(ssim, psnr, [0.95])
    assert pick(ssim, psnr, [-1.0]) == ([1, 0, 2], [True, True, True])  # (a NaN does not reach even a target below every SSIM)


def test_all_nan_falls_back_to_the_highest_psnr():
    ssim = [[NAN, NAN, NAN, 0.1]] * 4
    # image 0: PSNR 30 at candidate 3; image 1: 35 at candidates 2 and 3, the first; image 2: inf at 3; image 3 has an SSIM
    assert pick(ssim, PSNR, [0.5]) == ([3, 2, 3, 0], [False, False, False, False]) == by_hand(ssim, PSNR, [0.5])
    assert pick(ssim, PSNR, [0.1]) == ([3, 2, 3, 0], [False, False, False, True])


def test_one_target_per_image():
    ssim = [[0.50, 0.90, 0.10, 0.70], [0.95, 0.80, 0.40, 0.60], [0.70, 0.99, 0.30, 0.65], [0.96, 0.85, 0.35, 0.69]]
    target = [0.96, 0.95, 0.30, 0.60]
    assert pick(ssim, PSNR, target) == ([3, 2, 1, 0], [True, True, True, True]) == by_hand(ssim, PSNR, target)
    g = torch.Generator().manual_seed(1)
    for _ in range(20):  # random tables with NaN sprinkled in, against the rule written out
        s = torch.rand((6, 9), generator=g, dtype=torch.float64)
        s[torch.rand((6, 9), generator=g) < 0.3] = NAN
        s[:, 4] = NAN
        p = torch.randint(20, 40, (6, 9), generator=g).double()
        tg = torch.rand((9,), generator=g, dtype=torch.float64)
        assert pick(s.tolist(), p.tolist(), tg.tolist()) == by_hand(s.tolist(), p.tolist(), tg.tolist())


def _no_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a context was asked for before the arguments were refused")
    monkeypatch.setattr(_lib, "context", refuse)


def test_encode_target_refuses_before_a_gpu_is_asked_for(monkeypatch):
    _no_context(monkeypatch)
    img = torch.zeros((3, 32, 40), dtype=torch.uint8)
    batch = torch.zeros((2, 3, 32, 40), dtype=torch.uint8)
    with pytest.raises(ValueError, match="exactly one of 'psnr' and 'ssim'"):
        lrf_amd.qmf_encode_target([img], psnr=30.0, ssim=0.9)
    with pytest.raises(ValueError, match="exactly one of 'psnr' and 'ssim'"):
        lrf_amd.qmf_encode_target([img])
    with pytest.raises(ValueError, match="exactly one of 'psnr' and 'ssim'"):
        lrf_amd.qmf_encode_target(batch, 30.0, ssim=0.9)
    with pytest.raises(ValueError, match="'ssim' must be one number or one per image"):
        lrf_amd.qmf_encode_target([img, img], ssim=[0.9, NAN])
    with pytest.raises(ValueError, match="'ssim' must be one number or one per image"):
        lrf_amd.qmf_encode_target(batch, ssim=NAN)
    with pytest.raises(ValueError, match="'ssim' must be one number or one per image"):
        lrf_amd.qmf_encode_target([img, img], ssim=[0.9, 0.8, 0.7])
    with pytest.raises(ValueError, match=r"image 1 \(6x40\) is smaller than the 7x7 window"):
        lrf_amd.qmf_encode_target([img, torch.zeros((3, 6, 40), dtype=torch.uint8)], ssim=0.9)
    with pytest.raises(ValueError, match=r"image 0 \(32x6\) is smaller than the 7x7 window"):
        lrf_amd.qmf_encode_target(torch.zeros((1, 3, 32, 6), dtype=torch.uint8), ssim=0.9)
    with pytest.raises(NotImplementedError, match="three-channel"):  # gray images go by color_space="RGB": psnr only
        lrf_amd.qmf_encode_target([img[:1]], ssim=0.9, color_space="RGB")
    with pytest.raises(ValueError, match=r"must be \[3,H,W\]"):
        lrf_amd.qmf_encode_target([img[:1]], ssim=0.9)
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        lrf_amd.qmf_encode_target(batch[:, :1], ssim=0.9)
    with pytest.raises(NotImplementedError):
        lrf_amd.qmf_encode_target([img.float()], ssim=0.9)
    with pytest.raises(ValueError, match="qualities"):
        lrf_amd.qmf_encode_target([img], ssim=0.9, qualities=[])


def test_psnr_keeps_its_position():
    import inspect
    params = list(inspect.signature(lrf_amd.qmf_encode_target).parameters)
    assert params[:3] == ["images", "psnr", "qualities"] and "ssim" in params


def test_image_metrics_ragged_refuses_before_a_gpu_is_asked_for(monkeypatch):
    _no_context(monkeypatch)
    a, b = torch.zeros((3, 9, 12), dtype=torch.uint8), torch.zeros((3, 9, 12), dtype=torch.uint8)
    with pytest.raises(ValueError, match="pair 1: both images must have one"):
        lrf_amd.image_metrics_ragged([a, a], [b, torch.zeros((3, 9, 13), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="pair 0: both images"):
        lrf_amd.image_metrics_ragged([a[None]], [b[None]])
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        lrf_amd.image_metrics_ragged([a, a[:, :6]], [b, b[:, :6]])
    with pytest.raises(ValueError, match="channels"):
        lrf_amd.image_metrics_ragged([a, a[:1]], [b, b[:1]])
    with pytest.raises(ValueError, match="one length"):
        lrf_amd.image_metrics_ragged([a, a], [b])
    with pytest.raises(ValueError, match="one length"):
        lrf_amd.image_metrics_ragged([], [])
    with pytest.raises(TypeError):
        lrf_amd.image_metrics_ragged([a.float()], [b])
    with pytest.raises(TypeError):
        lrf_amd.image_metrics_ragged(a, b)
    assert _lib.check_metrics_ragged_args([a, a[:, :6]], [b, b[:, :6]], want_ssim=False) == (3, [(9, 12), (6, 12)])


def test_the_new_names_are_exported():
    for name in ("image_metrics_ragged", "select_target_ssim", "qmf_encode_target"):
        assert name in lrf_amd.__all__ and callable(getattr(lrf_amd, name))
    assert "lrf_image_metrics_ragged_u8" in _lib.EXPORTS and "lrf_qmf_ssim_ragged_rgb_u8" in _lib.EXPORTS
