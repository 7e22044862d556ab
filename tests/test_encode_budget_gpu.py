"""GPU suite (-m gpu): qmf_encode_budget against a brute force built from public functions that do not know it — qmf_encode_batch
(deflate="device") at every quality, len() of each stream, qmf_decode_batch + psnr_batch, then the selection rule in plain Python.
Chosen qualities, the reached flags, the sizes, both tables (the PSNR bitwise float64) and the streams (byte for byte) must be
EQUAL.  Every budget is taken from the brute-force size table; no byte number is fixed in advance."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, make_image

pytestmark = pytest.mark.gpu

H, W = 192, 256
QUALITIES = list(range(1, 33))


def _batch():
    """the batch of tests/test_encode_target_gpu.py: three smooth images, four crops of the natural fixture, two of uniform noise"""
    nat = torch.from_numpy(np.load(os.path.join(GOLDEN, "nat_q7.npz"))["image"])
    imgs = [make_image(dict(kind="smooth", seed=300 + i, H=H, W=W)) for i in range(3)]
    imgs += [nat[:, y:y + H, x:x + W] for y, x in ((0, 0), (200, 300), (400, 600), (450, 100))]
    g = torch.Generator().manual_seed(11)
    imgs += [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for _ in range(2)]
    return torch.stack(imgs).contiguous()


_BRUTE = {}


def _brute(images, qualities=QUALITIES):
    """(streams [Q][B], sizes int64 [Q,B], PSNR float64 [Q,B] on the host), computed once per quality list"""
    import lrf_amd
    key = (tuple(qualities), images.shape[0])
    if key not in _BRUTE:
        streams = [lrf_amd.qmf_encode_batch(images, quality=q, deflate="device") for q in qualities]
        size = torch.tensor([[len(s) for s in row] for row in streams], dtype=torch.int64)
        table = torch.stack([lrf_amd.psnr_batch(images, lrf_amd.qmf_decode_batch(row)).cpu() for row in streams])
        _BRUTE[key] = (streams, size, table)
    return _BRUTE[key]


def _rule(size, table, qualities, budget):
    """the issue's rule in plain Python -> (row index per image, reached per image); the lowest error is the highest PSNR"""
    order = sorted(range(len(qualities)), key=lambda i: qualities[i])
    index, reached = [], []
    for b in range(size.shape[1]):
        fit = [i for i in order if int(size[i, b]) <= int(budget[b])]
        if fit:
            index.append(min(fit, key=lambda i: (-table[i, b].item(), int(size[i, b]), qualities[i])))
        else:
            index.append(min(order, key=lambda i: (int(size[i, b]), qualities[i])))
        reached.append(bool(fit))
    return index, reached


def _assert_equal(out, images, qualities, budget):
    streams, size, table = _brute(images, qualities)
    B = images.shape[0]
    budget = [int(budget)] * B if not hasattr(budget, "__len__") else [int(x) for x in budget]
    index, reached = _rule(size, table, qualities, budget)
    print("budget", budget, "chosen", out["quality"], "brute", [qualities[i] for i in index], "reached", out["reached"].tolist(),
          "nbytes", out["nbytes"].tolist())
    assert out["size_table"].dtype == torch.int64 and torch.equal(out["size_table"], size)
    assert out["table"].dtype == torch.float64 and torch.equal(out["table"], table)  # bitwise
    assert out["quality"] == [qualities[i] for i in index]
    assert out["reached"].dtype == torch.bool and out["reached"].tolist() == reached
    assert out["nbytes"].dtype == torch.int64 and out["nbytes"].tolist() == [int(size[i, b]) for b, i in enumerate(index)]
    assert torch.equal(out["psnr"], torch.stack([table[i, b] for b, i in enumerate(index)]))  # bitwise
    for b, i in enumerate(index):
        assert out["streams"][b] == streams[i][b], (b, qualities[i])
    return index, reached


def test_budget_equals_the_brute_force_and_spreads_over_qualities():
    import lrf_amd
    images = _batch()
    _, size, _ = _brute(images)
    # one budget for the batch from the brute-force size table: its median over all (quality, image) pairs
    budget = int(size.flatten().median())
    out = lrf_amd.qmf_encode_budget(images, nbytes=budget)
    _assert_equal(out, images, QUALITIES, budget)
    assert len(set(out["quality"])) >= 3, out["quality"]
    assert bool((out["nbytes"][out["reached"]] <= budget).all())
    # Both values of `reached`: the median does not give them on this batch (every image's smallest stream, 885 to 1,120 bytes,
    # lies far below it), so the quantile that does is used — the 0.03 quantile of the same table, which falls among the images'
    # smallest streams.  No single budget gives both flags AND three qualities here: the sizes grow with the quality on every
    # image of this batch, so a budget that some image's smallest stream misses admits nothing but the lowest triple anywhere.
    low = int(torch.quantile(size.flatten().double(), 0.03, interpolation="lower"))
    out_low = lrf_amd.qmf_encode_budget(images, nbytes=low)
    _assert_equal(out_low, images, QUALITIES, low)
    assert set(out_low["reached"].tolist()) == {True, False}, out_low["reached"].tolist()
    assert bool((out_low["nbytes"][out_low["reached"]] <= low).all()) and bool((out_low["nbytes"][~out_low["reached"]] > low).all())
    # a stream is what the per-image encoder writes at the chosen quality ...
    for b in (0, 4, 8):
        assert out["streams"][b] == lrf_amd.qmf_encode_batch(images[b:b + 1], quality=out["quality"][b], deflate="device")[0]
    # ... decodes, on the host path and through the device inflate, to the image whose PSNR is reported, at the reported rate
    for b, s in enumerate(out["streams"]):  # (one by one: their ranks differ)
        dec = lrf_amd.qmf_decode(s).cpu()
        assert torch.equal(dec, lrf_amd.qmf_decode_batch([s], inflate="device")[0].cpu())
        assert torch.equal(lrf_amd.psnr_batch(images[b:b + 1], dec[None]).cpu(), out["psnr"][b:b + 1])
        assert out["bpp"][b].item() == lrf_amd.bits_per_pixel((H, W), s)
    assert out["bpp"].dtype == torch.float64 and out["psnr"].dtype == torch.float64
    # the same budget as bits per pixel (half a byte above it, so that the floor lands on it), a float and a tensor
    bpp = (budget + 0.5) * 8 / (H * W)
    assert lrf_amd.qmf_encode_budget(images, bpp=bpp)["streams"] == out["streams"]
    assert lrf_amd.qmf_encode_budget(images, bpp=torch.full((images.shape[0],), bpp, dtype=torch.float64))["streams"] == out["streams"]


def test_zero_budget_takes_the_smallest_stream():
    import lrf_amd
    images = _batch()
    _, size, _ = _brute(images)
    out = lrf_amd.qmf_encode_budget(images, nbytes=0)
    _assert_equal(out, images, QUALITIES, 0)
    assert out["reached"].tolist() == [False] * images.shape[0]
    assert torch.equal(out["nbytes"], size.min(dim=0).values)


def test_a_budget_above_every_size_takes_the_lowest_error():
    import lrf_amd
    images = _batch()
    _, size, table = _brute(images)
    out = lrf_amd.qmf_encode_budget(images, nbytes=int(size.max()) + 1)
    _assert_equal(out, images, QUALITIES, int(size.max()) + 1)
    assert out["reached"].tolist() == [True] * images.shape[0]
    assert torch.equal(out["psnr"], table.max(dim=0).values)


def test_per_image_budgets():
    import lrf_amd
    images = _batch()
    _, size, _ = _brute(images)
    B = images.shape[0]
    budget = [int(size[3 + 3 * b, b]) for b in range(B)]  # image b's own size at quality 4 + 3 b
    out = lrf_amd.qmf_encode_budget(images, nbytes=budget)
    index, reached = _assert_equal(out, images, QUALITIES, budget)
    assert all(reached) and all(int(n) <= x for n, x in zip(out["nbytes"], budget))
    for b, i in enumerate(index):  # at the budget exactly where the stream of that size is the best fit
        if int(size[i, b]) == budget[b]:
            assert int(out["nbytes"][b]) == budget[b]
    assert any(int(n) == x for n, x in zip(out["nbytes"], budget))
    as_tensor = lrf_amd.qmf_encode_budget(images, nbytes=torch.tensor(budget))
    assert as_tensor["streams"] == out["streams"]
    bpp = torch.tensor([(x + 0.5) * 8 / (H * W) for x in budget], dtype=torch.float64)
    assert lrf_amd.qmf_encode_budget(images, bpp=bpp)["streams"] == out["streams"]


def test_qualities_that_reach_ranks_above_32():
    import lrf_amd
    images = _batch()[2:7]
    qualities = [60, 10, 40, 11]  # 60 -> ranks (38, 19, 19): outside the fused sweep; unsorted on purpose
    assert max(lrf_amd.qmf_ranks((H, W), quality=60)) > 32
    _, size, _ = _brute(images, qualities)
    for budget in (int(size.flatten().median()), int(size.min()), 0, int(size.max()) + 1):
        _assert_equal(lrf_amd.qmf_encode_budget(images, nbytes=budget, qualities=qualities), images, qualities, budget)


def test_host_and_device_input_give_the_same_result():
    import lrf_amd
    images = _batch()
    _, size, _ = _brute(images)
    budget = int(size.flatten().median())
    a = lrf_amd.qmf_encode_budget(images, nbytes=budget)
    b = lrf_amd.qmf_encode_budget(images.cuda(), nbytes=budget)
    assert a["streams"] == b["streams"] and a["quality"] == b["quality"]
    for key in ("nbytes", "bpp", "psnr", "reached", "size_table", "table"):
        assert not b[key].is_cuda and torch.equal(a[key], b[key]), key
