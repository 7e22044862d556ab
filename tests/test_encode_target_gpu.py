"""GPU suite (-m gpu): qmf_encode_target against a brute force built from existing public functions only — qmf_encode_sweep to
byte streams at every quality, qmf_decode_batch, psnr_batch, then the selection rule in plain Python.  Chosen qualities, the
reached flags, the PSNR (bitwise float64), the whole table and the streams (byte for byte) must be EQUAL."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, make_image

pytestmark = pytest.mark.gpu

H, W = 192, 256
QUALITIES = list(range(1, 33))


def _batch():
    """nine images of one size: three smooth, four crops of the natural fixture, two of uniform noise"""
    nat = torch.from_numpy(np.load(os.path.join(GOLDEN, "nat_q7.npz"))["image"])
    imgs = [make_image(dict(kind="smooth", seed=300 + i, H=H, W=W)) for i in range(3)]
    imgs += [nat[:, y:y + H, x:x + W] for y, x in ((0, 0), (200, 300), (400, 600), (450, 100))]
    g = torch.Generator().manual_seed(11)
    imgs += [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for _ in range(2)]
    return torch.stack(imgs).contiguous()


_BRUTE = {}


def _brute(images, qualities=QUALITIES):
    """(streams [Q][B], table float64 [Q,B] on the host) by the existing public functions"""
    import lrf_amd
    key = tuple(qualities)
    if key not in _BRUTE:
        sweep = lrf_amd.qmf_encode_sweep(images, qualities=qualities)
        table = torch.stack([lrf_amd.psnr_batch(images, lrf_amd.qmf_decode_batch(s)).cpu() for s in sweep])
        _BRUTE[key] = (sweep, table)
    return _BRUTE[key]


def _rule(table, qualities, target):
    """the issue's rule in plain Python -> (row index per image, reached per image)"""
    order = sorted(range(len(qualities)), key=lambda i: qualities[i])
    index, reached = [], []
    for b in range(table.shape[1]):
        tb = float(target[b]) if hasattr(target, "__len__") else float(target)
        hit = [i for i in order if table[i, b].item() >= tb]
        if hit:
            index.append(hit[0])
            reached.append(True)
        else:
            best = max(table[i, b].item() for i in order)
            index.append([i for i in order if table[i, b].item() == best][0])
            reached.append(False)
    return index, reached


def _assert_equal(out, images, qualities, target):
    sweep, table = _brute(images, qualities)
    index, reached = _rule(table, qualities, target)
    print("target", target, "chosen", out["quality"], "brute", [qualities[i] for i in index], "reached", out["reached"].tolist())
    assert out["table"].dtype == torch.float64 and torch.equal(out["table"], table)
    assert out["quality"] == [qualities[i] for i in index]
    assert out["reached"].tolist() == reached
    assert torch.equal(out["psnr"], torch.stack([table[i, b] for b, i in enumerate(index)]))  # bitwise
    for b, i in enumerate(index):
        assert out["streams"][b] == sweep[i][b], (b, qualities[i])


def test_target_equals_the_brute_force_and_spreads_over_qualities():
    import lrf_amd
    images = _batch()
    _, table = _brute(images)
    # the target comes from the brute-force table — its median PSNR — so that some images pass it at the lowest quality, some
    # inside the grid and the noise images never: at least three different choices, by construction of the batch
    target = float(table.median())
    out = lrf_amd.qmf_encode_target(images, target)
    _assert_equal(out, images, QUALITIES, target)
    assert len(set(out["quality"])) >= 3, out["quality"]
    assert True in out["reached"].tolist()
    # a stream is what the per-image encoder writes at the chosen quality
    for b in (0, 4, 8):
        assert out["streams"][b] == lrf_amd.qmf_encode_batch(images[b:b + 1], quality=out["quality"][b])[0]
    # ... and decodes to the reported PSNR
    dec = torch.stack([lrf_amd.qmf_decode(s).cpu() for s in out["streams"]])  # (one by one: their ranks differ)
    assert torch.equal(lrf_amd.psnr_batch(images, dec).cpu(), out["psnr"])


def test_unreachable_target_takes_the_best_candidate():
    import lrf_amd
    images = _batch()
    _, table = _brute(images)
    out = lrf_amd.qmf_encode_target(images, 200.0)
    _assert_equal(out, images, QUALITIES, 200.0)
    assert out["reached"].tolist() == [False] * images.shape[0]
    assert torch.equal(out["psnr"], table.max(dim=0).values)


def test_zero_db_takes_the_lowest_quality():
    import lrf_amd
    images = _batch()
    out = lrf_amd.qmf_encode_target(images, 0.0)
    _assert_equal(out, images, QUALITIES, 0.0)
    assert out["quality"] == [1] * images.shape[0] and all(out["reached"].tolist())


def test_per_image_targets():
    import lrf_amd
    images = _batch()
    _, table = _brute(images)
    target = [table[5 + 3 * b, b].item() for b in range(images.shape[0])]  # image b's own PSNR at quality 6 + 3 b
    out = lrf_amd.qmf_encode_target(images, target)
    _assert_equal(out, images, QUALITIES, target)
    out_t = lrf_amd.qmf_encode_target(images, torch.tensor(target, dtype=torch.float64))
    assert out_t["streams"] == out["streams"]


def test_qualities_that_reach_ranks_above_32():
    import lrf_amd
    images = _batch()[2:7]
    qualities = [60, 10, 40, 11]  # 60 -> ranks (38, 19, 19): outside the fused sweep; unsorted on purpose
    assert max(lrf_amd.qmf_ranks((H, W), quality=60)) > 32
    _, table = _brute(images, qualities)
    for target in (float(table[2].median()), float(table[0].min()), 0.0, 200.0):
        _assert_equal(lrf_amd.qmf_encode_target(images, target, qualities=qualities), images, qualities, target)


def test_host_and_device_input_give_the_same_streams():
    import lrf_amd
    images = _batch()
    _, table = _brute(images)
    target = float(table.median())
    a = lrf_amd.qmf_encode_target(images, target)
    b = lrf_amd.qmf_encode_target(images.cuda(), target)
    assert a["streams"] == b["streams"] and a["quality"] == b["quality"] and torch.equal(a["table"], b["table"])
