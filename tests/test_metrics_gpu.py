"""GPU suite (-m gpu): lrf_image_metrics_u8 / lrf_amd.image_metrics_batch against the host definitions lrf_amd.metrics.ssim / psnr.
The squared error is an exact integer and must be EQUAL; the SSIM differs by float64 rounding of ~20 operations per window and the
order of at most 1.2e6 additions (bar 1e-9); the host PSNR is float32 (bar 1e-4 dB).  tests/metrics_cases.py holds the pairs."""
import math

import numpy as np
import pytest
import torch

from conftest import config3_image
from metrics_cases import PSNR_BAR, SSIM_BAR, cases, pairs_of_size

pytestmark = pytest.mark.gpu


def _host(a, b):
    from lrf_amd import metrics
    with np.errstate(invalid="ignore"):
        return metrics.ssim(a, b).item(), metrics.psnr(a, b).item()


def _check(name, a, b, sse, psnr, ssim):
    """one image pair (uint8 host tensors [C,H,W]) against the host functions, every figure printed before it is asserted"""
    ref_s, ref_p = _host(a, b)
    exact = int(((a.long() - b.long()) ** 2).sum())
    print(f"{name}: sse {sse} / {exact}  ssim {ssim!r} / {ref_s!r} (diff {abs(ssim - ref_s):.3g})  psnr {psnr!r} / {ref_p!r}")
    assert sse == exact, name
    if math.isnan(ref_s):
        assert math.isnan(ssim), name
    else:
        assert abs(ssim - ref_s) <= SSIM_BAR, (name, ssim, ref_s)
    if math.isinf(ref_p):
        assert psnr == ref_p, name
    else:
        assert abs(psnr - ref_p) <= PSNR_BAR, (name, psnr, ref_p)


def _extra_cases():
    rng = np.random.default_rng(2)
    for H, W in [(40, 67), (23, 130), (64, 100), (31, 71)]:  # widths not divisible by 4 or 16, more than one tile each way
        for name, a, b in list(pairs_of_size(H, W, rng))[1:4]:
            yield name, a, b
    a = rng.integers(0, 256, (1, 7, 7), dtype=np.uint8)
    yield "1x7x7", a, (a ^ 3).astype(np.uint8)
    for name, a, b in list(pairs_of_size(50, 96, rng, C=1))[2:7]:
        yield "C=1 " + name, a, b
    a = np.full((3, 20, 33), 77, np.uint8)  # constant first image: NaN on the host
    yield "constant pair", a, a.copy()
    a = rng.integers(0, 256, (5, 30, 64), dtype=np.uint8)
    yield "C=5", a, np.clip(a.astype(int) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)


def test_device_metrics_equal_the_host_definitions():
    import lrf_amd
    n = 0
    for name, a, b in list(cases()) + list(_extra_cases()):
        ta, tb = torch.from_numpy(a), torch.from_numpy(b)
        m = lrf_amd.image_metrics_batch(ta, tb)
        assert m["sse"].dtype == torch.int64 and m["ssim"].dtype == torch.float64 and m["psnr"].dtype == torch.float64
        assert m["sse"].is_cuda and tuple(m["ssim"].shape) == (1,)
        assert math.isclose(m["mse"].item(), m["sse"].item() / a.size, rel_tol=4 * 2.0 ** -52)  # (one float64 division on the device)
        _check(name, ta, tb, m["sse"].item(), m["psnr"].item(), m["ssim"].item())
        n += 1
    assert n >= 60
    # pairs of one size as a batch, from tensors that are on the device already
    rng = np.random.default_rng(3)
    batch = list(pairs_of_size(61, 47, rng))
    A = torch.from_numpy(np.stack([p[1] for p in batch])).cuda()
    Bt = torch.from_numpy(np.stack([p[2] for p in batch])).cuda()
    m = lrf_amd.image_metrics_batch(A, Bt)
    for i, (name, a, b) in enumerate(batch):
        _check("batched " + name, torch.from_numpy(a), torch.from_numpy(b), m["sse"][i].item(), m["psnr"][i].item(), m["ssim"][i].item())
    # the library's own refusal (the Python checks come first, so this goes to the entry point directly)
    from lrf_amd import _lib
    lib, ctx = _lib.load(), _lib.context()
    s = torch.empty(1, dtype=torch.int64, device="cuda")
    d = torch.empty(1, dtype=torch.float64, device="cuda")
    small = torch.zeros((1, 3, 6, 9), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        _lib.check(lib.lrf_image_metrics_u8(ctx._h, small.data_ptr(), small.data_ptr(), 1, 3, 6, 9, s.data_ptr(), d.data_ptr()))
    with pytest.raises(ValueError):
        _lib.check(lib.lrf_image_metrics_u8(ctx._h, small.data_ptr(), small.data_ptr(), 0, 3, 6, 9, s.data_ptr(), None))
    with pytest.raises(ValueError):
        _lib.check(lib.lrf_image_metrics_u8(ctx._h, small.data_ptr(), None, 1, 3, 6, 9, s.data_ptr(), None))


def test_an_image_scores_the_same_bits_wherever_it_stands():
    import lrf_amd
    rng = np.random.default_rng(4)
    for H, W in [(96, 160), (45, 77)]:
        A = torch.from_numpy(rng.integers(0, 256, (37, 3, H, W), dtype=np.uint8)).cuda()
        noise = torch.from_numpy(rng.integers(-12, 13, (37, 3, H, W))).cuda()
        Bt = (A.long() + noise).clamp(0, 255).to(torch.uint8)
        bits = lambda t: t.view(torch.int64).cpu()
        whole = lrf_amd.image_metrics_batch(A, Bt)
        again = lrf_amd.image_metrics_batch(A, Bt)
        assert torch.equal(bits(whole["ssim"]), bits(again["ssim"])) and torch.equal(whole["sse"], again["sse"])
        for i in (0, 17, 36):
            alone = lrf_amd.image_metrics_batch(A[i], Bt[i])
            assert torch.equal(bits(alone["ssim"]), bits(whole["ssim"][i:i + 1])), (H, W, i)
            assert alone["sse"].item() == whole["sse"][i].item()
            order = [i] + [j for j in range(37) if j != i]  # image i first ...
            first = lrf_amd.image_metrics_batch(A[order].contiguous(), Bt[order].contiguous())
            assert torch.equal(bits(first["ssim"][:1]), bits(whole["ssim"][i:i + 1])), (H, W, i)
            order = order[1:] + [i]  # ... and last
            last = lrf_amd.image_metrics_batch(A[order].contiguous(), Bt[order].contiguous())
            assert torch.equal(bits(last["ssim"][-1:]), bits(whole["ssim"][i:i + 1])), (H, W, i)
        assert len(set(bits(whole["ssim"]).tolist())) == 37  # (different images)


def test_psnr_alone_gives_the_same_squared_error():
    import lrf_amd
    rng = np.random.default_rng(5)
    for shape in [(5, 3, 64, 96), (3, 3, 33, 47), (2, 1, 5, 6), (2, 3, 50, 50)]:  # 16-, 1-, 1- and 4-byte pieces
        A = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))
        Bt = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))
        m = lrf_amd.image_metrics_batch(A, Bt, want_ssim=False)
        assert "ssim" not in m
        exact = ((A.long() - Bt.long()) ** 2).sum(dim=(1, 2, 3))
        assert torch.equal(m["sse"].cpu(), exact), shape
        p = lrf_amd.psnr_batch(A, Bt)
        assert torch.equal(p, m["psnr"])
        if shape[-2] >= 7:
            full = lrf_amd.image_metrics_batch(A, Bt)
            assert torch.equal(full["sse"], m["sse"]) and torch.equal(full["psnr"], p)
            assert torch.equal(lrf_amd.ssim_batch(A, Bt).view(torch.int64), full["ssim"].view(torch.int64))
        ref = torch.stack([lrf_amd.psnr(A[i], Bt[i]) for i in range(shape[0])]).double()
        assert (p.cpu() - ref).abs().max().item() <= PSNR_BAR


def test_full_size_batches():
    """The real workload: 256 x 3x512x768 decoded at quality 7 against their originals, and config 4's odd height."""
    import lrf_amd
    from lrf_amd import _lib
    imgs = torch.stack([config3_image(i % 24) for i in range(256)])
    imgs[24:] ^= torch.arange(256 - 24, dtype=torch.uint8).view(-1, 1, 1, 1) % 8  # (copies that differ in their low bits)
    dev = imgs.cuda()
    rec = lrf_amd.qmf_decode_batch(lrf_amd.qmf_encode_batch(dev, quality=7))
    ctx = _lib.context()
    ctx.profile_kernels([_lib.LRF_K_METRICS])
    ctx.profile_reset()
    try:
        m = lrf_amd.image_metrics_batch(dev, rec)
        ms, launches = ctx.kernel_time(_lib.LRF_K_METRICS)
    finally:
        ctx.profile(False)
    print(f"256 x 3x512x768: LRF_K_METRICS {ms:.3f} ms in {launches} call(s)")
    assert launches > 0 and ms > 0
    rec_h = rec.cpu()
    for i in (0, 5, 23, 24, 100, 171, 254, 255):
        _check(f"512x768 image {i}", imgs[i], rec_h[i], m["sse"][i].item(), m["psnr"][i].item(), m["ssim"][i].item())
    g = torch.Generator().manual_seed(11)
    A = torch.randint(0, 256, (4, 3, 1365, 2048), dtype=torch.uint8, generator=g)
    A[1] = (A[1] // 16) * 3 + 40  # a narrow data_range
    Bt = (A.int() + torch.randint(-20, 21, A.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    m = lrf_amd.image_metrics_batch(A, Bt)
    for i in range(4):
        _check(f"1365x2048 image {i}", A[i], Bt[i], m["sse"][i].item(), m["psnr"][i].item(), m["ssim"][i].item())


def test_sweep_with_device_metrics_matches_the_host_sweep():
    import lrf_amd
    imgs = [config3_image(i)[:, :96, :160].contiguous() for i in (0, 5, 20, 23)]  # test_batched_sweep_equals_the_per_image_loop's
    qualities = (2, 9, 21, 33)
    stack = torch.stack(imgs)
    host = lrf_amd.rd_sweep_batched(stack, qualities, metrics="host")
    dev = lrf_amd.rd_sweep_batched(stack, qualities, metrics="device")
    assert len(host) == len(dev) == 16
    for h, d in zip(host, dev):
        assert (h["image"], h["quality"]) == (d["image"], d["quality"])
        assert set(d) == set(h) | {"metrics time (ms)"} and "metrics time (ms)" not in h
        for k in ("bit rate (bpp)", "compression ratio", "SSIM pinned to scikit-image"):
            assert h[k] == d[k], (k, h[k], d[k])
        print(h["image"], h["quality"], h["PSNR (dB)"], d["PSNR (dB)"], h["SSIM"], d["SSIM"])
        assert abs(h["PSNR (dB)"] - d["PSNR (dB)"]) <= PSNR_BAR
        assert abs(h["SSIM"] - d["SSIM"]) <= SSIM_BAR
        assert d["metrics time (ms)"] > 0
    one = lrf_amd.rd_sweep(imgs, qualities, lrf_amd.qmf_encode, lrf_amd.qmf_decode)
    dflt = {(r["image"], r["quality"]): r for r in lrf_amd.rd_sweep_batched(stack, qualities)}
    for r in one:
        for k in ("compression ratio", "bit rate (bpp)", "PSNR (dB)", "SSIM"):
            assert r[k] == dflt[(r["image"], r["quality"])][k], k
        assert "metrics time (ms)" not in dflt[(r["image"], r["quality"])]
