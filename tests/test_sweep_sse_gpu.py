"""GPU suite (-m gpu): lrf_qmf_sweep_sse_rgb_u8 / Context.sweep_sse — the squared error of a sweep straight from its factors —
against the two calls it replaces, Context.decode_rgb followed by Context.image_metrics.  Everything is an exact integer and
must be EQUAL.  The geometries reach every decode body: 512x768 the 16-aligned tiles, 662x992 and 1365x2048 the strip tiles
(odd height, 3-row pooling windows), 173x264 the general kernels (its chroma planes pad by an odd half)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, config3_image

pytestmark = pytest.mark.gpu

TRIPLES = [(1, 1, 1), (4, 2, 2), (7, 3, 3), (16, 8, 8), (26, 13, 13), (32, 16, 16)]
BIG = (40, 20, 20)  # above 32: not a sweep triple, scored through Q = 1


def _nat():
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "nat_q7.npz"))["image"])


def _geometries():
    nat = _nat()
    yield "512x768", torch.stack([config3_image(0), config3_image(21)])
    yield "662x992 nat", nat.unsqueeze(0)
    yield "173x264 odd", torch.stack([nat[:, 40:213, 100:364], nat[:, 300:473, 500:764]]).contiguous()
    yield "1365x2048", torch.cat([nat, nat.flip(1), nat.flip(2)], 1).repeat(1, 1, 3)[:, :1365, :2048].contiguous().unsqueeze(0)


def _ctx():
    from lrf_amd import _lib
    return _lib.context(None)


def _reference(ctx, dev, factors, triples):
    """[Q,B] int64 by the parent's two calls: decode to memory, then the flat squared-error read"""
    H, W = dev.shape[-2:]
    return torch.stack([ctx.image_metrics(dev, ctx.decode_rgb(U, V, H, W, list(t)), want_ssim=False)[0] for (U, V), t in zip(factors, triples)])


@pytest.mark.parametrize("name,images", list(_geometries()), ids=[n for n, _ in _geometries()])
def test_sweep_sse_equals_decode_then_metrics(name, images):
    import lrf_amd
    ctx = _ctx()
    dev = images.cuda(ctx.device).contiguous()
    factors = ctx.encode_sweep_rgb(dev, TRIPLES, 10, -16, 15)
    got = ctx.sweep_sse(dev, factors, TRIPLES)
    ref = _reference(ctx, dev, factors, TRIPLES)
    print(name, "sweep", got.tolist(), "reference", ref.tolist())
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(TRIPLES), images.shape[0])
    assert torch.equal(got, ref), name
    assert int(got.min()) > 0  # (a lossy decode of these images: a kernel that added nothing would not pass as "equal zeros")
    # one triple at a time gives the same rows (Q = 1 is lrf_qmf_encode_rgb_u8's layout)
    for q in (0, 3):
        assert torch.equal(ctx.sweep_sse(dev, [factors[q]], [TRIPLES[q]])[0], ref[q]), (name, q)
    big = lrf_amd.qmf_factorize_batch(dev, list(BIG), num_iters=10)
    got_big = ctx.sweep_sse(dev, [big], [BIG])
    ref_big = _reference(ctx, dev, [big], [BIG])
    print(name, BIG, got_big.tolist(), ref_big.tolist())
    assert torch.equal(got_big, ref_big), name
    # the public face
    assert torch.equal(lrf_amd.sweep_sse_batch(images, factors, TRIPLES), ref)


@pytest.mark.parametrize("hw", [(512, 768), (173, 264), (200, 992)])
def test_random_factors_saturate_and_still_agree(hw):
    """factors drawn from the whole int8 range within the bounds: the colour chain leaves [0, 255] on both sides, so the clamp
    (fmed3 + truncation) is what decides many bytes"""
    from lrf_amd import _lib
    ctx = _ctx()
    H, W = hw
    g = torch.Generator().manual_seed(H)
    dev = torch.randint(0, 256, (2, 3, H, W), dtype=torch.uint8, generator=g).cuda(ctx.device)
    triples = [(7, 3, 3), (16, 8, 8), (3, 2, 1), (40, 20, 20)]
    dims = _lib.plane_dims(H, W)
    factors = []
    for t in triples:
        nu, nv = sum(d[4] * r for d, r in zip(dims, t)), 64 * sum(t)
        factors.append((torch.randint(-16, 16, (2, nu), dtype=torch.int8, generator=g).cuda(ctx.device),
                        torch.randint(-16, 16, (2, nv), dtype=torch.int8, generator=g).cuda(ctx.device)))
    for (U, V), t in zip(factors, triples):
        dec = ctx.decode_rgb(U, V, H, W, list(t))
        assert int(dec.min()) == 0 and int(dec.max()) == 255, (hw, t)  # otherwise the clamp is untested
    got = ctx.sweep_sse(dev, factors, triples)  # (separate buffers: the binding lays them out back to back)
    ref = _reference(ctx, dev, factors, triples)
    print(hw, got.tolist(), ref.tolist())
    assert torch.equal(got, ref)


def test_against_the_cpu_oracle():
    """the oracle's decode of the same factors (numpy, int64 sums) gives the kernel's integers"""
    import lrf_amd
    from lrf_amd.codec import split_factors
    from oracle import oracle
    ctx = _ctx()
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (2, 3, 120, 200), dtype=torch.uint8, generator=g)
    img[1] = _nat()[:, 200:320, 300:500]
    dev = img.cuda(ctx.device)
    for t in [(7, 3, 3), (20, 10, 10)]:
        U, V = lrf_amd.qmf_factorize_batch(dev, list(t), num_iters=10)
        got = ctx.sweep_sse(dev, [(U, V)], [t])[0].tolist()
        for b in range(2):
            f = split_factors(U[b].cpu().numpy(), V[b].cpu().numpy(), (120, 200), list(t))
            ref = oracle.planes_to_rgb(f[0::2], f[1::2], 120, 200)
            want = int(((img[b].numpy().astype(np.int64) - ref.astype(np.int64)) ** 2).sum())
            print(t, b, got[b], want)
            assert got[b] == want


@pytest.mark.parametrize("hw", [(176, 256), (173, 264), (150, 992)])
def test_an_images_result_does_not_depend_on_batch_sweep_or_position(hw):
    ctx = _ctx()
    H, W = hw
    nat = _nat()
    imgs = torch.stack([nat[:, 37 * i:37 * i + H, 0:W] for i in range(5)]).contiguous()
    dev = imgs.cuda(ctx.device)
    triples = [(7, 3, 3), (2, 1, 1), (16, 8, 8), (26, 13, 13)]
    factors = ctx.encode_sweep_rgb(dev, triples, 10, -16, 15)
    t, (U, V) = triples[0], factors[0]
    in_batch = ctx.sweep_sse(dev, [(U, V)], [t])[0]
    first = ctx.sweep_sse(dev, factors, triples)[0]
    order = [1, 2, 3, 0]
    last = ctx.sweep_sse(dev, [factors[i] for i in order], [triples[i] for i in order])[3]
    alone = torch.cat([ctx.sweep_sse(dev[i:i + 1], [(U[i:i + 1], V[i:i + 1])], [t])[0] for i in range(5)])
    print(hw, alone.tolist(), in_batch.tolist(), first.tolist(), last.tolist())
    assert torch.equal(alone, in_batch) and torch.equal(alone, first) and torch.equal(alone, last)


def test_refusals():
    """NULL or misshapen buffers raise ValueError; nothing is launched (the squared-error buffer is never written)"""
    import ctypes

    from lrf_amd import _lib
    ctx = _ctx()
    dev = torch.zeros((2, 3, 64, 96), dtype=torch.uint8, device=f"cuda:{ctx.device}")
    t = (7, 3, 3)
    dims = _lib.plane_dims(64, 96)
    nu, nv = sum(d[4] * r for d, r in zip(dims, t)), 64 * sum(t)
    U = torch.zeros((2, nu), dtype=torch.int8, device=dev.device)
    V = torch.zeros((2, nv), dtype=torch.int8, device=dev.device)
    assert tuple(ctx.sweep_sse(dev, [(U, V)], [t]).shape) == (1, 2)  # (the valid call these are variations of)
    bad = [
        (dev, None, [t]), (dev, [(U, V)], None), (dev, [(None, V)], [t]), (dev, [(U, None)], [t]), (dev, [], []),
        (dev, [(U[:, :-1], V)], [t]), (dev, [(U, V[:, :-8])], [t]), (dev, [(U[:1], V[:1])], [t]), (dev, [(U, V), (U, V)], [t]),
        (dev, [(U, V)], [(7, 3)]), (dev, [(U, V)], [(0, 3, 3)]), (dev, [(U, V)], [(65, 3, 3)]), (dev[:, :2], [(U, V)], [t]),
        (dev, [(U.cpu(), V.cpu())], [t]), (dev.cpu(), [(U, V)], [t]),
    ]
    for rgb, f, tr in bad:
        with pytest.raises(ValueError):
            ctx.sweep_sse(rgb, f, tr)
    # the C entry point itself: NULL pointers, Q < 1, B and ranks out of range give LRF_EINVAL (-1) before anything is launched
    lib = ctx._lib
    sse = torch.full((2,), -5, dtype=torch.int64, device=dev.device)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    R = (ctypes.c_int * 3)(*t)
    R0 = (ctypes.c_int * 3)(7, 0, 3)
    R65 = (ctypes.c_int * 3)(65, 3, 3)
    calls = [
        (ctx._h, None, p(U), p(V), 2, 64, 96, 1, R, p(sse)), (ctx._h, p(dev), None, p(V), 2, 64, 96, 1, R, p(sse)),
        (ctx._h, p(dev), p(U), None, 2, 64, 96, 1, R, p(sse)), (ctx._h, p(dev), p(U), p(V), 2, 64, 96, 1, None, p(sse)),
        (ctx._h, p(dev), p(U), p(V), 2, 64, 96, 1, R, None), (None, p(dev), p(U), p(V), 2, 64, 96, 1, R, p(sse)),
        (ctx._h, p(dev), p(U), p(V), 2, 64, 96, 0, R, p(sse)), (ctx._h, p(dev), p(U), p(V), 0, 64, 96, 1, R, p(sse)),
        (ctx._h, p(dev), p(U), p(V), 65536, 64, 96, 1, R, p(sse)), (ctx._h, p(dev), p(U), p(V), 2, 64, 96, 1, R0, p(sse)),
        (ctx._h, p(dev), p(U), p(V), 2, 64, 96, 1, R65, p(sse)),
    ]
    for args in calls:
        assert lib.lrf_qmf_sweep_sse_rgb_u8(*args) == -1, args
    torch.cuda.synchronize()
    assert sse.tolist() == [-5, -5]
