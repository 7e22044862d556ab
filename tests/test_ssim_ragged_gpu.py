"""GPU suite (-m gpu): squared error and SSIM of items that differ in size and ranks, scored from their factors
(Context.ssim_ragged, lrf_qmf_ssim_ragged_rgb_u8), against Context.decode_ragged on the same descriptors followed by
image_metrics_batch(source[None], decoded[None]) per item — bit for bit, the SSIM compared as int64 views.  The item list is
tests/test_sse_ragged_gpu.py's (random int8 factors, random sources at odd offsets, sources shared): every decode body and every
rank class, the 16x16 item included (16 >= 7: the metric takes it)."""
import ctypes

import pytest
import torch

from test_sse_ragged_gpu import ITEMS, Made

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).tolist()


class Ref:
    """decode_ragged + image_metrics_batch per item: computed once, left unchanged"""
    _ref = None

    @classmethod
    def get(cls):
        if cls._ref is None:
            import lrf_amd
            ctx, U, V, rgb, items, dec, want = Made.get()
            ms = []
            for (H, W, _, _, _, so), d in zip(items, dec):
                src = rgb[so:so + 3 * H * W].view(1, 3, H, W).clone()
                ms.append(lrf_amd.image_metrics_batch(src, d[None].contiguous()))
            cls._ref = (torch.cat([m["sse"] for m in ms]).cpu(), torch.cat([m["ssim"] for m in ms]).cpu())
        return cls._ref


def test_every_item_equals_decode_then_metrics():
    ctx, U, V, rgb, items, dec, want = Made.get()
    ref_sse, ref_ssim = Ref.get()
    sse, ssim = ctx.ssim_ragged(rgb, items, U, V)
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and sse.is_cuda and tuple(ssim.shape) == (len(items),)
    print("ssim", ssim.tolist(), "decode + uniform", ref_ssim.tolist())
    assert sse.tolist() == ref_sse.tolist() == want
    assert bits(ssim) == bits(ref_ssim)
    assert len(items) == len(ITEMS) and (16, 16) in {it[:2] for it in items}
    assert bool(torch.isfinite(ssim).all()) and len(set(bits(ssim))) == len(items)  # nothing is trivially equal


def test_squared_error_equals_sse_ragged():
    ctx, U, V, rgb, items, dec, want = Made.get()
    assert ctx.ssim_ragged(rgb, items, U, V)[0].tolist() == ctx.sse_ragged(rgb, items, U, V).tolist()


def test_the_scratch_cap_changes_nothing():
    ctx, U, V, rgb, items, dec, want = Made.get()
    ref_sse, ref_ssim = Ref.get()
    one = (3 * 64 * 64 + 15) // 16 * 16  # one 64x64 item: the five of them a chunk each, the smaller items in twos and threes
    for cap in (1, one, 2 * one + 5, 0):
        sse, ssim = ctx.ssim_ragged(rgb, items, U, V, scratch_bytes=cap)
        assert sse.tolist() == ref_sse.tolist() and bits(ssim) == bits(ref_ssim), cap


def test_order_and_neighbours_do_not_matter():
    ctx, U, V, rgb, items, dec, want = Made.get()
    ref_sse, ref_ssim = Ref.get()
    perm = torch.randperm(len(items), generator=torch.Generator().manual_seed(3)).tolist()
    sse, ssim = ctx.ssim_ragged(rgb, [items[i] for i in perm], U, V, scratch_bytes=40000)
    assert sse.tolist() == [ref_sse[i].item() for i in perm] and bits(ssim) == [bits(ref_ssim)[i] for i in perm]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        sse, ssim = ctx.ssim_ragged(rgb, items, U, V, scratch_bytes=40000)
    s.synchronize()
    assert sse.tolist() == ref_sse.tolist() and bits(ssim) == bits(ref_ssim)


def test_trim_frees_the_scratch():
    ctx, U, V, rgb, items, dec, want = Made.get()
    ref_sse, ref_ssim = Ref.get()
    ctx.trim()
    assert ctx.workspace_bytes() == 0
    ctx.ssim_ragged(rgb, items, U, V, scratch_bytes=40000)
    small = ctx.workspace_bytes()
    ctx.ssim_ragged(rgb, items, U, V)
    total = sum((3 * H * W + 15) // 16 * 16 for H, W, *_ in items)
    assert ctx.workspace_bytes() >= total > 40000 and ctx.workspace_bytes() - small >= total - 40000  # one chunk: every decoded image at once
    ctx.trim()
    assert ctx.workspace_bytes() == 0
    sse, ssim = ctx.ssim_ragged(rgb, items, U, V)  # and the next call allocates again
    assert sse.tolist() == ref_sse.tolist() and bits(ssim) == bits(ref_ssim)


def test_refusals_launch_nothing():
    from lrf_amd import _lib
    ctx, U, V, rgb, items, dec, want = Made.get()
    ref_sse, ref_ssim = Ref.get()
    lib = _lib.load()
    sse = torch.full((4,), 0x5A5A, dtype=torch.int64, device="cuda")
    ssim = torch.full((4,), 0.25, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(n, descs, scratch=0, rgb_len=None, out=sse, want_=ssim):
        desc = (_lib.RaggedImage * max(1, len(descs)))()
        for d, (H, W, t, uo, vo, ro) in zip(desc, descs):
            d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, uo, vo, ro
            d.R[0], d.R[1], d.R[2] = t
        ctx.use_torch_stream()
        return lib.lrf_qmf_ssim_ragged_rgb_u8(ctx._h, n, desc, ptr(U), U.numel(), ptr(V), V.numel(), ptr(rgb), rgb.numel() if rgb_len is None else rgb_len,
                                              scratch, ptr(out), ptr(want_))
    ok = items[:3]
    H, W, t, uo, vo, ro = ok[2]
    einval = {
        "6 rows": call(3, ok[:2] + [(6, 64, (1, 1, 1), 0, 0, 0)]),
        "6 columns": call(3, ok[:2] + [(64, 6, (1, 1, 1), 0, 0, 0)]),
        "source range": call(3, ok[:2] + [(H, W, t, uo, vo, rgb.numel() - 3 * H * W + 1)]),
        "rgb_len short": call(3, ok, rgb_len=ro + 3 * H * W - 1),
        "negative source": call(3, ok[:2] + [(H, W, t, uo, vo, -1)]),
        "rank 0": call(3, ok[:2] + [(H, W, (8, 0, 8), uo, vo, ro)]),
        "u range": call(3, ok[:2] + [(H, W, t, U.numel(), vo, ro)]),
        "negative scratch": call(3, ok, scratch=-1),
        "n = 0": call(0, ok),
        "NULL sse": call(3, ok, out=None),
        "NULL ssim": call(3, ok, want_=None),
    }
    assert all(rc == -1 for rc in einval.values()), einval
    torch.cuda.synchronize()
    assert bool((sse == 0x5A5A).all()) and bool((ssim == 0.25).all()), "a refused call wrote to its output"
    assert call(3, ok) == 0
    assert sse[:3].tolist() == ref_sse[:3].tolist() and bits(ssim[:3]) == bits(ref_ssim[:3])
    assert sse[3].item() == 0x5A5A and ssim[3].item() == 0.25
    for bad in ([(6, 64, (1, 1, 1), 0, 0, 0)], [ok[0][:5] + (rgb.numel(),)], []):
        with pytest.raises(ValueError):
            ctx.ssim_ragged(rgb, bad, U, V)
    with pytest.raises(ValueError):
        ctx.ssim_ragged(rgb, ok, U, V, scratch_bytes=-1)
    with pytest.raises(TypeError):
        ctx.ssim_ragged(rgb, ok, U.float(), V)
