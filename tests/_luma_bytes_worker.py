"""Child process of tests/test_luma_bytes_gpu.py: under LRF_PERSIST=1 and the LRF_LUMA_BYTES setting the parent chose (both are
read once per process) factorises one geometry's batch at every case of the table and saves, per case, U, V, the number of
LRF_K_BCD_PERSIST launches and what lrf_ctx_last_luma_source said — and the images, so that the parent can ask the CPU oracle.
Job "fallback": the calls that must NOT take the path (sides that are no multiples of 16, a tensor one byte off 8-alignment, the
pipelined encoder), each beside the same images on the direct, aligned call.

The tables at the top import nothing heavy: the test module reads them at collection time."""
import os
import sys

import numpy as np

D = (-16, 15)
# geometry -> (H, W, blocks the batch must reach): the smallest sizes at which the row -> patch mapping can go wrong
#   48x80     luma M = 60: one partial sub-tile that spans six patch rows (nwl = 10); chroma M = 15; three blocks an image
#   128x208   nwl = 26; luma M = 416 = 384 + 32: a second block that starts mid patch row and is a 32-row partial sub-tile
#   32x1040   nwl = 130 > 64: sub-tiles inside one patch row and across its end; luma M = 520
GEOMS = {"48x80": (48, 80, 1024), "128x208": (128, 208, 1024), "32x1040": (32, 1040, 1024)}
TRIPLES = [(1, 1, 1), (4, 4, 4), (5, 4, 1), (7, 3, 3), (8, 8, 8)]
CASES = [(r, D, k) for r in TRIPLES for k in (2, 3)] + [((7, 3, 3), (-128, 127), 3)]
FALLBACK_ODD = (173, 264, 1088)  # not multiples of 16
FALLBACK_CASE = ((7, 3, 3), D, 3)


def case_name(ranks, bounds, K):
    return f"{tuple(ranks)} {tuple(bounds)} K={K}"


def batch_size(H, W, min_blocks):
    """images that make `min_blocks` blocks (one wave each: 384 rows of a plane's patch matrix)"""
    from lrf_amd import _lib
    per_image = sum((M + 383) // 384 for (_, _, _, _, M) in _lib.plane_dims(H, W))
    return (min_blocks + per_image - 1) // per_image


def oracle_images(B):
    """the images the parent compares with the CPU oracle: every eighth, the first (all zero) and the last (constant)"""
    return sorted(set(range(0, B, 8)) | {0, B - 1})


def build_images(B, H, W):
    """uint8 CUDA [B,3,H,W]: smooth plus noise, every fourth image uniform noise, an all-zero and a constant image"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(43 + H)
    base = torch.rand(B, 3, max(H // 8, 1), max(W // 8, 1), generator=g, device="cuda") * 255
    imgs = (torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
            + torch.randn(B, 3, H, W, generator=g, device="cuda") * 6).clamp(0, 255).to(torch.uint8)
    for b in range(2, B, 4):
        imgs[b] = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    imgs[0] = 0
    imgs[B - 1] = 99
    return imgs


def _call(ctx, lrf_amd, torch, imgs, ranks, bounds, K):
    """one call -> (U, V, persistent launches, luma source)"""
    ctx.profile_kernels([lrf_amd._lib.LRF_K_BCD_PERSIST])
    ctx.profile_reset()
    U, V = lrf_amd.qmf_factorize_batch(imgs, ranks, num_iters=K, bounds=bounds)
    torch.cuda.synchronize()
    n = ctx.kernel_time(lrf_amd._lib.LRF_K_BCD_PERSIST)[1]
    ctx.profile(False)
    src = str(ctx.last_luma_source())
    U, V = U.cpu().numpy(), V.cpu().numpy()
    ctx.synchronize()  # raises if a poll of k_bcd_p expired
    return U, V, n, src


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import lrf_amd

    job, out = sys.argv[1], sys.argv[2]
    torch.cuda.set_device(0)
    ctx = lrf_amd._lib.context(0)
    res = {}
    if job in GEOMS:
        H, W, min_blocks = GEOMS[job]
        imgs = build_images(batch_size(H, W, min_blocks), H, W)
        assert imgs.data_ptr() % 8 == 0
        res["images"] = imgs.cpu().numpy()
        for i, (ranks, bounds, K) in enumerate(CASES):
            res[f"U{i}"], res[f"V{i}"], n, src = _call(ctx, lrf_amd, torch, imgs, ranks, bounds, K)
            res[f"launches{i}"], res[f"source{i}"] = np.array(n), np.array(src)
    else:
        assert job == "fallback"
        ranks, bounds, K = FALLBACK_CASE
        # (a) sides that are no multiples of 16
        H, W, min_blocks = FALLBACK_ODD
        imgs = build_images(batch_size(H, W, min_blocks), H, W)
        res["odd_U"], res["odd_V"], n, src = _call(ctx, lrf_amd, torch, imgs, ranks, bounds, K)
        res["odd_launches"], res["odd_source"] = np.array(n), np.array(src)
        # (b) an eligible geometry: aligned, then the same bytes one byte off 8-alignment
        H, W, min_blocks = GEOMS["48x80"]
        imgs = build_images(batch_size(H, W, min_blocks), H, W)
        res["al_U"], res["al_V"], n, src = _call(ctx, lrf_amd, torch, imgs, ranks, bounds, K)
        res["al_launches"], res["al_source"] = np.array(n), np.array(src)
        flat = torch.empty(imgs.numel() + 8, dtype=torch.uint8, device="cuda")
        off = (1 - flat.data_ptr()) % 8  # so that the view starts at 1 mod 8
        shifted = flat[off:off + imgs.numel()].view(imgs.shape)
        shifted.copy_(imgs)
        assert shifted.data_ptr() % 8 == 1 and shifted.is_contiguous()
        res["off_U"], res["off_V"], n, src = _call(ctx, lrf_amd, torch, shifted, ranks, bounds, K)
        res["off_launches"], res["off_source"] = np.array(n), np.array(src)
        # (c) the pipelined encoder on the same images, the whole batch one sub-batch: its slots hand their upload buffer back
        # behind the planes kernel
        pipe = lrf_amd._lib.Pipe(0, slots=2, sub_batch=imgs.shape[0])
        host = imgs.cpu().pin_memory()
        Up, Vp = pipe.encode_rgb_host(host, list(ranks), K, bounds[0], bounds[1])
        res["pipe_U"], res["pipe_V"] = Up.numpy(), Vp.numpy()
        res["pipe_sources"] = np.array([str(pipe.slot_context(s).last_luma_source()) for s in range(pipe.slots)])
        pipe.close()
    ctx.check()
    np.savez(out, **res)
    print("DONE", job, os.environ.get("LRF_LUMA_BYTES"), flush=True)
