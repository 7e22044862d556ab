"""Child process of tests/test_bcdp_quads_gpu.py: factorises one geometry's batch at every case of the table under the
LRF_PERSIST setting the parent chose (the switch is read once per process) and saves, per case, U, V and the number of
LRF_K_BCD_PERSIST launches — and the images, so that the parent can ask the CPU oracle.

The tables at the top import nothing heavy: the test module reads them at collection time."""
import os
import sys

import numpy as np

D = (-16, 15)
# geometry -> (H, W, blocks the batch must reach).  173x264: luma M = 726 (a 384-row and a 342-row block), chroma M = 187; every
# plane ends in a partial sub-tile, planes start at U offsets that are no multiples of 16; 272 images = 1088 blocks.  24x40: luma
# M = 15, chroma M = 6: one sub-tile with few live rows (the MFMAs still consume all 64 tile rows), one block a plane.
GEOMS = {"odd": (173, 264, 1088), "tiny": (24, 40, 1024)}
# both quad counts and the 4 / 5 boundary, a padded last quad, launches whose waves alternate between one-quad and two-quad items
TRIPLES = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4), (5, 4, 1), (6, 2, 5), (7, 3, 3), (8, 8, 8)]
# K = 1: plan_bcd keeps a single iteration on the launch-per-iteration kernel (no persistent launch: both children run the
# same kernels); K = 2: the first-iteration body (old U = X W0) and one iteration on old int8 rows; K = 3: two of those
ITERS = (1, 2, 3)
# (ranks, bounds, K) of a geometry; (-128, 127): the Gauss-Seidel outside the exact-integer range, on one case
CASES = [(r, D, k) for r in TRIPLES for k in ITERS] + [((7, 3, 3), (-128, 127), 3)]


def case_name(ranks, bounds, K):
    return f"{tuple(ranks)} {tuple(bounds)} K={K}"


def expected_launches(K):
    return 1 if K >= 2 else 0


def batch_size(H, W, min_blocks):
    """images that make `min_blocks` blocks (one wave each: 384 rows of a plane's patch matrix)"""
    from lrf_amd import _lib
    per_image = sum((M + 383) // 384 for (_, _, _, _, M) in _lib.plane_dims(H, W))
    return (min_blocks + per_image - 1) // per_image


def build_images(B, H, W):
    """uint8 CUDA [B,3,H,W]: smooth plus noise, every fourth image uniform noise, an all-zero and a constant image"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(41 + H)
    base = torch.rand(B, 3, max(H // 8, 1), max(W // 8, 1), generator=g, device="cuda") * 255
    imgs = (torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
            + torch.randn(B, 3, H, W, generator=g, device="cuda") * 6).clamp(0, 255).to(torch.uint8)
    for b in range(2, B, 4):
        imgs[b] = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    imgs[0] = 0
    imgs[B - 1] = 99
    return imgs


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import lrf_amd

    geom, out = sys.argv[1], sys.argv[2]
    H, W, min_blocks = GEOMS[geom]
    B = batch_size(H, W, min_blocks)
    torch.cuda.set_device(0)
    imgs = build_images(B, H, W)
    ctx = lrf_amd._lib.context(0)
    res = {"images": imgs.cpu().numpy()}
    for i, (ranks, bounds, K) in enumerate(CASES):
        ctx.profile_kernels([lrf_amd._lib.LRF_K_BCD_PERSIST])
        ctx.profile_reset()
        U, V = lrf_amd.qmf_factorize_batch(imgs, ranks, num_iters=K, bounds=bounds)
        torch.cuda.synchronize()
        res[f"launches{i}"] = np.array(ctx.kernel_time(lrf_amd._lib.LRF_K_BCD_PERSIST)[1])
        ctx.profile(False)
        res[f"U{i}"] = U.cpu().numpy()
        res[f"V{i}"] = V.cpu().numpy()
        ctx.synchronize()  # raises if a poll of k_bcd_p expired
    ctx.check()
    np.savez(out, **res)
    print("DONE", geom, os.environ.get("LRF_PERSIST"), B, [int(res[f"launches{i}"]) for i in range(len(CASES))], flush=True)
