"""Child process of tests/test_geometry_gpu.py: under LRF_PERSIST=1 and LRF_FUSED_GRAM_MIN_CHUNKS=1 (both read once per process)
factorises, for each of three small 16-aligned sizes, a batch large enough (tests/_luma_bytes_worker.py's rule) that the call forms
its patch matrices in k_planes16_gram and its k_bcd_p reads luma from the image bytes, and saves the images, U, V, the launch
counts and what lrf_ctx_last_luma_source said.  The parent compares every image with the CPU oracle on the planes of the
definition in tests/geometry_cases.py.

The tables at the top import nothing heavy: the test module reads them at collection time."""
import os
import sys

import numpy as np

SIZES = [(32, 32), (48, 48), (32, 48)]
RANKS, K, BOUNDS = (3, 2, 2), 2, (-16, 15)
MIN_BLOCKS = 1024


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import lrf_amd
    from _luma_bytes_worker import batch_size

    out = sys.argv[1]
    torch.cuda.set_device(0)
    ctx = lrf_amd._lib.context(0)
    res = {}
    for H, W in SIZES:
        B = batch_size(H, W, MIN_BLOCKS)
        g = torch.Generator().manual_seed(97 * H + W)
        imgs = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()
        assert imgs.data_ptr() % 8 == 0
        ctx.profile_kernels([lrf_amd._lib.LRF_K_BCD_PERSIST, lrf_amd._lib.LRF_K_PLANES_GRAM, lrf_amd._lib.LRF_K_PLANES])
        ctx.profile_reset()
        U, V = lrf_amd.qmf_factorize_batch(imgs, RANKS, num_iters=K, bounds=BOUNDS)
        torch.cuda.synchronize()
        counts = [ctx.kernel_time(k)[1] for k in (lrf_amd._lib.LRF_K_BCD_PERSIST, lrf_amd._lib.LRF_K_PLANES_GRAM, lrf_amd._lib.LRF_K_PLANES)]
        ctx.profile(False)
        key = f"{H}x{W}"
        res[key + "_images"], res[key + "_U"], res[key + "_V"] = imgs.cpu().numpy(), U.cpu().numpy(), V.cpu().numpy()
        res[key + "_launches"], res[key + "_source"] = np.array(counts), np.array(str(ctx.last_luma_source()))
        ctx.synchronize()  # raises if a poll of k_bcd_p expired
    ctx.check()
    np.savez(out, **res)
    print("DONE", flush=True)
