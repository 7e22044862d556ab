"""Child process of tests/test_x_residency_gpu.py: under the LRF_PERSIST, LRF_LUMA_BYTES and LRF_X_KEEP_MB settings the parent
chose (all read once per process) factorises one case's batch and saves U, V, the number of LRF_K_BCD_PERSIST launches and
what lrf_ctx_last_luma_source and lrf_ctx_last_x_residency said.

The table at the top imports nothing heavy: the test module reads it at collection time."""
import os
import sys

import numpy as np

# case -> (images, H, W, ranks, K, LRF_LUMA_BYTES)
#   small   256 x 208x176: luma 572 rows (384 + 188), chroma 143: four blocks an image, 1024 in all — the smallest call
#           LRF_PERSIST=1 puts on the persistent kernel; luma and chroma blocks both end in a ragged sub-tile; luma from the bytes
#   fp32    44 x 512x768 with LRF_LUMA_BYTES=0 (1056 blocks): the fall-back whose luma blocks read fp32 X, streamed non-temporal
CASES = {"small": (256, 208, 176, (7, 3, 3), 3, "1"), "fp32": (44, 512, 768, (7, 3, 3), 3, "0")}


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import lrf_amd
    from _luma_bytes_worker import build_images

    case, out = sys.argv[1], sys.argv[2]
    B, H, W, ranks, K, _ = CASES[case]
    torch.cuda.set_device(0)
    ctx = lrf_amd._lib.context(0)
    assert ctx.last_x_residency() is None
    imgs = build_images(B, H, W)
    assert imgs.data_ptr() % 8 == 0
    ctx.profile_kernels([lrf_amd._lib.LRF_K_BCD_PERSIST])
    ctx.profile_reset()
    U, V = lrf_amd.qmf_factorize_batch(imgs, ranks, num_iters=K)
    torch.cuda.synchronize()
    launches = ctx.kernel_time(lrf_amd._lib.LRF_K_BCD_PERSIST)[1]
    ctx.profile(False)
    kept = ctx.last_x_residency()
    src = str(ctx.last_luma_source())
    # a second call on the same context: the tables of the first are resident, the factors must not depend on that
    U2, V2 = lrf_amd.qmf_factorize_batch(imgs, ranks, num_iters=K)
    torch.cuda.synchronize()
    U, V, U2, V2 = U.cpu().numpy(), V.cpu().numpy(), U2.cpu().numpy(), V2.cpu().numpy()
    ctx.synchronize()  # raises if a poll of k_bcd_p expired
    ctx.check()
    np.savez(out, U=U, V=V, U2=U2, V2=V2, launches=np.array(launches), source=np.array(src), kept=np.array(kept, dtype=np.int64),
             images_sum=np.array(int(imgs.sum().item())))
    print("DONE", case, os.environ.get("LRF_PERSIST"), os.environ.get("LRF_X_KEEP_MB"), flush=True)
