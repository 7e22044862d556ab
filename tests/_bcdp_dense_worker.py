"""Child process of tests/test_bcdp_dense.py: factorises one geometry's batch at each of its rank triples under the LRF_PERSIST
setting the parent chose (the switch is read once per process) and saves U, V and the number of k_bcd_p launches per triple."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lrf_amd

# geometry -> (H, W, images, rank triples, iterations): the benchmark's batch on default thresholds, and a batch of 1088 blocks
# whose planes start at U offsets that are not multiples of 16, at ranks below 4, with a partial last sub-tile per plane
CASES = {
    "bench": (512, 768, 256, ((7, 3, 3), (4, 2, 2)), 10),
    "odd": (173, 264, 272, ((3, 2, 1), (2, 3, 3)), 4),
}

geom, out = sys.argv[1], sys.argv[2]
H, W, B, triples, K = CASES[geom]
torch.cuda.set_device(0)
g = torch.Generator(device="cuda").manual_seed(23)
base = torch.rand(B, 3, H // 8, W // 8, generator=g, device="cuda") * 255
imgs = (torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
        + torch.randn(B, 3, H, W, generator=g, device="cuda") * 6).clamp(0, 255).to(torch.uint8)
del base
ctx = lrf_amd._lib.context(0)
res = {}
for i, ranks in enumerate(triples):
    ctx.profile_kernels([lrf_amd._lib.LRF_K_BCD_PERSIST])
    ctx.profile_reset()
    U, V = lrf_amd.qmf_factorize_batch(imgs, ranks, num_iters=K)
    torch.cuda.synchronize()
    res[f"launches{i}"] = np.array(ctx.kernel_time(lrf_amd._lib.LRF_K_BCD_PERSIST)[1])
    ctx.profile(False)
    res[f"U{i}"] = U.cpu().numpy()
    res[f"V{i}"] = V.cpu().numpy()
ctx.synchronize()  # raises if a poll of k_bcd_p expired
np.savez(out, **res)
print("ok", geom, os.environ.get("LRF_PERSIST"), [int(res[f"launches{i}"]) for i in range(len(triples))], flush=True)
