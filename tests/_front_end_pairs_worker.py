"""Child process of tests/test_front_end_pairs_gpu.py: under the LRF_FUSED_GRAM_MIN_CHUNKS, LRF_LUMA_BYTES and LRF_PERSIST
settings the parent chose (all read once per process) prints one line per call with a digest of its int8 factors, then which
planes kernel ran and where k_bcd_p read luma from; saves the factors of ORACLE_CALL for the parent's comparison with the oracle.

The tables at the top import nothing heavy: the test module reads them."""
import hashlib
import os
import sys

# (H, W), ranks — what each size is the smallest case of, in k_planes16_gram's terms (a unit = 16 rows x 32 patch columns, a
# chunk = 384 luma rows at these batch sizes):
GEOMETRIES = (((16, 16), (1, 1, 1)),    # one unit, one chunk; 2 live patch columns of 32
              ((16, 528), (4, 2, 2)),   # three segments, the last with 2 live patch columns
              ((48, 272), (7, 3, 3)),   # three strips of two segments, the second ragged (2 live columns)
              ((112, 256), (7, 3, 3)),  # M = 448: two chunks of 3 and 4 units
              ((128, 256), (7, 3, 3)),  # two chunks of equal unit counts
              ((208, 256), (7, 3, 3)))  # M = 832: three chunks (4, 4, 5 units)
SMALL_BATCHES = (1, 2, 3)  # odd and even chunk totals
# a batch that LRF_PERSIST=1 puts on k_bcd_p (1024 blocks, three or more an image), whose rank <= 8 body reads luma from the
# image bytes unless LRF_LUMA_BYTES=0: the only calls that run k_planes16_gram<false>
PERSIST_BATCH = 344
ORACLE_CALL = ((112, 256), 3)


def build_images(B, H, W, seed):
    """smooth colour fields plus noise, saturated in places (zero and 255 bytes); the same bytes in the worker and in the parent"""
    import torch
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, H // 8 + 1, W // 8 + 1, generator=g) * 300 - 20
    return (torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
            + torch.randn(B, 3, H, W, generator=g) * 6).clamp(0, 255).to(torch.uint8)


def seed_of(H, W, B):
    return 100000 * B + 1000 * (H // 16) + W // 16


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import numpy as np
    import torch
    import lrf_amd
    from lrf_amd import _lib

    out = sys.argv[1]
    ctx = _lib.context(0)
    ctx.profile_kernels([_lib.LRF_K_PLANES_GRAM, _lib.LRF_K_PLANES, _lib.LRF_K_BCD_PERSIST])
    ctx.profile_reset()

    def digest(*tensors):
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    for (H, W), ranks in GEOMETRIES:
        for B in SMALL_BATCHES:
            U, V = lrf_amd.qmf_factorize_batch(build_images(B, H, W, seed_of(H, W, B)).cuda(), ranks)
            print("encode", (B, H, W), ranks, digest(U, V), flush=True)
            if ((H, W), B) == ORACLE_CALL:
                np.savez(out, U=U.cpu().numpy(), V=V.cpu().numpy())
    torch.cuda.synchronize()
    small = (ctx.kernel_time(_lib.LRF_K_PLANES_GRAM)[1], ctx.kernel_time(_lib.LRF_K_PLANES)[1], ctx.kernel_time(_lib.LRF_K_BCD_PERSIST)[1])
    sources = set()
    for (H, W), ranks in GEOMETRIES:
        imgs = build_images(PERSIST_BATCH, H, W, seed_of(H, W, PERSIST_BATCH)).cuda()
        assert imgs.data_ptr() % 8 == 0
        U, V = lrf_amd.qmf_factorize_batch(imgs, ranks)
        print("encode", (PERSIST_BATCH, H, W), ranks, digest(U, V), flush=True)
        sources.add(str(ctx.last_luma_source()))
    torch.cuda.synchronize()
    ctx.synchronize()  # raises if a poll of k_bcd_p expired
    ctx.check()
    n = (ctx.kernel_time(_lib.LRF_K_PLANES_GRAM)[1], ctx.kernel_time(_lib.LRF_K_PLANES)[1], ctx.kernel_time(_lib.LRF_K_BCD_PERSIST)[1])
    ctx.profile(False)
    print("launches: small k_planes16_gram %d k_planes16 %d k_bcd_p %d; persist k_planes16_gram %d k_planes16 %d k_bcd_p %d luma from %s"
          % (small + (n[0] - small[0], n[1] - small[1], n[2] - small[2], "/".join(sorted(sources)))), file=sys.stderr, flush=True)
