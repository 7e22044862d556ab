"""Child process of tests/test_encode_ragged_gpu.py: the ragged encode where the fast kernels run.  Started with LRF_PERSIST=1
in its environment (the plan settings are read once per process): with that hook the persistent kernel k_bcd_p takes a call from
1024 blocks.  One list of images of two sizes and two rank triples, large enough as ONE call and far too small per image; every
image against the uniform encoder called for it alone, four of them — one per (size, triple) — against the CPU oracle.
Prints one RESULT line of JSON and DONE."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

SIZES = [(512, 768), (384, 512)]
TRIPLES = [(7, 3, 3), (12, 6, 6)]
MIN_BLOCKS = 1024  # LRF_BCDW_MIN_BLOCKS: the persistent kernel's threshold under LRF_PERSIST=1, and k_bcd_w*'s
K, LO, HI = 10, -16, 15
LRF_K_BCD, LRF_K_BCD_PERSIST = 2, 6


def items():
    """48 images alternating the sizes, the triples alternating at half that rate (all four pairs occur), then further
    images in the same rotation until the call's plane table holds MIN_BLOCKS blocks of 384 rows -> [(H, W, triple)], blocks"""
    from lrf_amd import _lib
    out, blocks = [], 0
    while len(out) < 48 or blocks < MIN_BLOCKS:
        j = len(out)
        H, W = SIZES[j % 2]
        out.append((H, W, TRIPLES[(j // 2) % 2]))
        blocks += sum(-(-d[4] // 384) for d in _lib.plane_dims(H, W))
    return out, blocks


def main():
    import torch
    from conftest import make_image
    from lrf_amd import _lib
    from lrf_amd.codec import split_factors
    from oracle import oracle
    assert os.environ.get("LRF_PERSIST") == "1"
    its, blocks = items()
    n = len(its)
    imgs = [make_image(dict(kind="smooth", seed=700 + j, H=H, W=W)) for j, (H, W, _) in enumerate(its)]
    ctx = _lib.context(0)
    alone = []
    for im, (H, W, t) in zip(imgs, its):
        U, V = ctx.encode_rgb(im[None].cuda(), list(t), K, LO, HI)
        alone.append((U[0].cpu().numpy(), V[0].cpu().numpy()))
    offs, off = [], 0
    for im in imgs:
        offs.append(off)
        off = (off + im.numel() + 15) // 16 * 16
    flat = torch.zeros((off,), dtype=torch.uint8)
    for im, o in zip(imgs, offs):
        flat[o:o + im.numel()] = im.reshape(-1)
    flat = flat.cuda()
    ctx.profile(True)
    ctx.profile_reset()
    U, V, u_off, v_off = ctx.encode_ragged(flat, [(H, W, t, o) for (H, W, t), o in zip(its, offs)], K, LO, HI)
    persist, bcd = ctx.kernel_time(LRF_K_BCD_PERSIST)[1], ctx.kernel_time(LRF_K_BCD)[1]
    ctx.profile(False)
    Uh, Vh = (x.numpy() for x in ctx.to_host(U, V))
    bad = []
    for j, ((ua, va), uo, vo) in enumerate(zip(alone, u_off, v_off)):
        if not (np.array_equal(Uh[uo:uo + ua.size], ua) and np.array_equal(Vh[vo:vo + va.size], va)):
            bad.append(f"image {j} {its[j]}: differs from the uniform encoder alone")
    checked = []
    for want in [(s, t) for s in SIZES for t in TRIPLES]:
        j = next(j for j, (H, W, t) in enumerate(its) if ((H, W), t) == want)
        H, W, t = its[j]
        got = split_factors(Uh[u_off[j]:u_off[j] + alone[j][0].size], Vh[v_off[j]:v_off[j] + alone[j][1].size], (H, W), t)
        X = oracle.rgb_to_planes(imgs[j].numpy())
        for c in range(3):
            uo_, vo_ = oracle.qmf_decompose(X[c], t[c], K, (LO, HI))
            if not (np.array_equal(got[2 * c], uo_.astype(np.int8)) and np.array_equal(got[2 * c + 1], vo_.astype(np.int8))):
                bad.append(f"image {j} {its[j]} plane {c}: differs from the oracle")
        checked.append(j)
    err = ""
    try:
        ctx.synchronize()
        ctx.check()
    except Exception as e:  # noqa: BLE001
        err = repr(e)
    print("RESULT " + json.dumps(dict(images=n, blocks=blocks, persist=persist, bcd=bcd, nbad=len(bad), bad=bad[:10], oracle=checked, ctx=err)), flush=True)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
