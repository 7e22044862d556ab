"""Child process of tests/test_encode_ragged_sweep_gpu.py: the ragged sweep encode under the environment switches that choose
kernels (the plan settings are read once per process, so every setting takes a fresh process).  The small list of the parent test
— four images, candidate lists of lengths 1 to 5, interleaved — against Context.encode_ragged called for every (image, triple)
alone; with LRF_PERSIST=1 also a list that is 1152 blocks as ONE call (seven images at the eight candidates of ranks <= 8), where
the persistent kernel takes all K iterations in one launch and each candidate alone is 12 or 24 blocks.
Prints one RESULT line of JSON and DONE."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

K, LO, HI = 10, -16, 15
LRF_K_BCD, LRF_K_BCD_PERSIST = 2, 6
SIZES = [(48, 64), (40, 56), (33, 47), (64, 64)]
# lengths 3, 1, 2, 5: image 0 spans the three rank families, image 2 shares a chroma rank between its candidates, image 3 has its
# largest luma rank and its largest chroma rank in different candidates
CANDS = [[(4, 2, 2), (12, 6, 6), (20, 10, 10)], [(7, 3, 3)], [(4, 2, 2), (6, 2, 2)], [(9, 4, 4), (3, 1, 1), (17, 8, 8), (8, 8, 8), (16, 12, 5)]]
BIG_SIZES = [(512, 768)] * 5 + [(384, 512)] * 2
BIG_CANDS = [(r, max(r // 2, 1), max(r // 2, 1)) for r in range(1, 9)]


def content(j, H, W):
    """seeded smooth-plus-noise content (conftest.make_image's recipe needs sides of 8 or more to interpolate from)"""
    from conftest import make_image
    Hs, Ws = -(-H // 8) * 8, -(-W // 8) * 8
    return make_image(dict(kind="smooth", seed=900 + j, H=Hs, W=Ws))[:, :H, :W].contiguous()


def interleaved(cand_lists):
    """[(image, triple)]: the candidates of the images round-robin, so that no image's candidates stand together"""
    return [(i, cand_lists[i][k]) for k in range(max(len(c) for c in cand_lists)) for i in range(len(cand_lists)) if k < len(cand_lists[i])]


def flat_of(imgs):
    import torch
    offs, off = [], 0
    for im in imgs:
        offs.append(off)
        off = (off + im.numel() + 15) // 16 * 16
    flat = torch.zeros((off,), dtype=torch.uint8)
    for im, o in zip(imgs, offs):
        flat[o:o + im.numel()] = im.reshape(-1)
    return flat.cuda(), offs


def alone(ctx, imgs, sizes, pairs, k, signs=None):
    """Context.encode_ragged for every (image, triple) of `pairs` alone -> [(U, V) numpy]; signs: per image its int8 array at the
    image's largest ranks [Rmax_Y + Rmax_Cb + Rmax_Cr], a candidate takes the leading signs of its ranks"""
    import torch
    out = []
    for i, t in pairs:
        sg = None
        if signs is not None and signs[i] is not None:
            full, rmax = signs[i]
            cut, at = [], 0
            for ch in range(3):
                cut.append(full[at:at + t[ch]])
                at += rmax[ch]
            sg = torch.from_numpy(np.concatenate(cut)).cuda()
        H, W = sizes[i]
        U, V, _, _ = ctx.encode_ragged(imgs[i].reshape(-1).cuda(), [(H, W, t, 0, 0 if sg is not None else -1)], k, LO, HI, sg)
        out.append((U.cpu().numpy(), V.cpu().numpy()))
    return out


def sweep(ctx, imgs, sizes, pairs, k, signs=None):
    """Context.encode_ragged_sweep of the list -> [(U, V) numpy] per candidate"""
    import torch
    flat, offs = flat_of(imgs)
    sign, sign_offs = None, [-1] * len(imgs)
    if signs is not None:
        parts, so = [], 0
        for i, s in enumerate(signs):
            if s is not None:
                sign_offs[i] = so
                parts.append(s[0])
                so += s[0].size
        sign = torch.from_numpy(np.concatenate(parts)).cuda()
    U, V, u_off, v_off = ctx.encode_ragged_sweep(flat, [(H, W, o, s) for (H, W), o, s in zip(sizes, offs, sign_offs)], [(i, list(t)) for i, t in pairs],
                                                 k, LO, HI, sign)
    Uh, Vh = (x.numpy() for x in ctx.to_host(U, V))
    return [(Uh[a:b], Vh[c:d]) for a, b, c, d in zip(u_off, u_off[1:] + [Uh.size], v_off, v_off[1:] + [Vh.size])]


def differing(got, want, pairs):
    return [f"candidate {j} (image {pairs[j][0]}, {pairs[j][1]})" for j, (g, w) in enumerate(zip(got, want))
            if not (g[0].shape == w[0].shape and g[1].shape == w[1].shape and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]))]


def main():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    imgs = [content(j, H, W) for j, (H, W) in enumerate(SIZES)]
    pairs = interleaved(CANDS)
    bad = differing(sweep(ctx, imgs, SIZES, pairs, K), alone(ctx, imgs, SIZES, pairs, K), pairs)
    res = dict(cands=len(pairs), bad=bad[:10], nbad=len(bad), big=0, persist=-1, bcd=-1)
    if os.environ.get("LRF_PERSIST") == "1":
        imgs = [content(20 + j, H, W) for j, (H, W) in enumerate(BIG_SIZES)]
        pairs = interleaved([BIG_CANDS] * len(BIG_SIZES))
        want = alone(ctx, imgs, BIG_SIZES, pairs, K)
        ctx.profile(True)
        ctx.profile_reset()
        got = sweep(ctx, imgs, BIG_SIZES, pairs, K)
        res["persist"], res["bcd"] = ctx.kernel_time(LRF_K_BCD_PERSIST)[1], ctx.kernel_time(LRF_K_BCD)[1]
        ctx.profile(False)
        big_bad = differing(got, want, pairs)
        res.update(big=len(pairs), nbad=len(bad) + len(big_bad), bad=(bad + ["big list: " + b for b in big_bad])[:10])
        res["blocks"] = sum(sum(-(-d[4] // 384) for d in _lib.plane_dims(*BIG_SIZES[i])) for i, _ in pairs)
    err = ""
    try:
        ctx.synchronize()
        ctx.check()
    except Exception as e:  # noqa: BLE001
        err = repr(e)
    res["ctx"] = err
    print("RESULT " + json.dumps(res), flush=True)
    print("DONE", flush=True)


if __name__ == "__main__":
    main()
