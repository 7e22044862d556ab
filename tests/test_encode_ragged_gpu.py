"""GPU suite (-m gpu): the ragged encode — images that differ in size and ranks in one call (Context.encode_ragged,
lrf_amd.qmf_encode_ragged) — against the uniform encoder called for each image alone, the CPU oracle and the reference's own
byte streams.  Everything is compared bitwise."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import Case, make_image

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# 32x272: 16-aligned, 34 luma patches per row = two workgroups per strip, the second partial; 64x96: 16-aligned; 40x272, 24x48:
# strip body <2,2>; 45x61: <3,3>; 173x264: <3,2>.  In this order neighbours (the last and the first too) differ in body.
SIZES = [(32, 272), (40, 272), (45, 61), (64, 96), (24, 48), (173, 264)]
BODY = {(32, 272): "tile16", (64, 96): "tile16", (40, 272): "strip22", (24, 48): "strip22", (45, 61): "strip33", (173, 264): "strip32"}
TRIPLES = [(1, 1, 1), (7, 3, 3), (8, 8, 5), (12, 6, 6), (16, 9, 16), (26, 13, 13), (32, 16, 16)]
K, LO, HI = 10, -16, 15
fam = lambda r: 0 if r <= 8 else (1 if r <= 16 else 2)


def eligible(H, W):
    """the triples the uniform encoder takes for this size with every rank within what qmf_ranks can give, R_c <= min(M_c, 64)"""
    from lrf_amd import _lib
    return [t for t in TRIPLES if all(r <= min(d[4], 64) for d, r in zip(_lib.plane_dims(H, W), t))]


def _mixed_list():
    """18 (H, W, triple): every size three times, each time with another of its eligible triples, dealt so that most neighbours
    differ in the luma rank family and all of them in body"""
    per_size = {hw: eligible(*hw) for hw in SIZES}
    # each size keeps at least two triples (24x48, whose chroma planes have six patches, keeps three; 45x61 four; the others all seven)
    assert all(len(v) >= 2 for v in per_size.values()) and [len(per_size[hw]) for hw in SIZES] == [7, 7, 4, 7, 3, 7]
    items = []
    for j in range(18):
        hw = SIZES[j % 6]
        el = per_size[hw]
        items.append((hw[0], hw[1], el[(3 * (j % 6) + 5 * (j // 6) + 5) % len(el)]))
    assert all(BODY[a[:2]] != BODY[b[:2]] for a, b in zip(items, items[1:]))
    assert len(set(items)) == 18 and {t for _, _, t in items} == set(TRIPLES)
    assert sum(fam(a[2][0]) != fam(b[2][0]) for a, b in zip(items, items[1:])) == 16  # of 17 neighbour pairs
    return items


def _content(j, H, W):
    if j == 7:
        return make_image(dict(kind="const", value=93, H=H, W=W))
    if j % 2:
        return make_image(dict(kind="randint", seed=500 + j, H=H, W=W))
    return make_image(dict(kind="smooth", seed=500 + j, H=max(H, 8), W=max(W, 8)))[:, :H, :W].contiguous()


class Mixed:
    """the 18 images and each one's factors from the uniform encoder called for it alone (B = 1): made once"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from lrf_amd import _lib
            ctx = _lib.context(0)
            items = _mixed_list()
            imgs = [_content(j, H, W) for j, (H, W, _) in enumerate(items)]
            alone = []
            for im, (H, W, t) in zip(imgs, items):
                U, V = ctx.encode_rgb(im[None].cuda(), list(t), K, LO, HI)
                alone.append((U[0].cpu().numpy(), V[0].cpu().numpy()))
            cls._made = (ctx, items, imgs, alone)
        return cls._made


def _ragged(ctx, items, imgs, order, signs=None):
    """encode_ragged of the images in `order` -> [(U, V) numpy] in that order"""
    offs, off = [], 0
    for i in order:
        offs.append(off)
        off = (off + imgs[i].numel() + 15) // 16 * 16
    flat = torch.zeros((off,), dtype=torch.uint8)
    for i, o in zip(order, offs):
        flat[o:o + imgs[i].numel()] = imgs[i].reshape(-1)
    U, V, u_off, v_off = ctx.encode_ragged(flat.cuda(), [(items[i][0], items[i][1], items[i][2], o) for i, o in zip(order, offs)], K, LO, HI)
    Uh, Vh = (x.numpy() for x in ctx.to_host(U, V))
    ends_u, ends_v = u_off[1:] + [Uh.size], v_off[1:] + [Vh.size]
    return [(Uh[a:b], Vh[c:d]) for a, b, c, d in zip(u_off, ends_u, v_off, ends_v)]


def _same(got, want):
    return got[0].shape == want[0].shape and got[1].shape == want[1].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_mixed_list_equals_the_uniform_encoder_and_the_oracle_image_by_image(oracle):
    from lrf_amd.codec import split_factors
    ctx, items, imgs, alone = Mixed.get()
    got = _ragged(ctx, items, imgs, range(len(items)))
    for i, (g, a) in enumerate(zip(got, alone)):
        assert _same(g, a), (i, items[i])
    for i, (H, W, t) in enumerate(items):  # and the CPU oracle: every image (0.23 Mpixel of planes in all)
        f = split_factors(got[i][0], got[i][1], (H, W), t)
        X = oracle.rgb_to_planes(imgs[i].numpy())
        for c in range(3):
            uo, vo = oracle.qmf_decompose(X[c], t[c], K, (LO, HI))
            assert np.array_equal(f[2 * c], uo.astype(np.int8)) and np.array_equal(f[2 * c + 1], vo.astype(np.int8)), (i, items[i], c)


def test_reversed_order_gives_the_same_bytes_per_image():
    ctx, items, imgs, alone = Mixed.get()
    order = list(range(len(items)))[::-1]
    for i, g in zip(order, _ragged(ctx, items, imgs, order)):
        assert _same(g, alone[i]), (i, items[i])


def test_one_image():
    ctx, items, imgs, alone = Mixed.get()
    bodies = [BODY[it[:2]] for it in items]
    for i in [bodies.index(b) for b in ("tile16", "strip22", "strip33", "strip32")] + [len(items) - 1]:
        assert _same(_ragged(ctx, items, imgs, [i])[0], alone[i]), items[i]


def test_uniform_list_equals_one_uniform_batch():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    H, W, t = 64, 96, (7, 3, 3)
    g = torch.Generator().manual_seed(5)
    batch = torch.randint(0, 256, (5, 3, H, W), dtype=torch.uint8, generator=g)
    Ub, Vb = (x.cpu() for x in ctx.encode_rgb(batch.cuda(), list(t), K, LO, HI))
    U, V, u_off, v_off = ctx.encode_ragged(batch.reshape(-1).cuda(), [(H, W, t, b * 3 * H * W) for b in range(5)], K, LO, HI)
    assert u_off == [b * Ub.shape[1] for b in range(5)] and v_off == [b * Vb.shape[1] for b in range(5)]
    assert torch.equal(U.cpu().view(5, -1), Ub) and torch.equal(V.cpu().view(5, -1), Vb)


def test_reference_byte_streams_with_their_signs_in_one_call_per_num_iters():
    """the fixtures of EXACT_CASES that use default kwargs, grouped by num_iters: with the reference's LAPACK signs passed per image
    the ragged encoder emits every fixture's byte stream"""
    import lrf_amd
    groups = {10: ["tiny_q7", "tiny_r7", "tiny_rank2", "odd_q7", "odd_r7", "smooth_q7", "smooth_r7", "nat_q7", "nat_r7", "s2odd_q7"],
              1: ["tiny_it1"], 2: ["tiny_it2"]}
    for iters, names in groups.items():
        cases = [Case(n) for n in names]
        assert all(c.kwargs.get("num_iters", 10) == iters and set(c.kwargs) <= {"rank", "quality", "num_iters"} for c in cases)
        out = lrf_amd.qmf_encode_ragged([c.image for c in cases], ranks=[c.ranks for c in cases], num_iters=iters,
                                        init_sign=[np.concatenate(c.signs()) for c in cases])
        for c, s in zip(cases, out):
            assert s == c.encoded, c.name
    cases = [Case(n) for n in ("tiny_q7", "odd_q7", "s2odd_q7")]  # and through `quality`, one value for all
    out = lrf_amd.qmf_encode_ragged([c.image for c in cases], quality=7, init_sign=[np.concatenate(c.signs()) for c in cases])
    assert [s == c.encoded for c, s in zip(cases, out)] == [True] * 3


def test_streams_and_round_trip():
    """qmf_encode_ragged's streams are qmf_encode_batch's per image (host and device images, a triple above rank 32 among them),
    and qmf_decode_ragged of them is qmf_decode of qmf_encode per image"""
    import lrf_amd
    ctx, items, imgs, alone = Mixed.get()
    pick = [0, 1, 2, 5, 10, 7]
    ims = [imgs[i] for i in pick] + [imgs[3]]
    triples = [list(items[i][2]) for i in pick] + [[40, 20, 20]]  # the last: outside the fused call, the uniform route
    streams = lrf_amd.qmf_encode_ragged(ims, ranks=triples)
    for im, t, s in zip(ims, triples, streams):
        assert s == lrf_amd.qmf_encode_batch(im[None], rank=t)[0], (tuple(im.shape), t)
    assert lrf_amd.qmf_encode_ragged([im.cuda() for im in ims], ranks=triples) == streams
    dec = lrf_amd.qmf_decode_ragged(streams)
    for im, t, d in zip(ims, triples, dec):
        assert torch.equal(d.cpu(), lrf_amd.qmf_decode(lrf_amd.qmf_encode(im, rank=t))), (tuple(im.shape), t)
    by_quality = lrf_amd.qmf_encode_ragged(ims[:3], quality=[3, 10, 20])
    for im, q, s in zip(ims, (3, 10, 20), by_quality):
        assert s == lrf_amd.qmf_encode_batch(im[None], quality=q)[0]


def test_c_entry_refuses_on_the_host_and_launches_nothing():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    lib = _lib.load()
    H, W, ranks = 64, 96, (7, 3, 3)
    dims = _lib.plane_dims(H, W)
    nu, nv, npx, ns = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks), 3 * H * W, sum(ranks)
    U = torch.full((2 * nu,), 0x5A, dtype=torch.int8, device="cuda")
    V = torch.full((2 * nv,), 0x5A, dtype=torch.int8, device="cuda")
    g = torch.Generator().manual_seed(2)
    rgb = torch.randint(0, 256, (2 * npx,), dtype=torch.uint8, generator=g).cuda()
    sign = torch.ones((2 * ns,), dtype=torch.int8, device="cuda")

    def call(n, images, K=10, lo=-16, hi=15, u_len=2 * nu, v_len=2 * nv, rgb_len=2 * npx, sign_len=2 * ns, u=U, v=V, src=rgb, sg=sign):
        desc = (_lib.RaggedEncodeImage * max(1, len(images or [])))()
        for d, (h, w, r, ro, uo, vo, so) in zip(desc, images or []):
            d.H, d.W, d.rgb_off, d.u_off, d.v_off, d.sign_off = h, w, ro, uo, vo, so
            d.R[0], d.R[1], d.R[2] = r
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ctx.use_torch_stream()
        return lib.lrf_qmf_encode_ragged_rgb_u8(ctx._h, n, desc if images is not None else None, ptr(src), rgb_len, K, lo, hi, ptr(sg), sign_len,
                                                ptr(u), u_len, ptr(v), v_len)

    ok = [(H, W, ranks, 0, 0, 0, 0), (H, W, ranks, npx, nu, nv, -1)]
    second = lambda **kw: [ok[0], tuple(kw.get(k, x) for k, x in zip(("H", "W", "R", "rgb", "u", "v", "s"), ok[1]))]
    einval = {
        "u range": call(2, ok, u_len=2 * nu - 1),
        "v range": call(2, ok, v_len=2 * nv - 1),
        "rgb range": call(2, ok, rgb_len=2 * npx - 1),
        "sign range": call(2, second(s=2 * ns - ns + 1)),
        "u offset past the end": call(2, second(u=nu + 1)),
        "v offset past the end": call(2, second(v=nv + 1)),
        "rgb offset past the end": call(2, second(rgb=npx + 1)),
        "negative u": call(2, second(u=-1)),
        "negative v": call(2, second(v=-1)),
        "negative rgb": call(2, second(rgb=-16)),
        "sign offset -2": call(2, second(s=-2)),
        "offset near 2^63": call(2, second(u=2 ** 63 - 1)),
        "U ranges overlap": call(2, second(u=nu - 1)),
        "V ranges overlap": call(2, second(v=0)),
        "rank 0": call(2, second(R=(7, 0, 3))),
        "n = 0": call(0, ok),
        "n = 65536": call(65536, ok),
        "no size": call(2, second(H=0)),
        "1x1": call(2, second(H=1, W=1)),  # the chroma plane would be empty: make_geom refuses it
        "bounds outside int8": call(2, ok, hi=128),
        "lo > hi": call(2, ok, lo=3, hi=2),
        "NULL images": call(2, None),
        "NULL rgb": call(2, ok, src=None),
        "NULL U": call(2, ok, u=None),
        "NULL V": call(2, ok, v=None),
    }
    assert all(rc == -1 for rc in einval.values()), einval
    enotsup = {
        "rank 33": call(2, second(R=(33, 3, 3))),
        "rank 65": call(2, second(R=(65, 3, 3))),
        "K = 0": call(2, ok, K=0),
        "an image of 2^31 / 3 pixels or more": call(2, second(H=30000, W=30000)),
    }
    assert all(rc == -2 for rc in enotsup.values()), enotsup
    torch.cuda.synchronize()
    assert bool((U == 0x5A).all()) and bool((V == 0x5A).all()), "a refused call wrote to its output"
    assert call(2, ok) == 0  # and the same call with the arguments right runs
    assert call(2, ok, sg=None, sign_len=0) == 0  # a NULL sign: default signs for every image, whatever its sign_off
    torch.cuda.synchronize()
    assert not bool((U == 0x5A).all()) and not bool((V == 0x5A).all())
    with pytest.raises(ValueError):
        ctx.encode_ragged(rgb, [(H, W, ranks, npx + 1)], K, LO, HI)
    with pytest.raises(ValueError):
        ctx.encode_ragged(rgb, [(H, W, (7, 3, 33), 0)], K, LO, HI)
    with pytest.raises(ValueError):
        ctx.encode_ragged(rgb, [], K, LO, HI)
    with pytest.raises(TypeError):
        ctx.encode_ragged(rgb.float(), [(H, W, ranks, 0)], K, LO, HI)


def test_table_survives_trim_and_a_changed_list():
    """the device table is cached on the descriptor bytes: a repeated call, a different list and a call after trim all encode right"""
    ctx, items, imgs, alone = Mixed.get()
    for order in ([0, 1, 2], [0, 1, 2], [2, 1, 0], [5]):
        for i, g in zip(order, _ragged(ctx, items, imgs, order)):
            assert _same(g, alone[i])
    ctx.trim()
    for i, g in zip([0, 1, 2], _ragged(ctx, items, imgs, [0, 1, 2])):
        assert _same(g, alone[i])


def test_fast_kernel_regime_in_a_child_process():
    """tests/_encode_ragged_worker.py with LRF_PERSIST=1: 57 images of two sizes and two triples are 1032 blocks in one call — the
    persistent kernel takes all K iterations in one launch — where each image alone is 12 or 24 blocks.  One child (imports, 57 small
    uniform calls, one ragged call, four oracle images), one time limit."""
    import _encode_ragged_worker as W
    its, blocks = W.items()
    assert len(its) >= 48 and blocks >= W.MIN_BLOCKS and {((H, Wd), t) for H, Wd, t in its} == {(s, t) for s in W.SIZES for t in W.TRIPLES}
    env = dict(os.environ, LRF_PERSIST="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_encode_ragged_worker.py")], env=env, capture_output=True, text=True, timeout=90)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "DONE" in r.stdout, r.stdout[-2000:]
    d = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert d["images"] == len(its) and d["blocks"] == blocks >= 1024
    assert d["persist"] == 1, f"LRF_K_BCD_PERSIST launches: {d['persist']} (LRF_K_BCD regions: {d['bcd']})"
    assert d["nbad"] == 0, "\n".join(d["bad"])
    assert len(d["oracle"]) == 4 and d["ctx"] == "", d
