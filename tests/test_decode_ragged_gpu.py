"""GPU suite (-m gpu): the ragged decode — images that differ in size and ranks in one call (Context.decode_ragged,
lrf_amd.qmf_decode_ragged) — against the uniform decoder called for each image alone, the CPU oracle, and the reference's own
pixels.  Factors are random int8 in [-16, 15]: no encode is needed, and the out-of-range pixels they give exercise the clamp.
Everything is compared bitwise."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, Case, make_image

pytestmark = pytest.mark.gpu

# 32x272: 16-aligned, 34 luma patches per row = two tiles per strip, the second partial; 64x96: 16-aligned; 40x272, 24x48: the
# strip body; 45x61, 173x264: the general kernels
SIZES = [(32, 272), (40, 272), (45, 61), (64, 96), (24, 48), (173, 264)]
# classes 0, 0, 1, 2, 3, 4, 4 of the tiled bodies, then three triples only the general kernel serves
TRIPLES = [(1, 1, 1), (7, 3, 3), (8, 8, 5), (12, 6, 6), (16, 9, 16), (26, 13, 13), (32, 16, 16), (33, 4, 4), (5, 17, 2), (64, 64, 64)]
GOLDEN_MIX = ["tiny_q7", "tiny_r7", "tiny_q20", "odd_q7", "odd_r7", "nat_q7", "s2odd_q7"]
TILE16, STRIP, R8, ANY = "tile16", "strip", "r8", "any"


def group_of(H, W, ranks):
    """the launch group of an image whose output is 8-byte aligned: the rule of decode_plan's comment (lrf_amd/csrc/lrf_plan.cpp;
    tests/test_decode_ragged_plan.py compares the whole rule with the library on the CPU) for the sizes above (among
    them only the odd-width 45x61 and 173x264, whose chroma padding is not four-aligned, fall outside the tiled bodies)"""
    if (H, W) in ((45, 61), (173, 264)) or ranks[0] > 32 or max(ranks[1:]) > 16:
        return R8 if max(ranks) <= 8 else ANY
    return TILE16 if H % 16 == 0 and W % 16 == 0 else STRIP


def _mixed_list():
    """30 (H, W, ranks): every size with five triples, the triples dealt so that each meets several sizes, in an order in which
    neighbours are of different launch groups"""
    items = [(H, W, TRIPLES[(2 * i + j) % len(TRIPLES)]) for j in range(5) for i, (H, W) in enumerate(SIZES)]
    assert len(items) == 30 and {t for _, _, t in items} == set(TRIPLES)
    groups = [group_of(*it) for it in items]
    assert set(groups) == {TILE16, STRIP, R8, ANY}
    assert sum(a != b for a, b in zip(groups, groups[1:])) >= 20
    return items


class Mixed:
    """the 30 images' factors in two flat buffers, and each image decoded alone by the uniform decoder: made once"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from lrf_amd import _lib
            ctx = _lib.context(0)
            rng = np.random.default_rng(2024)
            items = _mixed_list()
            us, vs = [], []
            for H, W, ranks in items:
                dims = _lib.plane_dims(H, W)
                us.append(rng.integers(-16, 16, sum(d[4] * r for d, r in zip(dims, ranks)), dtype=np.int8))
                vs.append(rng.integers(-16, 16, 64 * sum(ranks), dtype=np.int8))
            alone = [ctx.decode_rgb(torch.from_numpy(u).cuda()[None], torch.from_numpy(v).cuda()[None], H, W, list(r))[0].cpu()
                     for (H, W, r), u, v in zip(items, us, vs)]
            cls._made = (ctx, items, us, vs, alone)
        return cls._made


def _ragged(ctx, items, us, vs, order):
    """decode_ragged of the images in `order` -> results in that order"""
    U = torch.from_numpy(np.concatenate([us[i] for i in order])).cuda()
    V = torch.from_numpy(np.concatenate([vs[i] for i in order])).cuda()
    images, uo, vo = [], 0, 0
    for i in order:
        images.append((items[i][0], items[i][1], items[i][2], uo, vo))
        uo += us[i].size
        vo += vs[i].size
    out = ctx.decode_ragged(U, V, images)
    assert len(out) == len(order)
    for o, i in zip(out, order):
        assert o.dtype == torch.uint8 and tuple(o.shape) == (3, items[i][0], items[i][1]) and o.data_ptr() % 16 == 0
    return [o.cpu() for o in out]


def test_mixed_list_equals_the_uniform_decoder_image_by_image(oracle):
    from lrf_amd.codec import split_factors
    ctx, items, us, vs, alone = Mixed.get()
    got = _ragged(ctx, items, us, vs, range(len(items)))
    for i, (g, a) in enumerate(zip(got, alone)):
        assert torch.equal(g, a), (i, items[i])
    assert any(int(a.min()) == 0 for a in alone) and any(int(a.max()) == 255 for a in alone)  # the clamp was at work
    for i, (H, W, ranks) in enumerate(items):  # and the CPU oracle: every image, so every launch group and class
        f = split_factors(us[i], vs[i], (H, W), ranks)
        assert np.array_equal(got[i].numpy(), oracle.planes_to_rgb(f[0::2], f[1::2], H, W)), (i, items[i])


def test_uniform_list_equals_one_uniform_batch():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    H, W, ranks = 64, 96, (7, 3, 3)
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    g = torch.Generator().manual_seed(5)
    U = torch.randint(-16, 16, (5, nu), dtype=torch.int8, generator=g).cuda()
    V = torch.randint(-16, 16, (5, nv), dtype=torch.int8, generator=g).cuda()
    batch = ctx.decode_rgb(U, V, H, W, list(ranks))
    out = ctx.decode_ragged(U.reshape(-1), V.reshape(-1), [(H, W, ranks, b * nu, b * nv) for b in range(5)])
    assert torch.equal(torch.stack(out), batch)


def test_one_image():
    ctx, items, us, vs, alone = Mixed.get()
    groups = [group_of(*it) for it in items]
    for i in [groups.index(g) for g in (TILE16, STRIP, R8, ANY)] + [len(items) - 1]:  # the first of every group, and the last image
        assert torch.equal(_ragged(ctx, items, us, vs, [i])[0], alone[i]), items[i]


def test_reversed_order_gives_the_same_bytes_per_image():
    ctx, items, us, vs, alone = Mixed.get()
    order = list(range(len(items)))[::-1]
    for i, g in zip(order, _ragged(ctx, items, us, vs, order)):
        assert torch.equal(g, alone[i]), (i, items[i])


def test_bytes_do_not_depend_on_the_pixel_quads_per_thread():
    """k_decode8_ragged's `reps` follows the launch's total: 100 x 173x264 at (7,3,3) are 4500 groups of 256 pixel quads, two quads
    per thread; one such image alone takes one.  The image's bytes must be the same."""
    from lrf_amd import _lib
    ctx = _lib.context(0)
    H, W, ranks, n = 173, 264, (7, 3, 3), 100
    assert n * -(-(H * ((W + 3) // 4)) // 256) // 2048 == 2
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    g = torch.Generator().manual_seed(9)
    U = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g).cuda()
    V = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g).cuda()
    out = ctx.decode_ragged(U.reshape(-1), V.reshape(-1), [(H, W, ranks, b * nu, b * nv) for b in range(n)])
    for b in (0, 37, 99):
        assert torch.equal(out[b], ctx.decode_ragged(U[b], V[b], [(H, W, ranks, 0, 0)])[0])
    assert torch.equal(torch.stack(out), ctx.decode_rgb(U, V, H, W, list(ranks)))


def test_golden_streams_of_mixed_sizes_and_ranks_give_the_reference_pixels():
    import lrf_amd
    cases = [Case(n) for n in GOLDEN_MIX]
    out = lrf_amd.qmf_decode_ragged([c.encoded for c in cases])
    assert len(out) == len(cases)
    for c, o in zip(cases, out):
        assert o.is_cuda and tuple(o.shape) == tuple(c.image.shape)
        assert hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() == c.decoded_sha256, c.name


def test_round_trip_of_a_target_encode_with_differing_triples():
    import lrf_amd
    H, W = 192, 256  # the nine-image batch of tests/test_encode_target_gpu.py
    nat = torch.from_numpy(np.load(os.path.join(GOLDEN, "nat_q7.npz"))["image"])
    imgs = [make_image(dict(kind="smooth", seed=300 + i, H=H, W=W)) for i in range(3)]
    imgs += [nat[:, y:y + H, x:x + W] for y, x in ((0, 0), (200, 300), (400, 600), (450, 100))]
    g = torch.Generator().manual_seed(11)
    imgs += [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for _ in range(2)]
    images = torch.stack(imgs).contiguous()
    table = lrf_amd.qmf_encode_target(images, 0.0)["table"]
    target = [table[2 + 3 * b, b].item() for b in range(images.shape[0])]  # image b's own PSNR at quality 3 + 3 b
    out = lrf_amd.qmf_encode_target(images, target)
    triples = {tuple(lrf_amd.qmf_ranks((H, W), quality=q)) for q in out["quality"]}
    assert len(triples) >= 3, out["quality"]
    dec = lrf_amd.qmf_decode_ragged(out["streams"])
    for i, s in enumerate(out["streams"]):
        assert torch.equal(dec[i].cpu(), lrf_amd.qmf_decode(s)), i
    assert torch.equal(lrf_amd.psnr_batch(images, torch.stack(dec)).cpu(), out["psnr"])  # bitwise


def test_c_entry_refuses_on_the_host_and_launches_nothing():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    lib = _lib.load()
    H, W, ranks = 64, 96, (7, 3, 3)
    dims = _lib.plane_dims(H, W)
    nu, nv, npx = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks), 3 * H * W
    U = torch.zeros((2 * nu,), dtype=torch.int8, device="cuda")
    V = torch.zeros((2 * nv,), dtype=torch.int8, device="cuda")
    rgb = torch.full((2 * npx,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(n, images, u_len=2 * nu, v_len=2 * nv, rgb_len=2 * npx, u=U, v=V, out=rgb):
        desc = (_lib.RaggedImage * max(1, len(images)))()
        for d, (h, w, r, uo, vo, ro) in zip(desc, images):
            d.H, d.W, d.u_off, d.v_off, d.rgb_off = h, w, uo, vo, ro
            d.R[0], d.R[1], d.R[2] = r
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ctx.use_torch_stream()
        return lib.lrf_qmf_decode_ragged_rgb_u8(ctx._h, n, desc, ptr(u), u_len, ptr(v), v_len, ptr(out), rgb_len)

    ok = [(H, W, ranks, 0, 0, 0), (H, W, ranks, nu, nv, npx)]
    refused = {
        "u range": call(2, ok, u_len=2 * nu - 1),
        "v range": call(2, ok, v_len=2 * nv - 1),
        "rgb range": call(2, ok, rgb_len=2 * npx - 1),
        "u offset past the end": call(2, [ok[0], (H, W, ranks, nu + 1, nv, npx)]),
        "v offset past the end": call(2, [ok[0], (H, W, ranks, nu, nv + 1, npx)]),
        "rgb offset past the end": call(2, [ok[0], (H, W, ranks, nu, nv, npx + 1)]),
        "negative u": call(2, [ok[0], (H, W, ranks, -1, nv, npx)]),
        "negative v": call(2, [ok[0], (H, W, ranks, nu, -1, npx)]),
        "negative rgb": call(2, [ok[0], (H, W, ranks, nu, nv, -16)]),
        "offset near 2^63": call(2, [ok[0], (H, W, ranks, 2 ** 63 - 1, nv, npx)]),
        "rank 0": call(2, [ok[0], (H, W, (7, 0, 3), nu, nv, npx)]),
        "rank 65": call(2, [ok[0], (H, W, (65, 3, 3), nu, nv, npx)]),
        "n = 0": call(0, ok),
        "n = 65536": call(65536, ok),
        "no size": call(2, [ok[0], (0, W, ranks, nu, nv, npx)]),
        "1x1": call(2, [ok[0], (1, 1, ranks, nu, nv, npx)]),  # the chroma plane would be empty: the uniform decoder refuses it too
        "NULL U": call(2, ok, u=None),
        "NULL rgb": call(2, ok, out=None),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    torch.cuda.synchronize()
    assert bool((rgb == 0xA5).all()), "a refused call wrote to its output"
    assert call(2, ok) == 0  # and the same call with the arguments right runs
    torch.cuda.synchronize()
    assert not bool((rgb == 0xA5).all())
    with pytest.raises(ValueError):
        ctx.decode_ragged(U, V, [(H, W, ranks, nu + 1, nv)])
    with pytest.raises(ValueError):
        ctx.decode_ragged(U, V, [(H, W, (7, 3, 65), 0, 0)])
    with pytest.raises(ValueError):
        ctx.decode_ragged(U, V, [])
    with pytest.raises(TypeError):
        ctx.decode_ragged(U.float(), V, [(H, W, ranks, 0, 0)])


def test_table_survives_trim_and_a_changed_list():
    """the device table is cached on the descriptor bytes: a repeated call, a different list and a call after trim all decode right"""
    ctx, items, us, vs, alone = Mixed.get()
    for order in ([0, 1, 2], [0, 1, 2], [2, 1, 0], [5]):
        for i, g in zip(order, _ragged(ctx, items, us, vs, order)):
            assert torch.equal(g, alone[i])
    ctx.trim()
    for i, g in zip([0, 1, 2], _ragged(ctx, items, us, vs, [0, 1, 2])):
        assert torch.equal(g, alone[i])
