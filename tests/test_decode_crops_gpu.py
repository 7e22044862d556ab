"""GPU suite (-m gpu): windows of compressed images straight from their factors (Context.decode_crops, lrf_amd.qmf_decode_crops,
lrf_amd.qmf_load_factors) against the uniform decoder's whole image sliced, the CPU oracle and the reference's own pixels.
Factors are random int8 in [-16, 15], as in test_decode_ragged_gpu.py: no encode is needed, and the out-of-range pixels they
give exercise the clamp.  Everything is compared bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Case

pytestmark = pytest.mark.gpu

# 24x48: the strip body; 32x272: 16-aligned, two tiles per strip, the second partial; 40x272: chroma rows padded; 45x61 and
# 173x264: odd sides, h_c / H != 0.5 (the general kernels)
GEOMETRIES = [(24, 48), (32, 272), (40, 272), (45, 61), (173, 264)]
# the tiled classes 0 and 4, the rank <= 8 body on the odd sizes, and the general body
ORIGIN_TRIPLES = [(7, 3, 3), (26, 13, 13), (33, 4, 4), (64, 64, 64)]
# the 30-image list of test_decode_ragged_gpu.py
SIZES = [(32, 272), (40, 272), (45, 61), (64, 96), (24, 48), (173, 264)]
TRIPLES = [(1, 1, 1), (7, 3, 3), (8, 8, 5), (12, 6, 6), (16, 9, 16), (26, 13, 13), (32, 16, 16), (33, 4, 4), (5, 17, 2), (64, 64, 64)]
GOLDEN_MIX = ["tiny_q7", "tiny_r7", "tiny_q20", "odd_q7", "odd_r7", "nat_q7", "s2odd_q7"]


def _random_factors(rng, H, W, ranks):
    from lrf_amd import _lib
    dims = _lib.plane_dims(H, W)
    return (rng.integers(-16, 16, sum(d[4] * r for d, r in zip(dims, ranks)), dtype=np.int8), rng.integers(-16, 16, 64 * sum(ranks), dtype=np.int8))


def _decode_alone(ctx, u, v, H, W, ranks):
    return ctx.decode_rgb(torch.from_numpy(u).cuda()[None], torch.from_numpy(v).cuda()[None], H, W, list(ranks))[0]


def _table(items, us, vs):
    images, uo, vo = [], 0, 0
    for (H, W, ranks), u, v in zip(items, us, vs):
        images.append((H, W, ranks, uo, vo))
        uo += u.size
        vo += v.size
    return torch.from_numpy(np.concatenate(us)).cuda(), torch.from_numpy(np.concatenate(vs)).cuda(), images


class Mixed:
    """the 30 images' factors in two flat device buffers, and each image decoded alone by the uniform decoder: made once"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from lrf_amd import _lib
            ctx = _lib.context(0)
            rng = np.random.default_rng(2024)
            items = [(H, W, TRIPLES[(2 * i + j) % len(TRIPLES)]) for j in range(5) for i, (H, W) in enumerate(SIZES)]
            fac = [_random_factors(rng, *it) for it in items]
            us, vs = [f[0] for f in fac], [f[1] for f in fac]
            alone = [_decode_alone(ctx, u, v, *it).cpu() for it, u, v in zip(items, us, vs)]
            U, V, images = _table(items, us, vs)
            cls._made = (ctx, items, us, vs, U, V, images, alone)
        return cls._made


def _boxes(items, size, seed):
    """per image its four corner windows plus four seeded random ones"""
    h, w = size
    rng = np.random.default_rng(seed)
    out = []
    for i, (H, W, _) in enumerate(items):
        out += [(i, 0, 0), (i, 0, W - w), (i, H - h, 0), (i, H - h, W - w)]
        out += [(i, int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))) for _ in range(4)]
    return out


def _expected(alone, boxes, size):
    h, w = size
    return torch.stack([alone[i][:, y:y + h, x:x + w] for i, y, x in boxes])


@pytest.mark.parametrize("ranks", ORIGIN_TRIPLES, ids=lambda r: "r%d_%d_%d" % r)
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_every_origin(H, W, ranks):
    """all windows of (9,13) of one image in one call == the uniform decoder's image unfolded"""
    from lrf_amd import _lib
    ctx = _lib.context(0)
    u, v = _random_factors(np.random.default_rng(H * 1000 + W + ranks[0]), H, W, ranks)
    whole = _decode_alone(ctx, u, v, H, W, ranks)
    h, w = 9, 13
    ys, xs = np.meshgrid(np.arange(H - h + 1), np.arange(W - w + 1), indexing="ij")
    boxes = np.stack([np.zeros(ys.size, dtype=np.int64), ys.ravel(), xs.ravel()], axis=1)
    got = ctx.decode_crops(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), [(H, W, ranks, 0, 0)], boxes, (h, w))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (boxes.shape[0], 3, h, w)
    want = whole.unfold(1, h, 1).unfold(2, w, 1).permute(1, 2, 0, 3, 4).reshape(-1, 3, h, w)
    assert torch.equal(got, want)
    assert int(whole.min()) == 0 and int(whole.max()) == 255  # the clamp was at work


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (16, 16), (24, 48)], ids=lambda s: "%dx%d" % s)
def test_mixed_list(oracle, size):
    from lrf_amd.codec import split_factors
    ctx, items, us, vs, U, V, images, alone = Mixed.get()
    boxes = _boxes(items, size, seed=size[0] * 100 + size[1])
    got = ctx.decode_crops(U, V, images, boxes, size).cpu()
    assert torch.equal(got, _expected(alone, boxes, size))
    h, w = size
    for i, (H, W, ranks) in enumerate(items):  # and the CPU oracle, every image: every launch group and class
        f = split_factors(us[i], vs[i], (H, W), ranks)
        ref = oracle.planes_to_rgb(f[0::2], f[1::2], H, W)
        for j in range(8 * i, 8 * i + 8):
            _, y, x = boxes[j]
            assert np.array_equal(got[j].numpy(), ref[:, y:y + h, x:x + w]), (items[i], boxes[j])


def test_whole_image():
    ctx, items, us, vs, U, V, images, alone = Mixed.get()
    seen = set()
    for i, (H, W, ranks) in enumerate(items):
        if (H, W) in seen:
            continue
        seen.add((H, W))
        assert torch.equal(ctx.decode_crops(U, V, images, [(i, 0, 0)], (H, W))[0].cpu(), alone[i]), items[i]
    for (H, W), ranks in zip(GEOMETRIES, ORIGIN_TRIPLES + [(12, 6, 6)]):
        u, v = _random_factors(np.random.default_rng(H + W), H, W, ranks)
        got = ctx.decode_crops(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), [(H, W, ranks, 0, 0)], [(0, 0, 0)], (H, W))
        assert torch.equal(got[0], _decode_alone(ctx, u, v, H, W, ranks)), (H, W, ranks)


def test_independence_of_order_and_repetition():
    ctx, items, us, vs, U, V, images, alone = Mixed.get()
    size = (7, 5)
    boxes = _boxes(items, size, seed=1)
    got = ctx.decode_crops(U, V, images, boxes, size)
    perm = np.random.default_rng(2).permutation(len(boxes))
    assert torch.equal(ctx.decode_crops(U, V, images, [boxes[j] for j in perm], size), got[torch.from_numpy(perm).cuda()])
    twice = ctx.decode_crops(U, V, images, [boxes[5], boxes[100], boxes[5]], size)
    assert torch.equal(twice[0], got[5]) and torch.equal(twice[2], got[5]) and torch.equal(twice[1], got[100])
    assert torch.equal(ctx.decode_crops(U, V, images, [boxes[77]], size)[0], got[77])  # alone in its call


def test_back_to_back_calls_with_different_lists():
    """eight calls, eight box lists, no synchronisation in between: more calls than staging slots, so a slot whose copy had not
    run when it was written again would show as another call's boxes; the same after trim"""
    ctx, items, us, vs, U, V, images, alone = Mixed.get()
    size = (16, 16)
    for round_ in range(2):
        lists = [_boxes(items, size, seed=50 + 10 * round_ + k) for k in range(8)]
        torch.cuda.synchronize()
        outs = [ctx.decode_crops(U, V, images, b, size) for b in lists]
        for b, o in zip(lists, outs):
            assert torch.equal(o.cpu(), _expected(alone, b, size))
        ctx.trim()


def test_golden_streams():
    import lrf_amd
    cases = [Case(n) for n in GOLDEN_MIX]
    streams = [c.encoded for c in cases]
    whole = [lrf_amd.qmf_decode(s) for s in streams]  # pinned to the reference's pixels by test_oracle_golden's sha256
    size = (min(32, min(d.shape[1] for d in whole)), min(32, min(d.shape[2] for d in whole)))
    boxes = _boxes([(d.shape[1], d.shape[2], None) for d in whole], size, seed=7)
    want = _expected([d.cpu() for d in whole], boxes, size)
    got = lrf_amd.qmf_decode_crops(streams, boxes, size)
    assert got.is_cuda and torch.equal(got.cpu(), want)
    res = lrf_amd.qmf_load_factors(streams)
    assert len(res) == len(streams) and res.sizes == [(d.shape[1], d.shape[2]) for d in whole]
    assert torch.equal(res.decode_crops(np.array(boxes), size).cpu(), want)
    assert torch.equal(lrf_amd.qmf_decode_crops(res, boxes, size).cpu(), want)
    for a, b in zip(res.decode(), lrf_amd.qmf_decode_ragged(streams)):
        assert torch.equal(a, b)


def test_c_entry_refuses_on_the_host_and_launches_nothing():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    lib = _lib.load()
    H, W, ranks, h, w = 64, 96, (7, 3, 3), 9, 13
    dims = _lib.plane_dims(H, W)
    nu, nv, npx = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks), 3 * h * w
    U = torch.zeros((2 * nu,), dtype=torch.int8, device="cuda")
    V = torch.zeros((2 * nv,), dtype=torch.int8, device="cuda")
    rgb = torch.full((3 * npx,), 0xA5, dtype=torch.uint8, device="cuda")
    ok_images = [(H, W, ranks, 0, 0), (H, W, ranks, nu, nv)]
    ok_crops = [(0, 0, 0), (1, H - h, W - w), (1, 3, 4)]

    def call(images=ok_images, crops=ok_crops, n_images=None, n_crops=None, size=(h, w), u_len=2 * nu, v_len=2 * nv, rgb_len=3 * npx, u=U, v=V, out=rgb,
             null_images=False, null_crops=False):
        desc = (_lib.RaggedImage * max(1, len(images)))()
        for d, (ih, iw, r, uo, vo) in zip(desc, images):
            d.H, d.W, d.u_off, d.v_off, d.rgb_off = ih, iw, uo, vo, 0
            d.R[0], d.R[1], d.R[2] = r
        cr = (_lib.Crop * max(1, len(crops)))()
        for c, (i, y, x) in zip(cr, crops):
            c.image, c.y0, c.x0 = i, y, x
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ctx.use_torch_stream()
        return lib.lrf_qmf_decode_crops_rgb_u8(ctx._h, len(images) if n_images is None else n_images, None if null_images else desc, ptr(u), u_len,
                                               ptr(v), v_len, len(crops) if n_crops is None else n_crops, None if null_crops else cr, size[0], size[1],
                                               ptr(out), rgb_len)

    refused = {
        "NULL U": call(u=None), "NULL V": call(v=None), "NULL rgb": call(out=None), "NULL images": call(null_images=True), "NULL crops": call(null_crops=True),
        "n_images = 0": call(n_images=0), "n_images = 65536": call(n_images=65536),
        "n_crops = 0": call(n_crops=0), "n_crops = 2^20 + 1": call(n_crops=2 ** 20 + 1),
        "h = 0": call(size=(0, w)), "w = 0": call(size=(h, 0)), "h < 0": call(size=(-h, w)),
        "image index 2": call(crops=ok_crops[:2] + [(2, 0, 0)]), "image index -1": call(crops=ok_crops[:2] + [(-1, 0, 0)]),
        "y0 < 0": call(crops=ok_crops[:2] + [(0, -1, 0)]), "x0 < 0": call(crops=ok_crops[:2] + [(0, 0, -1)]),
        "past the bottom": call(crops=ok_crops[:2] + [(0, H - h + 1, 0)]), "past the right": call(crops=ok_crops[:2] + [(0, 0, W - w + 1)]),
        "taller than the image": call(crops=[(0, 0, 0)], size=(H + 1, w), rgb_len=2 ** 40), "near 2^31": call(crops=[(0, 2 ** 31 - 1, 0)]),
        "rank 0": call(images=[ok_images[0], (H, W, (7, 0, 3), nu, nv)]), "rank 65": call(images=[ok_images[0], (H, W, (65, 3, 3), nu, nv)]),
        "no size": call(images=[ok_images[0], (0, W, ranks, nu, nv)]), "1x1": call(images=[ok_images[0], (1, 1, ranks, nu, nv)]),
        "u range": call(u_len=2 * nu - 1), "v range": call(v_len=2 * nv - 1), "rgb range": call(rgb_len=3 * npx - 1),
        "u offset past the end": call(images=[ok_images[0], (H, W, ranks, nu + 1, nv)]), "negative v": call(images=[ok_images[0], (H, W, ranks, nu, -1)]),
        "offset near 2^63": call(images=[ok_images[0], (H, W, ranks, 2 ** 63 - 1, nv)]),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    torch.cuda.synchronize()
    assert bool((rgb == 0xA5).all()), "a refused call wrote to its output"
    assert call() == 0  # and the same call with the arguments right runs
    torch.cuda.synchronize()
    assert not bool((rgb == 0xA5).any())  # zero factors: every byte of the three crops was written
    with pytest.raises(ValueError):
        ctx.decode_crops(U, V, ok_images, [(0, H - h + 1, 0)], (h, w))
    with pytest.raises(TypeError):
        ctx.decode_crops(U, V, ok_images, [(0.0, 0.0, 0.0)], (h, w))


@pytest.mark.parametrize("n,ranks", [(256, (7, 3, 3)), (64, (26, 13, 13))], ids=["256_r7", "64_r26"])
def test_at_the_loaders_shape(n, ranks):
    from lrf_amd import _lib
    ctx = _lib.context(0)
    H, W, h, w = 512, 768, 224, 224
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    g = torch.Generator().manual_seed(n)
    U = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g).cuda()
    V = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g).cuda()
    rng = np.random.default_rng(n)
    boxes = np.stack([np.arange(n), rng.integers(0, H - h + 1, n), rng.integers(0, W - w + 1, n)], axis=1)
    got = ctx.decode_crops(U.reshape(-1), V.reshape(-1), [(H, W, ranks, b * nu, b * nv) for b in range(n)], boxes, (h, w))
    whole = ctx.decode_rgb(U, V, H, W, list(ranks))
    want = torch.stack([whole[b, :, y:y + h, x:x + w] for b, y, x in boxes])
    assert torch.equal(got, want)


def test_the_entries_that_share_the_resident_descriptor_table_take_turns():
    """decode_crops, decode_scaled_crops, decode_resized_crops and decode_scaled keep their image descriptors in one device table
    that stays resident under its bytes, decode_ragged in one of its own: two lists that differ in ranks alone, the entries in
    turn on one context with nothing waited for in between (a new list's upload must not overtake the kernels still reading the
    old one), a trim in the middle — every result byte-equal to the same call made alone on a fresh context"""
    from lrf_amd import _lib
    rng = np.random.default_rng(77)
    lists = {}
    for name, ranks in (("A", (7, 3, 3)), ("B", (26, 13, 13))):
        items = [(24, 48, ranks), (45, 61, ranks)]
        fac = [_random_factors(rng, *it) for it in items]
        lists[name] = _table(items, [f[0] for f in fac], [f[1] for f in fac])
    windows = [(0, 0, 0), (1, 36, 48), (0, 15, 35), (1, 7, 3)]
    scaled = [(0, 2, 0, 0), (1, 2, 18, 26), (1, 4, 8, 12), (0, 4, 1, 7), (1, 8, 2, 4)]
    boxes = [(0, 0, 0, 24, 48, 0), (1, 3, 5, 40, 50, 1), (1, 20, 20, 9, 9, 0), (0, 4, 8, 16, 32, 1)]
    calls = [
        lambda c: c.decode_crops(*lists["A"], windows, (9, 13)),
        lambda c: c.decode_scaled_crops(*lists["A"], scaled, (4, 4)),
        lambda c: c.decode_resized_crops(*lists["B"], boxes, (8, 8)),
        lambda c: c.decode_crops(*lists["B"], windows, (9, 13)),
        lambda c: c.decode_crops(*lists["A"], windows, (9, 13)),
        lambda c: (c.trim(), None)[1],
        lambda c: c.decode_scaled(*lists["A"], 2),
        lambda c: c.decode_ragged(*lists["B"]),
    ]
    flat = lambda r: [] if r is None else [t.cpu() for t in (r if isinstance(r, list) else [r])]
    ctx = _lib.Context(0)
    try:
        got = [call(ctx) for call in calls]  # (no synchronisation between the calls: the results are read after the last)
        got = [flat(r) for r in got]
    finally:
        ctx.close()
    for k, call in enumerate(calls):
        fresh = _lib.Context(0)
        try:
            want = flat(call(fresh))
        finally:
            fresh.close()
        assert len(got[k]) == len(want) and all(torch.equal(a, b) for a, b in zip(got[k], want)), f"call {k}"
    assert sum(len(g) for g in got) == 5 + 2 + 2  # five [n, 3, h, w] tensors, two scaled images, two whole images
