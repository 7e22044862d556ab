"""GPU suite (-m gpu): boxes of any size resampled to one output size straight from the factors (Context.decode_resized_crops,
ResidentFactors.decode_resized_crops, lrf_amd.qmf_decode_resized_crops) against the definition in numpy (tests/resized_decode.py:
reference_resized) over the level images of the CPU oracle (f = 1) and of scaled_decode.reference_scaled (f = 2, 4, 8).  Factors
are random int8 in [-16, 15] as in test_decode_scaled_gpu.py.  Every comparison with the reference is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Case
from resized_decode import reference_resized, resized_level
from scaled_decode import random_factors, reference_scaled

pytestmark = pytest.mark.gpu

# 64x96, 32x272: sides multiples of 16; 45x61, 173x264: odd sides, padded planes, partial blocks at the levels; 9x9: the smallest
GEOMETRIES = [(64, 96), (32, 272), (45, 61), (173, 264), (9, 9)]
# ranks <= 8 (the decode8 fill, twice), past 8 (the general fill), the largest
TRIPLES = [(1, 1, 1), (7, 3, 3), (26, 13, 13), (64, 64, 64)]
SIZES_OUT = [(5, 7), (16, 16), (17, 33)]  # (17, 33): two tiles of rows
GOLDEN = ["tiny_q7", "tiny_q20", "odd_q7", "nat_q7", "s2odd_q7", "s1_q7"]
# the staged path's tiles (lrf_plan.h: LRF_RS_TH, LRF_RS_TW, LRF_RS_FH, LRF_RS_FW and resized_staged), to say which path a box takes
TH, TW, FH, FW = 16, 64, 44, 192


def staged(hb, wb, oh, ow):
    f = resized_level(hb, wb, oh, ow)
    bound = lambda tile, n_out, nb: (min(tile, n_out) - 1) * nb // (n_out * f) + 3
    return bound(TH, oh, hb) <= FH and bound(TW, ow, wb) <= FW


class Levels:
    """the level images of one image's factors, each made when first asked for"""

    def __init__(self, oracle, u, v, H, W, ranks):
        from lrf_amd.codec import split_factors
        self.oracle, self.f6, self.H, self.W, self.made = oracle, split_factors(u, v, (H, W), ranks), H, W, {}

    def __getitem__(self, f):
        if f not in self.made:
            self.made[f] = (self.oracle.planes_to_rgb(self.f6[0::2], self.f6[1::2], self.H, self.W) if f == 1
                            else reference_scaled(self.f6, self.H, self.W, f, self.oracle))
        return self.made[f]

    def resized(self, box, size, flip):
        return reference_resized(self[resized_level(box[2], box[3], *size)], box, size, flip)


_CASES = {}


def _case(oracle, H, W, ranks):
    """(u, v, Levels) of one image, made once and shared by the output sizes: the first seed of the case's sequence at which at
    least 5 % of the bytes of every level lie strictly between 0 and 255, so that no comparison is one of saturated bytes"""
    key = (H, W, ranks)
    if key not in _CASES:
        for k in range(64):
            rng = np.random.default_rng(H * 1000 + W + ranks[0] + 7919 * k)
            u, v = random_factors(rng, H, W, ranks)
            lv = Levels(oracle, u, v, H, W, ranks)
            if all(float(((lv[f] > 0) & (lv[f] < 255)).mean()) >= 0.05 for f in (1, 2, 4, 8)):
                break
        else:
            raise AssertionError(f"no seed gives {H}x{W} at {ranks} unsaturated bytes")
        _CASES[key] = (u, v, lv)
    return _CASES[key]


def _boxes_of(H, W, size, seed):
    """(y0, x0, hb, wb) of one image for one output size: see the module's tests for why each is there"""
    oh, ow = size
    out = [(0, 0, H, W), (H // 2, W // 3, 1, 1), (H - 3, W - 3, 3, 3), (1, 2, 3, 3)]
    if oh <= H and ow <= W:
        out += [(H - oh, W - ow, oh, ow), ((H - oh) // 2, (W - ow) // 3, oh, ow)]  # the plain crop, at the corner and inside
    for f in (2, 4, 8):
        if f * oh <= H and f * ow <= W:
            y, x = (H - f * oh) // f * f, (W - f * ow) // f * f
            out += [(y, x, f * oh, f * ow), (0, 0, f * oh, f * ow)]  # the crop of level f, at the last aligned origin and the first
            out += [(H - f * oh, W - f * ow, f * oh, f * ow)]  # the same box at the corner, aligned or not
            out += [(1, 0, f * oh - 1, f * ow)]  # one row short of level f: level f / 2
            if f * oh + 1 <= H and f * ow + 1 <= W:
                out += [(0, 0, f * oh + 1, f * ow + 1)]
    hb, wb = min(H, 2 * oh + 1), min(W, 3 * ow + 2)
    out += [(H - hb, W - wb, hb, wb)]  # the bottom-right corner: the taps' clamp
    out += [(H - 8, 0, 8, W), (0, W - 8, H, 8)]  # 8 x W and H x 8: extreme aspect ratios (the direct path where W is large)
    rng = np.random.default_rng(seed)
    for _ in range(4):
        hb, wb = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        out.append((int(rng.integers(0, H - hb + 1)), int(rng.integers(0, W - wb + 1)), hb, wb))
    return out


@pytest.mark.parametrize("size", SIZES_OUT, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ranks", TRIPLES, ids=lambda r: "r%d_%d_%d" % r)
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_boxes_of_one_image(oracle, H, W, ranks, size):
    from lrf_amd import _lib
    ctx = _lib.context(0)
    u, v, lv = _case(oracle, H, W, ranks)
    boxes = _boxes_of(H, W, size, seed=H + W + size[0])
    rows = [(0,) + b + (flip,) for b in boxes for flip in (0, 1)]
    got = ctx.decode_resized_crops(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), [(H, W, ranks, 0, 0)], rows, size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(rows), 3) + size
    got = got.cpu().numpy()
    for j, r in enumerate(rows):
        assert np.array_equal(got[j], lv.resized(r[1:5], size, r[5])), (H, W, ranks, size, r, resized_level(r[3], r[4], *size), staged(r[3], r[4], *size))
    if (H, W) == (173, 264):  # both paths and every level were met
        assert {resized_level(b[2], b[3], *size) for b in boxes} == {1, 2, 4, 8} and {staged(b[2], b[3], *size) for b in boxes} == {True, False}


@pytest.mark.parametrize("ranks", [(7, 3, 3), (26, 13, 13)], ids=lambda r: "r%d_%d_%d" % r)
@pytest.mark.parametrize("H,W", [(64, 96), (45, 61)])
def test_the_two_identities_against_the_crop_kernels(H, W, ranks):
    """a box of the output's size == decode_crops; a box of f x the output at a multiple of f == decode_scaled_crops: every origin"""
    from lrf_amd import _lib
    ctx = _lib.context(0)
    u, v = random_factors(np.random.default_rng(H + W + ranks[0]), H, W, ranks)
    U, V, images = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), [(H, W, ranks, 0, 0)]
    oh, ow = 5, 7
    for f in (1, 2, 4, 8):
        if f * oh > H or f * ow > W:
            continue
        ys, xs = np.meshgrid(np.arange(0, H - f * oh + 1, f), np.arange(0, W - f * ow + 1, f), indexing="ij")
        n = ys.size
        z = np.zeros(n, dtype=np.int64)
        rows = np.stack([z, ys.ravel(), xs.ravel(), z + f * oh, z + f * ow, z], axis=1)
        got = ctx.decode_resized_crops(U, V, images, rows, (oh, ow))
        if f == 1:
            want = ctx.decode_crops(U, V, images, rows[:, :3], (oh, ow))
        else:
            want = ctx.decode_scaled_crops(U, V, images, np.stack([z, z + f, ys.ravel() // f, xs.ravel() // f], axis=1), (oh, ow))
        assert torch.equal(got, want), f
        rows[:, 5] = 1
        assert torch.equal(ctx.decode_resized_crops(U, V, images, rows, (oh, ow)), want.flip(3)), f


class Mixed:
    """the 30-image list of test_decode_scaled_gpu.py with boxes on every level and path, and every box decoded alone: made once"""
    _made = None
    SIZE = (16, 16)

    @classmethod
    def get(cls):
        if cls._made is None:
            from test_decode_scaled_gpu import Mixed as ScaledMixed
            ctx, items, us, vs, U, V, images, _ = ScaledMixed.get()
            rng = np.random.default_rng(77)
            rows = []
            for i, (H, W, _) in enumerate(items):
                for y0, x0, hb, wb in [(0, 0, H, W), (H - 16, W - 16, 16, 16), (0, 0, min(H, 32), 32), (H - 8, 0, 8, W), (H // 2, W // 2, 1, 1)] + _boxes_of(H, W, cls.SIZE, i)[-4:]:
                    rows.append((i, y0, x0, hb, wb, int(rng.integers(0, 2))))
            alone = []
            for i, y0, x0, hb, wb, flip in rows:  # its image alone in the table, the box alone in the call
                H, W, ranks = items[i]
                alone.append(ctx.decode_resized_crops(torch.from_numpy(us[i]).cuda(), torch.from_numpy(vs[i]).cuda(), [(H, W, ranks, 0, 0)],
                                                      [(0, y0, x0, hb, wb, flip)], cls.SIZE)[0])
            cls._made = (ctx, items, us, vs, U, V, images, rows, torch.stack(alone))
        return cls._made


def test_mixed_list_in_one_call(oracle):
    ctx, items, us, vs, U, V, images, rows, alone = Mixed.get()
    groups = {(staged(r[3], r[4], *Mixed.SIZE), resized_level(r[3], r[4], *Mixed.SIZE), max(items[r[0]][2]) <= 8) for r in rows}
    assert {g[:2] for g in groups} >= {(True, 1), (True, 2), (True, 4), (True, 8), (False, 1)} and len(groups) >= 9  # levels, paths and rank classes
    got = ctx.decode_resized_crops(U, V, images, rows, Mixed.SIZE)
    assert torch.equal(got, alone)
    for j in range(0, len(rows), 23):  # a dozen of them against the reference too
        i, y0, x0, hb, wb, flip = rows[j]
        H, W, ranks = items[i]
        assert np.array_equal(got[j].cpu().numpy(), Levels(oracle, us[i], vs[i], H, W, ranks).resized((y0, x0, hb, wb), Mixed.SIZE, flip)), rows[j]


def test_independence_of_order_and_repetition():
    ctx, items, us, vs, U, V, images, rows, alone = Mixed.get()
    perm = np.random.default_rng(2).permutation(len(rows))
    assert torch.equal(ctx.decode_resized_crops(U, V, images, [rows[j] for j in perm], Mixed.SIZE), alone[torch.from_numpy(perm).cuda()])
    twice = ctx.decode_resized_crops(U, V, images, [rows[5], rows[100], rows[5]], Mixed.SIZE)
    assert torch.equal(twice[0], alone[5]) and torch.equal(twice[2], alone[5]) and torch.equal(twice[1], alone[100])


def test_back_to_back_calls_with_different_lists():
    """eight calls, eight lists and sizes, no synchronisation in between: more calls than staging slots; the same after trim"""
    ctx, items, us, vs, U, V, images, rows, alone = Mixed.get()
    for round_ in range(2):
        rng = np.random.default_rng(50 + round_)
        lists = [[rows[j] for j in rng.permutation(len(rows))[:40 + 5 * k]] for k in range(8)]
        sizes = [(5, 7), (16, 16), (17, 33), (8, 70)] * 2
        want = [ctx.decode_resized_crops(U, V, images, b, s).cpu() for b, s in zip(lists, sizes)]  # one at a time, each waited for
        torch.cuda.synchronize()
        outs = [ctx.decode_resized_crops(U, V, images, b, s) for b, s in zip(lists, sizes)]
        for o, w in zip(outs, want):
            assert torch.equal(o.cpu(), w)
        ctx.trim()


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_golden_streams(oracle, inflate):
    import lrf_amd
    cases = [Case(n) for n in GOLDEN]
    streams = [c.encoded for c in cases]
    size = (16, 16)
    boxes, flips, want = [], [], []
    rng = np.random.default_rng(13)
    for i, c in enumerate(cases):
        H, W = c.image.shape[-2:]
        levels = {1: lrf_amd.qmf_decode(c.encoded).cpu().numpy()}  # pinned to the reference's pixels by test_oracle_golden's sha256
        for y0, x0, hb, wb in [(0, 0, H, W), (H - 16, W - 16, 16, 16), (3, 5, 40, 50), (H - 8, 0, 8, W)] + _boxes_of(H, W, size, i)[-2:]:
            f = resized_level(hb, wb, *size)
            if f not in levels:
                levels[f] = reference_scaled(c.ref_factors(), H, W, f, oracle)
            flip = bool(rng.integers(0, 2))
            boxes.append((i, y0, x0, hb, wb))
            flips.append(flip)
            want.append(reference_resized(levels[f], (y0, x0, hb, wb), size, flip))
    want = np.stack(want)
    got = lrf_amd.qmf_decode_resized_crops(streams, boxes, size, flips, inflate=inflate)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    res = lrf_amd.qmf_load_factors(streams, inflate=inflate)
    assert np.array_equal(res.decode_resized_crops(boxes, size, flips).cpu().numpy(), want)
    assert np.array_equal(lrf_amd.qmf_decode_resized_crops(res, boxes, size, flips).cpu().numpy(), want)
    noflip = lrf_amd.qmf_decode_resized_crops(res, boxes, size).cpu()
    assert torch.equal(lrf_amd.qmf_decode_resized_crops(res, boxes, size, True).cpu(), noflip.flip(3))
    assert torch.equal(lrf_amd.qmf_decode_resized_crops(res, boxes, size, False).cpu(), noflip)


def test_c_entry_refuses_on_the_host_and_launches_nothing():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    lib = _lib.load()
    H, W, ranks, oh, ow = 64, 96, (7, 3, 3), 5, 7
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    U = torch.zeros((2 * nu,), dtype=torch.int8, device="cuda")
    V = torch.zeros((2 * nv,), dtype=torch.int8, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def descs(images):
        desc = (_lib.RaggedImage * max(1, len(images)))()
        for d, (ih, iw, r, uo, vo, ro) in zip(desc, images):
            d.H, d.W, d.u_off, d.v_off, d.rgb_off = ih, iw, uo, vo, ro
            d.R[0], d.R[1], d.R[2] = r
        return desc

    npx = 3 * oh * ow
    rgb = torch.full((3 * npx,), 0xA5, dtype=torch.uint8, device="cuda")
    ok_images = [(H, W, ranks, 0, 0, 0), (H, W, ranks, nu, nv, 0)]
    ok_crops = [(0, 0, 0, H, W, 0), (1, H - 8, 0, 8, W, 1), (1, 3, 5, 11, 13, 0)]

    def call(images=ok_images, crops=ok_crops, n_images=None, n_crops=None, size=(oh, ow), u_len=2 * nu, v_len=2 * nv, rgb_len=3 * npx, u=U, v=V, out=rgb,
             null_images=False, null_crops=False):
        cr = (_lib.ResizedCrop * max(1, len(crops)))()
        for c, (i, y, x, h, w, fl) in zip(cr, crops):
            c.image, c.y0, c.x0, c.h, c.w, c.flip = i, y, x, h, w, fl
        ctx.use_torch_stream()
        return lib.lrf_qmf_decode_resized_crops_rgb_u8(ctx._h, len(images) if n_images is None else n_images, None if null_images else descs(images), ptr(u),
                                                       u_len, ptr(v), v_len, len(crops) if n_crops is None else n_crops, None if null_crops else cr, size[0],
                                                       size[1], ptr(out), rgb_len)

    second = lambda **kw: [ok_images[0], tuple(kw.get(k, d) for k, d in zip(("H", "W", "ranks", "u_off", "v_off", "rgb_off"), ok_images[1]))]
    third = lambda c: ok_crops[:2] + [c]
    refused = {
        "NULL U": call(u=None), "NULL V": call(v=None), "NULL rgb": call(out=None), "NULL images": call(null_images=True), "NULL crops": call(null_crops=True),
        "n_images = 0": call(n_images=0), "n_images = 65536": call(n_images=65536),
        "n_crops = 0": call(n_crops=0), "n_crops = 2^20 + 1": call(n_crops=2 ** 20 + 1),
        "oh = 0": call(size=(0, ow)), "ow = 0": call(size=(oh, 0)), "oh < 0": call(size=(-oh, ow)), "oh = 16385": call(size=(16385, ow), rgb_len=2 ** 40),
        "ow = 16385": call(size=(oh, 16385), rgb_len=2 ** 40),
        "image index 2": call(crops=third((2, 0, 0, 5, 5, 0))), "image index -1": call(crops=third((-1, 0, 0, 5, 5, 0))),
        "y0 < 0": call(crops=third((0, -1, 0, 5, 5, 0))), "x0 < 0": call(crops=third((0, 0, -1, 5, 5, 0))),
        "h = 0": call(crops=third((0, 0, 0, 0, 5, 0))), "w = 0": call(crops=third((0, 0, 0, 5, 0, 0))), "h < 0": call(crops=third((0, 9, 9, -3, 5, 0))),
        "past the bottom": call(crops=third((0, 1, 0, H, W, 0))), "past the right": call(crops=third((0, 0, W - 4, 5, 5, 0))),
        "taller than the image": call(crops=third((0, 0, 0, H + 1, W, 0))), "near 2^31": call(crops=third((0, 2 ** 31 - 1, 0, 2, 2, 0))),
        "h near 2^31": call(crops=third((0, 1, 0, 2 ** 31 - 1, 2, 0))),
        "rank 0": call(images=second(ranks=(7, 0, 3))), "rank 65": call(images=second(ranks=(65, 3, 3))),
        "no size": call(images=second(H=0)), "1x1": call(images=second(H=1, W=1)), "size 2^31": call(images=second(H=2 ** 31)),
        "u range": call(u_len=2 * nu - 1), "v range": call(v_len=2 * nv - 1), "rgb range": call(rgb_len=3 * npx - 1), "rgb_len 0": call(rgb_len=0),
        "u offset past the end": call(images=second(u_off=nu + 1)), "negative u": call(images=second(u_off=-1)), "negative v": call(images=second(v_off=-1)),
        "offset near 2^63": call(images=second(u_off=2 ** 63 - 1)),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    torch.cuda.synchronize()
    assert bool((rgb == 0xA5).all()), "a refused call wrote to its output"
    assert call() == 0  # and the same call with the arguments right runs
    torch.cuda.synchronize()
    assert not bool((rgb == 0xA5).any())  # zero factors: every byte of the three crops was written (none is 0xA5)
    images5 = [im[:5] for im in ok_images]
    with pytest.raises(ValueError):
        ctx.decode_resized_crops(U, V, images5, [(0, 1, 0, H, W, 0)], (oh, ow))
    with pytest.raises(TypeError):
        ctx.decode_resized_crops(U, V, images5, [(0.0, 0.0, 0.0, 5.0, 5.0, 0.0)], (oh, ow))
    with pytest.raises(ValueError):
        ctx.decode_resized_crops(U.cpu(), V.cpu(), images5, ok_crops, (oh, ow))


def _random_resized_crop_box(rng, H, W):
    """torchvision's RandomResizedCrop.get_params: area fraction uniform in [0.08, 1], aspect ratio log-uniform in [3/4, 4/3],
    ten tries, then the centre fallback"""
    for _ in range(10):
        area = H * W * rng.uniform(0.08, 1.0)
        ar = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        w, h = int(round(np.sqrt(area * ar))), int(round(np.sqrt(area / ar)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
    r = W / H
    w, h = (W, int(round(W / (4 / 3)))) if r > 4 / 3 else ((int(round(H * 3 / 4)), H) if r < 3 / 4 else (W, H))
    return (H - h) // 2, (W - w) // 2, h, w


def test_at_the_loaders_shape(oracle):
    from lrf_amd import _lib
    ctx = _lib.context(0)
    n, H, W, ranks, size = 64, 512, 768, (7, 3, 3), (224, 224)
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    g = torch.Generator().manual_seed(n)
    Uh = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g)
    Vh = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g)
    U, V = Uh.cuda().reshape(-1), Vh.cuda().reshape(-1)
    images = [(H, W, ranks, b * nu, b * nv) for b in range(n)]
    rng = np.random.default_rng(n)
    rows = [(b,) + _random_resized_crop_box(rng, H, W) + (int(rng.integers(0, 2)),) for b in range(n)]
    levels = [resized_level(r[3], r[4], *size) for r in rows]
    assert set(levels) == {1, 2} and all(staged(r[3], r[4], *size) for r in rows)  # what the loader draws stays on the staged path
    got = ctx.decode_resized_crops(U, V, images, rows, size)
    assert tuple(got.shape) == (n, 3) + size
    check = [levels.index(1), levels.index(2), n - 1]
    for b in check:
        lv = Levels(oracle, Uh[b].numpy(), Vh[b].numpy(), H, W, ranks)
        assert np.array_equal(got[b].cpu().numpy(), lv.resized(rows[b][1:5], size, rows[b][5])), rows[b]
