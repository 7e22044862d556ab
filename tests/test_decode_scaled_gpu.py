"""GPU suite (-m gpu): compressed images at 1/2, 1/4, 1/8 scale straight from their factors (Context.decode_scaled,
Context.decode_scaled_crops, lrf_amd.qmf_decode_scaled, ResidentFactors.decode / .decode_crops with scale=) against the
definition in numpy and the CPU oracle (tests/scaled_decode.py: reference_scaled).  Factors are random int8 in [-16, 15] as in
test_decode_crops_gpu.py: no encode is needed, and the out-of-range pixels they give exercise the clamp.  Every comparison with
the reference is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import Case
from scaled_decode import SCALES, block_average_u8, random_factors, reference_scaled, scaled_dims

pytestmark = pytest.mark.gpu

# sides multiples of 16: the tiled kernel at ranks up to (32, 16, 16) — 32x272: 17 chroma patches per row; 64x96: several rows
TILED = [(16, 16), (32, 272), (64, 96)]
# 24x48, 40x272: padded planes; 45x61, 173x264: odd sides, h_c / H != 0.5, partial blocks; 9x9 and 8x10: the smallest odd and even
# sizes the decoders accept (one patch per chroma plane, at f = 8 blocks of one row) — 2x2 and 9x7 are sizes make_geom refuses,
# as the reference's reflect padding does (a chroma plane of 1 or 3 columns under 7 or 5 of padding): REFUSED below
GENERAL = [(24, 48), (40, 272), (45, 61), (173, 264), (9, 9), (8, 10)]
REFUSED = [(2, 2), (9, 7)]
# the tiled classes 0 and 4, and (ranks past the tiled bounds) the general kernel on every geometry
WHOLE_TRIPLES = [(1, 1, 1), (7, 3, 3), (26, 13, 13), (33, 4, 4), (64, 64, 64)]
# the 30-image list of test_decode_ragged_gpu.py
SIZES = [(32, 272), (40, 272), (45, 61), (64, 96), (24, 48), (173, 264)]
TRIPLES = [(1, 1, 1), (7, 3, 3), (8, 8, 5), (12, 6, 6), (16, 9, 16), (26, 13, 13), (32, 16, 16), (33, 4, 4), (5, 17, 2), (64, 64, 64)]
GOLDEN = ["tiny_q7", "tiny_q20", "odd_q7", "nat_q7", "s2odd_q7", "s1_q7"]


def _reference(oracle, u, v, H, W, ranks, f):
    from lrf_amd.codec import split_factors
    return reference_scaled(split_factors(u, v, (H, W), ranks), H, W, f, oracle)


def _alone(ctx, u, v, H, W, ranks, f):
    return ctx.decode_scaled(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), [(H, W, ranks, 0, 0)], f)[0]


def _table(items, us, vs):
    images, uo, vo = [], 0, 0
    for (H, W, ranks), u, v in zip(items, us, vs):
        images.append((H, W, ranks, uo, vo))
        uo += u.size
        vo += v.size
    return torch.from_numpy(np.concatenate(us)).cuda(), torch.from_numpy(np.concatenate(vs)).cuda(), images


_CASES = {}


def _whole_case(oracle, H, W, ranks, extremes=False):
    """(u, v, {f: reference}) of one whole-image case, made once.  The inputs are conditioned so that the comparison is not one
    of saturated bytes: the first seed of the case's sequence at which, at every scale, at least 5 % of the reference's bytes
    lie strictly between 0 and 255 (the first seed serves everywhere but on the few output pixels of the smallest sizes)."""
    key = (H, W, ranks, extremes)
    if key not in _CASES:
        for k in range(64):
            rng = np.random.default_rng(H * 1000 + W + ranks[0] + 7919 * k)
            u, v = random_factors(rng, H, W, ranks, lo=-128, hi=128, vlo=-1, vhi=2) if extremes else random_factors(rng, H, W, ranks)
            if extremes:
                u[:2] = (-128, 127)  # both ends of int8, whatever the draw
            refs = {f: _reference(oracle, u, v, H, W, ranks, f) for f in SCALES}
            if all(float(((r > 0) & (r < 255)).mean()) >= 0.05 for r in refs.values()):
                break
        else:
            raise AssertionError(f"no seed gives {H}x{W} at {ranks} unsaturated bytes")
        _CASES[key] = (u, v, refs)
    return _CASES[key]


def _check_whole(oracle, H, W, ranks, extremes=False):
    from lrf_amd import _lib
    ctx = _lib.context(0)
    u, v, refs = _whole_case(oracle, H, W, ranks, extremes)
    for f in SCALES:
        assert float(((refs[f] > 0) & (refs[f] < 255)).mean()) >= 0.05
        got = _alone(ctx, u, v, H, W, ranks, f)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3,) + scaled_dims(H, W, f)
        assert np.array_equal(got.cpu().numpy(), refs[f]), (H, W, ranks, f)


@pytest.mark.parametrize("ranks", WHOLE_TRIPLES, ids=lambda r: "r%d_%d_%d" % r)
@pytest.mark.parametrize("H,W", TILED + GENERAL)
def test_whole_images(oracle, H, W, ranks):
    _check_whole(oracle, H, W, ranks)


@pytest.mark.parametrize("ranks", [(3, 2, 2), (7, 3, 3)], ids=lambda r: "r%d_%d_%d" % r)
@pytest.mark.parametrize("H,W", [(32, 272), (64, 96), (45, 61), (173, 264)])
def test_int8_extremes(oracle, H, W, ranks):
    """U over all of int8, V in [-1, 1]: the largest u a byte holds, -128 included, through the unpacking and the integer sums"""
    u, v, refs = _whole_case(oracle, H, W, ranks, extremes=True)
    assert int(u.min()) == -128 and int(u.max()) == 127 and int(v.min()) == -1 and int(v.max()) == 1
    _check_whole(oracle, H, W, ranks, extremes=True)


@pytest.mark.parametrize("H,W", REFUSED)
def test_sizes_the_decoders_refuse_are_refused(H, W):
    from lrf_amd import _lib
    ctx = _lib.context(0)
    U, V = torch.zeros(4096, dtype=torch.int8, device="cuda"), torch.zeros(4096, dtype=torch.int8, device="cuda")
    for f in SCALES:
        with pytest.raises(ValueError):
            ctx.decode_scaled(U, V, [(H, W, (1, 1, 1), 0, 0)], f)
        with pytest.raises(ValueError):
            ctx.decode_scaled_crops(U, V, [(H, W, (1, 1, 1), 0, 0)], [(0, f, 0, 0)], (1, 1))
    with pytest.raises(ValueError):
        ctx.decode_rgb(U[None, :256], V[None, :192], H, W, [1, 1, 1])  # the full decoder too


def test_the_clamp_was_at_work_over_the_set(oracle):
    """0 and 255 both occur among the references of every geometry's cases, and of the extremes"""
    for H, W in TILED + GENERAL:
        seen = set()
        for ranks in WHOLE_TRIPLES:
            for r in _whole_case(oracle, H, W, ranks)[2].values():
                seen |= {int(r.min()), int(r.max())}
        assert {0, 255} <= seen, (H, W, seen)
    for H, W in [(32, 272), (64, 96), (45, 61), (173, 264)]:
        for ranks in [(3, 2, 2), (7, 3, 3)]:
            refs = _whole_case(oracle, H, W, ranks, extremes=True)[2]
            assert min(int(r.min()) for r in refs.values()) == 0 and max(int(r.max()) for r in refs.values()) == 255


class Mixed:
    """the 30 images' factors in two flat device buffers: made once"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from lrf_amd import _lib
            ctx = _lib.context(0)
            rng = np.random.default_rng(2024)
            items = [(H, W, TRIPLES[(2 * i + j) % len(TRIPLES)]) for j in range(5) for i, (H, W) in enumerate(SIZES)]
            fac = [random_factors(rng, *it) for it in items]
            us, vs = [f[0] for f in fac], [f[1] for f in fac]
            U, V, images = _table(items, us, vs)
            whole = {f: [w.cpu() for w in ctx.decode_scaled(U, V, images, f)] for f in SCALES}
            cls._made = (ctx, items, us, vs, U, V, images, whole)
        return cls._made


@pytest.mark.parametrize("f", SCALES)
def test_mixed_list(oracle, f):
    ctx, items, us, vs, U, V, images, whole = Mixed.get()
    assert len(whole[f]) == len(items)
    for i, (H, W, ranks) in enumerate(items):  # every launch group and class: each image as decoded alone
        assert tuple(whole[f][i].shape) == (3,) + scaled_dims(H, W, f)
        assert torch.equal(whole[f][i], _alone(ctx, us[i], vs[i], H, W, ranks, f).cpu()), (items[i], f)
    for i in (0, 3, 6, 14, 22, 29):  # six of them against the reference: three on the tiled kernel (classes 0, 4, 0), three on the general one
        H, W, ranks = items[i]
        assert np.array_equal(whole[f][i].numpy(), _reference(oracle, us[i], vs[i], H, W, ranks, f)), (items[i], f)
    perm = np.random.default_rng(f).permutation(len(items))
    Up, Vp, images_p = _table([items[j] for j in perm], [us[j] for j in perm], [vs[j] for j in perm])
    for j, got in zip(perm, ctx.decode_scaled(Up, Vp, images_p, f)):
        assert torch.equal(got.cpu(), whole[f][j])


@pytest.mark.parametrize("f", SCALES)
@pytest.mark.parametrize("H,W,ranks", [(64, 96, (7, 3, 3)), (64, 96, (26, 13, 13)), (45, 61, (7, 3, 3))], ids=["tiled_r7", "tiled_r26", "general_r7"])
def test_every_origin(H, W, ranks, f):
    """all windows of (5,7) of one scaled image in one call == the scaled whole image unfolded"""
    from lrf_amd import _lib
    ctx = _lib.context(0)
    u, v = random_factors(np.random.default_rng(H * 1000 + W + ranks[0] + f), H, W, ranks)
    whole = _alone(ctx, u, v, H, W, ranks, f)
    Hs, Ws = scaled_dims(H, W, f)
    h, w = 5, 7
    ys, xs = np.meshgrid(np.arange(Hs - h + 1), np.arange(Ws - w + 1), indexing="ij")
    boxes = np.stack([np.zeros(ys.size, dtype=np.int64), np.full(ys.size, f), ys.ravel(), xs.ravel()], axis=1)
    got = ctx.decode_scaled_crops(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), [(H, W, ranks, 0, 0)], boxes, (h, w))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (boxes.shape[0], 3, h, w)
    want = whole.unfold(1, h, 1).unfold(2, w, 1).permute(1, 2, 0, 3, 4).reshape(-1, 3, h, w)
    assert torch.equal(got, want)


def _boxes(items, size, seed):
    """per image its four corner windows plus four seeded random ones, each at a scale drawn from {2, 4, 8}"""
    h, w = size
    rng = np.random.default_rng(seed)
    out = []
    for i, (H, W, _) in enumerate(items):
        for k in range(8):
            f = int(rng.choice(SCALES))
            Hs, Ws = scaled_dims(H, W, f)
            y, x = ((0, 0), (0, Ws - w), (Hs - h, 0), (Hs - h, Ws - w))[k] if k < 4 else (int(rng.integers(0, Hs - h + 1)), int(rng.integers(0, Ws - w + 1)))
            out.append((i, f, y, x))
    return out


def _expected(whole, boxes, size):
    h, w = size
    return torch.stack([whole[f][i][:, y:y + h, x:x + w] for i, f, y, x in boxes])


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (2, 6)], ids=lambda s: "%dx%d" % s)
def test_mixed_windows_with_per_crop_scales(size):
    ctx, items, us, vs, U, V, images, whole = Mixed.get()
    boxes = _boxes(items, size, seed=size[0] * 100 + size[1])
    assert {b[1] for b in boxes} == set(SCALES)
    got = ctx.decode_scaled_crops(U, V, images, boxes, size).cpu()
    assert torch.equal(got, _expected(whole, boxes, size))


def test_whole_image_as_a_window():
    ctx, items, us, vs, U, V, images, whole = Mixed.get()
    for i in range(6):
        for f in SCALES:
            assert torch.equal(ctx.decode_scaled_crops(U, V, images, [(i, f, 0, 0)], scaled_dims(*items[i][:2], f))[0].cpu(), whole[f][i]), (items[i], f)


def test_independence_of_order_and_repetition():
    ctx, items, us, vs, U, V, images, whole = Mixed.get()
    size = (3, 5)
    boxes = _boxes(items, size, seed=1)
    got = ctx.decode_scaled_crops(U, V, images, boxes, size)
    perm = np.random.default_rng(2).permutation(len(boxes))
    assert torch.equal(ctx.decode_scaled_crops(U, V, images, [boxes[j] for j in perm], size), got[torch.from_numpy(perm).cuda()])
    twice = ctx.decode_scaled_crops(U, V, images, [boxes[5], boxes[100], boxes[5]], size)
    assert torch.equal(twice[0], got[5]) and torch.equal(twice[2], got[5]) and torch.equal(twice[1], got[100])
    assert torch.equal(ctx.decode_scaled_crops(U, V, images, [boxes[77]], size)[0], got[77])  # alone in its call


def test_back_to_back_calls_with_different_lists():
    """eight calls, eight box lists, no synchronisation in between: more calls than staging slots, and one pooled-table
    workspace that every call rewrites; the same after trim"""
    ctx, items, us, vs, U, V, images, whole = Mixed.get()
    size = (3, 5)
    for round_ in range(2):
        lists = [_boxes(items, size, seed=50 + 10 * round_ + k) for k in range(8)]
        torch.cuda.synchronize()
        outs = [ctx.decode_scaled_crops(U, V, images, b, size) for b in lists]
        for b, o in zip(lists, outs):
            assert torch.equal(o.cpu(), _expected(whole, b, size))
        ctx.trim()


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_golden_streams(oracle, inflate):
    import lrf_amd
    cases = [Case(n) for n in GOLDEN]
    streams = [c.encoded for c in cases]
    res = lrf_amd.qmf_load_factors(streams, inflate=inflate)
    full = [lrf_amd.qmf_decode(s) for s in streams]  # pinned to the reference's pixels by test_oracle_golden's sha256
    decodes = {1: [d.cuda() for d in full]}
    for f in SCALES:
        got = lrf_amd.qmf_decode_scaled(streams, f, inflate=inflate)
        decodes[f] = res.decode(scale=f)
        assert res.scaled_sizes(f) == [tuple(g.shape[1:]) for g in got]
        for c, g, r, whole in zip(cases, got, decodes[f], full):
            H, W = c.image.shape[-2:]
            ref = reference_scaled(c.ref_factors(), H, W, f, oracle)
            assert g.is_cuda and np.array_equal(g.cpu().numpy(), ref) and np.array_equal(r.cpu().numpy(), ref), (c.name, f)
            d = np.abs(ref.astype(np.float64) - block_average_u8(whole.cpu().numpy(), f))
            assert d.mean() <= 0.5 and (d > 1).mean() <= 0.01, (c.name, f, d.mean(), (d > 1).mean())
        assert all(torch.equal(a, b) for a, b in zip(lrf_amd.qmf_decode_scaled(res, f), got))
    assert all(torch.equal(a, b) for a, b in zip(res.decode(), decodes[1])) and all(torch.equal(a, b) for a, b in zip(res.decode(scale=1), decodes[1]))
    size = (4, 6)
    rng = np.random.default_rng(11)
    crops, scales = [], []
    for k in range(48):
        i, f = k % len(cases), (1, 2, 4, 8)[(k // len(cases)) % 4]
        hs, ws = decodes[f][i].shape[1:]
        crops.append((i, int(rng.integers(0, hs - size[0] + 1)), int(rng.integers(0, ws - size[1] + 1))))
        scales.append(f)
    want = torch.stack([decodes[f][i][:, y:y + size[0], x:x + size[1]] for (i, y, x), f in zip(crops, scales)])
    assert torch.equal(res.decode_crops(crops, size, scale=scales), want)
    assert torch.equal(lrf_amd.qmf_decode_crops(streams, crops, size, inflate=inflate, scale=scales), want)
    ones = [j for j, f in enumerate(scales) if f == 1]
    assert torch.equal(lrf_amd.qmf_decode_crops(res, [crops[j] for j in ones], size), want[ones])  # scale 1 is qmf_decode_crops as it is today


def test_c_entries_refuse_on_the_host_and_launch_nothing():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    lib = _lib.load()
    H, W, ranks, f, h, w = 64, 96, (7, 3, 3), 2, 5, 7
    Hs, Ws = scaled_dims(H, W, f)
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

    # ---- whole images
    npx = 3 * Hs * Ws
    rgb = torch.full((2 * npx,), 0xA5, dtype=torch.uint8, device="cuda")
    ok_images = [(H, W, ranks, 0, 0, 0), (H, W, ranks, nu, nv, npx)]

    def whole(images=ok_images, n=None, scale=f, u_len=2 * nu, v_len=2 * nv, rgb_len=2 * npx, u=U, v=V, out=rgb, null_images=False):
        ctx.use_torch_stream()
        return lib.lrf_qmf_decode_scaled_rgb_u8(ctx._h, len(images) if n is None else n, None if null_images else descs(images), scale, ptr(u), u_len,
                                                ptr(v), v_len, ptr(out), rgb_len)

    second = lambda **kw: [ok_images[0], tuple(kw.get(k, d) for k, d in zip(("H", "W", "ranks", "u_off", "v_off", "rgb_off"), ok_images[1]))]
    refused = {
        "NULL U": whole(u=None), "NULL V": whole(v=None), "NULL rgb": whole(out=None), "NULL images": whole(null_images=True),
        "n = 0": whole(n=0), "n = 65536": whole(n=65536),
        "scale 1": whole(scale=1), "scale 3": whole(scale=3), "scale 16": whole(scale=16), "scale 0": whole(scale=0), "scale -2": whole(scale=-2),
        "rank 0": whole(second(ranks=(7, 0, 3))), "rank 65": whole(second(ranks=(65, 3, 3))),
        "no size": whole(second(H=0)), "1x1": whole(second(H=1, W=1)), "size 2^31": whole(second(H=2 ** 31)),
        "u range": whole(u_len=2 * nu - 1), "v range": whole(v_len=2 * nv - 1), "rgb range": whole(rgb_len=2 * npx - 1),
        "u offset past the end": whole(second(u_off=nu + 1)), "negative u": whole(second(u_off=-1)), "negative v": whole(second(v_off=-1)),
        "negative rgb": whole(second(rgb_off=-1)), "rgb offset past the end": whole(second(rgb_off=npx + 1)),
        "offset near 2^63": whole(second(u_off=2 ** 63 - 1)), "rgb offset near 2^63": whole(second(rgb_off=2 ** 63 - 1)),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    torch.cuda.synchronize()
    assert bool((rgb == 0xA5).all()), "a refused call wrote to its output"
    assert whole() == 0  # and the same call with the arguments right runs
    torch.cuda.synchronize()
    assert not bool((rgb == 0xA5).any())  # zero factors: every byte of the two images was written

    # ---- windows
    npx = 3 * h * w
    rgb = torch.full((3 * npx,), 0xA5, dtype=torch.uint8, device="cuda")
    ok_crops = [(0, 2, 0, 0), (1, 2, Hs - h, Ws - w), (1, 8, 3, 5)]  # 64x96 at 1/8: 8x12

    def crops_call(images=ok_images, crops=ok_crops, n_images=None, n_crops=None, size=(h, w), u_len=2 * nu, v_len=2 * nv, rgb_len=3 * npx, u=U, v=V, out=rgb,
                   null_images=False, null_crops=False):
        cr = (_lib.ScaledCrop * max(1, len(crops)))()
        for c, (i, s, y, x) in zip(cr, crops):
            c.image, c.scale, c.y0, c.x0 = i, s, y, x
        ctx.use_torch_stream()
        return lib.lrf_qmf_decode_scaled_crops_rgb_u8(ctx._h, len(images) if n_images is None else n_images, None if null_images else descs(images), ptr(u),
                                                      u_len, ptr(v), v_len, len(crops) if n_crops is None else n_crops, None if null_crops else cr, size[0],
                                                      size[1], ptr(out), rgb_len)

    third = lambda c: ok_crops[:2] + [c]
    refused = {
        "NULL U": crops_call(u=None), "NULL V": crops_call(v=None), "NULL rgb": crops_call(out=None), "NULL images": crops_call(null_images=True),
        "NULL crops": crops_call(null_crops=True),
        "n_images = 0": crops_call(n_images=0), "n_images = 65536": crops_call(n_images=65536),
        "n_crops = 0": crops_call(n_crops=0), "n_crops = 2^20 + 1": crops_call(n_crops=2 ** 20 + 1),
        "h = 0": crops_call(size=(0, w)), "w = 0": crops_call(size=(h, 0)), "h < 0": crops_call(size=(-h, w)),
        "scale 1": crops_call(crops=third((0, 1, 0, 0))), "scale 3": crops_call(crops=third((0, 3, 0, 0))), "scale 16": crops_call(crops=third((0, 16, 0, 0))),
        "image index 2": crops_call(crops=third((2, 2, 0, 0))), "image index -1": crops_call(crops=third((-1, 2, 0, 0))),
        "y0 < 0": crops_call(crops=third((0, 2, -1, 0))), "x0 < 0": crops_call(crops=third((0, 2, 0, -1))),
        "past the bottom": crops_call(crops=third((0, 2, Hs - h + 1, 0))), "past the right": crops_call(crops=third((0, 2, 0, Ws - w + 1))),
        "inside the image, outside its scaled size": crops_call(crops=third((0, 8, 4, 0))),
        "taller than the scaled image": crops_call(crops=[(0, 2, 0, 0)], size=(Hs + 1, w), rgb_len=2 ** 40), "near 2^31": crops_call(crops=[(0, 2, 2 ** 31 - 1, 0)]),
        "rank 0": crops_call(images=second(ranks=(7, 0, 3))), "rank 65": crops_call(images=second(ranks=(65, 3, 3))),
        "no size": crops_call(images=second(H=0)), "1x1": crops_call(images=second(H=1, W=1)),
        "u range": crops_call(u_len=2 * nu - 1), "v range": crops_call(v_len=2 * nv - 1), "rgb range": crops_call(rgb_len=3 * npx - 1),
        "u offset past the end": crops_call(images=second(u_off=nu + 1)), "negative v": crops_call(images=second(v_off=-1)),
        "offset near 2^63": crops_call(images=second(u_off=2 ** 63 - 1)),
    }
    assert all(rc == -1 for rc in refused.values()), refused
    torch.cuda.synchronize()
    assert bool((rgb == 0xA5).all()), "a refused call wrote to its output"
    assert crops_call() == 0
    torch.cuda.synchronize()
    assert not bool((rgb == 0xA5).any())
    images5 = [im[:5] for im in ok_images]
    with pytest.raises(ValueError):
        ctx.decode_scaled_crops(U, V, images5, [(0, 2, Hs - h + 1, 0)], (h, w))
    with pytest.raises(TypeError):
        ctx.decode_scaled_crops(U, V, images5, [(0.0, 2.0, 0.0, 0.0)], (h, w))
    with pytest.raises(ValueError):
        ctx.decode_scaled(U, V, images5, 3)


def test_at_the_loaders_shape(oracle):
    from lrf_amd import _lib
    ctx = _lib.context(0)
    n, H, W, ranks = 64, 512, 768, (7, 3, 3)
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    g = torch.Generator().manual_seed(n)
    Uh = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g)
    Vh = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g)
    U, V = Uh.cuda().reshape(-1), Vh.cuda().reshape(-1)
    images = [(H, W, ranks, b * nu, b * nv) for b in range(n)]
    rng = np.random.default_rng(n)
    for f, size in ((2, (224, 224)), (8, (56, 56))):
        whole = ctx.decode_scaled(U, V, images, f)
        Hs, Ws = scaled_dims(H, W, f)
        for b in (0, 31, 63):
            assert np.array_equal(whole[b].cpu().numpy(), _reference(oracle, Uh[b].numpy(), Vh[b].numpy(), H, W, ranks, f)), (b, f)
        boxes = np.stack([np.arange(n), np.full(n, f), rng.integers(0, Hs - size[0] + 1, n), rng.integers(0, Ws - size[1] + 1, n)], axis=1)
        got = ctx.decode_scaled_crops(U, V, images, boxes, size)
        want = torch.stack([whole[b][:, y:y + size[0], x:x + size[1]] for b, _, y, x in boxes])
        assert torch.equal(got, want), f
