"""The gray loader on the GPU: lrf_qmf_decode_gray_ragged_u8, lrf_qmf_decode_gray_crops_u8, lrf_qmf_decode_gray_resized_crops_u8,
their _tensor forms and the Python entry points that route lists of gray streams to them.  Every comparison is bitwise against the
exact-integer numpy definitions of tests/gray_loader.py (test_gray_loader.py checks those against the reference's fixtures)."""
import ctypes

import numpy as np
import pytest
import torch

import gray_loader as gl
from tensor_format import bits, boxes_of, staged
from test_channels import GRAY8_CASES, ChanCase

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
P = ctypes.POINTER


class Loaded:
    """a list of cases as flat factors on the device, with the definitions of their levels (computed once, on demand)"""

    def __init__(self, cases):
        from lrf_amd import _lib
        self.cases = cases
        self.images, Uh, Vh = gl.flat_list(cases)
        self.ctx = _lib.context(0)
        self.U, self.V = torch.from_numpy(Uh).cuda(), torch.from_numpy(Vh).cuda()
        self._levels = {}

    def level(self, i, f):
        if (i, f) not in self._levels:
            H, W, R, tone = self.cases[i]
            self._levels[(i, f)] = gl.level(*gl.case_factors(H, W, R, tone), H, W, f)
        return self._levels[(i, f)]

    def factors(self, i):
        return gl.case_factors(*self.cases[i])


@pytest.fixture(scope="module")
def everything():
    return Loaded(gl.shuffled_cases())


# the crops, the resized crops and the tensor forms: one image per size and a spread of ranks and tones; (45, 61) and (9, 9) are the
# odd geometries of the colour suite's box lists
SOME = [(37, 53, 7, "mid"), (64, 96, 9, "dark"), (173, 264, 64, "bright"), (56, 440, 17, "mid"), (16, 24, 4, "mid"), (45, 61, 26, "mid"),
        (9, 9, 64, "dark"), (173, 264, 7, "mid")]


@pytest.fixture(scope="module")
def some():
    return Loaded(SOME)


def raw_ragged(ld, scale, out, offs, images=None, u_len=None, v_len=None, out_len=None):
    """lrf_qmf_decode_gray_ragged_u8 itself, with the caller's offsets -> its return code"""
    from lrf_amd import _lib
    desc = _lib._gray_images(ld.images if images is None else images, offs)
    ld.ctx.use_torch_stream()
    return ld.ctx._lib.lrf_qmf_decode_gray_ragged_u8(ld.ctx._h, len(desc), desc, scale, ctypes.c_void_p(ld.U.data_ptr()), ld.U.numel() if u_len is None else u_len,
                                                     ctypes.c_void_p(ld.V.data_ptr()), ld.V.numel() if v_len is None else v_len,
                                                     ctypes.c_void_p(out.data_ptr()), out.numel() if out_len is None else out_len)


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("scale", gl.LEVELS)
def test_ragged_decode_is_the_definition_and_touches_nothing_else(everything, scale, base):
    """all sizes x ranks x tones shuffled into one list; the output base aligned and one byte past alignment, three sentinel bytes
    between images: the whole buffer must equal the one built on the host"""
    ld = everything
    offs, off = [], 2
    for i in range(len(ld.cases)):
        offs.append(off)
        off += ld.level(i, scale).size + 3
    want = np.full(off, SENTINEL, np.uint8)
    for i, o in enumerate(offs):
        L = ld.level(i, scale)
        want[o:o + L.size] = L.reshape(-1)
    buf = torch.full((off + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[base:base + off]
    assert out.data_ptr() % 16 == base
    assert raw_ragged(ld, scale, out, offs) == 0
    got = buf.cpu().numpy()
    ld.ctx.check()
    assert np.array_equal(got[base:base + off], want)
    assert (got[:base] == SENTINEL).all() and (got[base + off:] == SENTINEL).all()


def test_ragged_decode_equals_the_uniform_decoder_called_for_each_image_alone(everything):
    ld = everything
    got = ld.ctx.decode_gray_ragged(ld.U, ld.V, ld.images)
    assert [tuple(g.shape) for g in got] == [(1, H, W) for H, W, *_ in ld.images] and all(g.data_ptr() % 16 == 0 for g in got)
    for g, (H, W, R, u_off, v_off) in zip(got, ld.images):
        M = gl.patches(H, W)
        alone = ld.ctx.decode_gray(ld.U[u_off:u_off + M * R].view(1, M, R), ld.V[v_off:v_off + 64 * R].view(1, 64, R), H, W)
        assert torch.equal(g, alone)


WINDOWS = [(1, 1), (3, 5), (16, 16), (13, 37)]


def window_list(ld, h, w):
    """(image, scale, y0, x0) of every image and level the window fits: the corners, origins that straddle patches, the last row
    and column; the scales alternate down the list"""
    rows = []
    for i, (H, W, *_) in enumerate(ld.images):
        top, left = (gl.padded(H, W)[0] - H) // 2, (gl.padded(H, W)[1] - W) // 2
        for f in gl.LEVELS:
            Hs, Ws = gl.scaled_dims(H, W, f)
            if h > Hs or w > Ws:
                continue
            ys = {0, Hs - h, min(Hs - h, 5), min(Hs - h, 7), min(Hs - h, max(0, 8 - top)), (Hs - h) // 2}
            xs = {0, Ws - w, min(Ws - w, 6), min(Ws - w, 7), min(Ws - w, max(0, 8 - left)), (Ws - w) // 3}
            rows += [(i, f, y, x) for y in sorted(ys) for x in sorted(xs)]
    order = np.random.default_rng(h * 100 + w).permutation(len(rows))
    return np.array([rows[k] for k in order], dtype=np.int64)


@pytest.mark.parametrize("size", WINDOWS)
def test_crops_of_mixed_scales_in_one_call_are_slices_of_their_levels(some, size):
    ld, (h, w) = some, size
    rows = window_list(ld, h, w)
    assert set(rows[:, 1].tolist()) == {1, 2, 4, 8} or size == (13, 37)
    got = ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, size).cpu().numpy()
    ld.ctx.check()
    assert got.shape == (len(rows), 1, h, w)
    for g, (i, f, y0, x0) in zip(got, rows.tolist()):
        assert np.array_equal(g[0], ld.level(i, f)[y0:y0 + h, x0:x0 + w]), (i, f, y0, x0)


def box_list(ld, size):
    """(image, y0, x0, hb, wb, flip) over the colour suite's box lists on its four geometries, flips alternating"""
    rows = []
    for i, (H, W, *_) in enumerate(ld.images):
        if (H, W) in ((64, 96), (45, 61), (9, 9), (173, 264)):
            rows += [(i, *b, (k + i) & 1) for k, b in enumerate(boxes_of(H, W, size, 7 * i + size[0]))]
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("flipped", [False, True])
@pytest.mark.parametrize("size", [(5, 7), (17, 33)])
def test_resized_crops_are_the_definition_on_both_paths(some, size, flipped):
    ld = some
    rows = box_list(ld, size)
    if flipped:
        rows[:, 5] ^= 1
    paths = {staged(hb, wb, *size) for _, _, _, hb, wb, _ in rows.tolist()}
    assert paths == {True, False}
    got = ld.ctx.decode_gray_resized_crops(ld.U, ld.V, ld.images, rows, size).cpu().numpy()
    ld.ctx.check()
    assert got.shape == (len(rows), 1) + size
    for g, (i, y0, x0, hb, wb, flip) in zip(got, rows.tolist()):
        H, W, *_ = ld.images[i]
        assert np.array_equal(g[0], gl.resized(*ld.factors(i), H, W, (y0, x0, hb, wb), size, bool(flip))), (i, y0, x0, hb, wb, flip)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_tensor_forms_are_two_roundings_then_the_conversion(some, dtype):
    """mean 0.449, std 0.226: a contracted multiply-add differs on 124 of the 256 byte values (test_gray_loader.py), so a fused
    kernel fails.  Crops of mixed scales and resized crops; out= into a slice of a larger batch; channels_last the same memory"""
    ld = some
    scale, bias = gl.constants(gl.MEAN, gl.STD)
    rows = window_list(ld, 13, 37)
    b = ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (13, 37))
    want = gl.tensor_of(b.cpu().numpy(), scale, bias, dtype)
    assert len(np.unique(b.cpu().numpy())) >= 100
    got = ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (13, 37), dtype=dtype, mean=gl.MEAN, std=gl.STD)
    assert got.dtype == dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))
    nhwc = ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (13, 37), dtype=dtype, mean=[gl.MEAN], std=(gl.STD,), channels_last=True)
    assert torch.equal(bits(nhwc), bits(want)) and nhwc.stride()[0] == 13 * 37 and nhwc.stride()[2:] == (37, 1)
    n = len(rows)
    big = torch.full((n + 5, 1, 13, 37), 7.0, dtype=dtype, device="cuda")
    res = ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (13, 37), dtype=dtype, mean=gl.MEAN, std=gl.STD, out=big[2:2 + n])
    assert res.data_ptr() == big[2:2 + n].data_ptr() and torch.equal(bits(big[2:2 + n]), bits(want))
    assert (big[:2] == 7.0).all() and (big[2 + n:] == 7.0).all()
    for size in ((5, 7), (17, 33)):
        boxes = box_list(ld, size)
        b = ld.ctx.decode_gray_resized_crops(ld.U, ld.V, ld.images, boxes, size)
        want = gl.tensor_of(b.cpu().numpy(), scale, bias, dtype)
        got = ld.ctx.decode_gray_resized_crops(ld.U, ld.V, ld.images, boxes, size, dtype=dtype, mean=gl.MEAN, std=gl.STD)
        assert torch.equal(bits(got), bits(want))
        big = torch.full((len(boxes) + 3, 1) + size, 7.0, dtype=dtype, device="cuda")
        ld.ctx.decode_gray_resized_crops(ld.U, ld.V, ld.images, boxes, size, dtype=dtype, mean=gl.MEAN, std=gl.STD, channels_last=True, out=big[3:])
        assert torch.equal(bits(big[3:]), bits(want)) and (big[:3] == 7.0).all()
    plain = ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (13, 37), dtype=dtype)  # to-tensor alone: b / 255
    assert torch.equal(bits(plain), bits(gl.tensor_of(ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (13, 37)).cpu().numpy(), *gl.constants(), dtype)))
    ld.ctx.check()


def test_the_python_entry_points_route_gray_lists(some):
    """the fixtures' streams plus streams of qmf_encode_batch(gray, color_space="RGB") of two sizes: every result equals qmf_decode
    of the stream put through the definition"""
    import lrf_amd
    from lrf_amd.codec import ResidentFactors, _two_factor_parts
    g = torch.Generator().manual_seed(9)
    streams = [ChanCase(n).encoded for n in GRAY8_CASES]
    for shape in ((2, 1, 24, 40), (3, 1, 37, 53)):
        streams += lrf_amd.qmf_encode_batch(torch.randint(0, 256, shape, dtype=torch.uint8, generator=g), color_space="RGB", quality=20)
    decoded = [lrf_amd.qmf_decode(s).numpy() for s in streams]
    facs = []
    for s, d in zip(streams, decoded):
        _, u, v, (C, H, W, _, R) = _two_factor_parts(s)
        facs.append((np.asarray(u, np.int8), np.asarray(v, np.int8), H, W))
        assert C == 1 and d.shape == (1, H, W) and np.array_equal(gl.level(*facs[-1], 1), d[0])
    got = lrf_amd.qmf_decode_ragged(streams)
    assert len(got) == len(streams) and all(x.is_cuda and x.dtype == torch.uint8 for x in got)
    assert all(np.array_equal(x.cpu().numpy(), d) for x, d in zip(got, decoded))
    rf = lrf_amd.qmf_load_factors(streams)
    assert isinstance(rf, ResidentFactors) and rf.channels == 1 and len(rf) == len(streams) and rf.sizes == [(f[2], f[3]) for f in facs]
    assert all(np.array_equal(x.cpu().numpy(), d) for x, d in zip(rf.decode(), decoded))
    for f in (2, 4, 8):
        want = [gl.level(*fc, f) for fc in facs]
        assert rf.scaled_sizes(f) == [w.shape for w in want]
        for res in (rf.decode(f), lrf_amd.qmf_decode_scaled(rf, f), lrf_amd.qmf_decode_scaled(streams, f)):
            assert all(x.shape == (1,) + w.shape and np.array_equal(x.cpu().numpy()[0], w) for x, w in zip(res, want))
    crops = [(i, 1, 2) for i in range(len(streams)) if facs[i][2] >= 16 and facs[i][3] >= 16] + [(0, 0, 0), (1, 0, 0)]
    scales = [(1, 2, 4)[k % 3] for k in range(len(crops))]
    for src in (rf, streams):
        one = lrf_amd.qmf_decode_crops(src, crops, (3, 5))
        assert one.shape == (len(crops), 1, 3, 5)
        assert all(np.array_equal(c.cpu().numpy(), decoded[i][:, y:y + 3, x:x + 5]) for c, (i, y, x) in zip(one, crops))
        mixed = lrf_amd.qmf_decode_crops(src, crops, (3, 5), scale=scales)
        assert all(np.array_equal(c.cpu().numpy()[0], gl.level(*facs[i], f)[y:y + 3, x:x + 5]) for c, (i, y, x), f in zip(mixed, crops, scales))
    boxes = [(i, 1, 0, facs[i][2] - 1, facs[i][3] - 1) for i in range(len(streams))] + [(0, 3, 4, 8, 8)]
    flips = [bool(k & 1) for k in range(len(boxes))]
    for src in (rf, streams):
        res = lrf_amd.qmf_decode_resized_crops(src, boxes, (5, 7), flip=flips)
        assert res.shape == (len(boxes), 1, 5, 7)
        for r, (i, y0, x0, hb, wb), fl in zip(res, boxes, flips):
            u, v, H, W = facs[i]
            assert np.array_equal(r.cpu().numpy()[0], gl.resized(u, v, H, W, (y0, x0, hb, wb), (5, 7), fl))
    scale, bias = gl.constants(gl.MEAN, gl.STD)
    t = lrf_amd.qmf_decode_resized_crops(rf, boxes, (5, 7), flip=flips, dtype=torch.float16, mean=gl.MEAN, std=[gl.STD])
    assert torch.equal(bits(t), bits(gl.tensor_of(lrf_amd.qmf_decode_resized_crops(rf, boxes, (5, 7), flip=flips).cpu().numpy(), scale, bias, torch.float16)))
    rf._ctx.check()


def test_every_entry_on_a_callers_stream_behind_queued_work(some):
    """the factors reach their buffers on a side stream, behind queued matmuls; each entry, set on that stream with
    lrf_ctx_set_stream (Context.use_torch_stream), must read them there: the default-stream results, bit for bit"""
    ld = some
    rows, boxes = window_list(ld, 3, 5), box_list(ld, (5, 7))
    calls = [lambda U, V: torch.cat([x.reshape(-1) for x in ld.ctx.decode_gray_ragged(U, V, ld.images, 1)]),
             lambda U, V: torch.cat([x.reshape(-1) for x in ld.ctx.decode_gray_ragged(U, V, ld.images, 4)]),
             lambda U, V: ld.ctx.decode_gray_crops(U, V, ld.images, rows, (3, 5)),
             lambda U, V: ld.ctx.decode_gray_crops(U, V, ld.images, rows, (3, 5), dtype=torch.bfloat16, mean=gl.MEAN, std=gl.STD),
             lambda U, V: ld.ctx.decode_gray_resized_crops(U, V, ld.images, boxes, (5, 7)),
             lambda U, V: ld.ctx.decode_gray_resized_crops(U, V, ld.images, boxes, (5, 7), dtype=torch.float16, mean=gl.MEAN, std=gl.STD)]
    want = [c(ld.U, ld.V).cpu() for c in calls]
    Us, Vs = torch.zeros_like(ld.U), torch.zeros_like(ld.V)
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        for _ in range(8):
            a = (a @ a).clamp_(-1, 1)
        Us.copy_(ld.U, non_blocking=True)
        Vs.copy_(ld.V, non_blocking=True)
        got = [c(Us, Vs) for c in calls]
    S.synchronize()
    ld.ctx.check()
    torch.cuda.synchronize()
    ld.ctx.use_torch_stream()  # back on the default stream for the tests that follow
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu().view(torch.uint8), w.view(torch.uint8))


def test_the_loaders_shape_sixty_four_images_one_random_resized_crop_each():
    """64 x 512x768 at rank 7, one RandomResizedCrop box each (area 8 % .. 100 %, aspect 3/4 .. 4/3) to 224x224: all staged"""
    from lrf_amd import _lib
    rng = np.random.default_rng(21)
    H, W, R, n = 512, 768, 7, 64
    M = gl.patches(H, W)
    u = rng.integers(-6, 6, (n, M, R), dtype=np.int8)
    v = rng.integers(-6, 6, (n, 64, R), dtype=np.int8)
    u[:, :, 0], v[:, :, 0] = 8, 15
    images = [(H, W, R, i * M * R, i * 64 * R) for i in range(n)]
    boxes = []
    for i in range(n):
        area, ratio = H * W * rng.uniform(0.08, 1.0), np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        wb, hb = min(W, max(1, int(round(np.sqrt(area * ratio))))), min(H, max(1, int(round(np.sqrt(area / ratio)))))
        boxes.append((i, int(rng.integers(0, H - hb + 1)), int(rng.integers(0, W - wb + 1)), hb, wb, i & 1))
    assert all(staged(b[3], b[4], 224, 224) for b in boxes)
    ctx = _lib.context(0)
    got = ctx.decode_gray_resized_crops(torch.from_numpy(u.reshape(-1)).cuda(), torch.from_numpy(v.reshape(-1)).cuda(), images, boxes, (224, 224)).cpu().numpy()
    ctx.check()
    for g, (i, y0, x0, hb, wb, flip) in zip(got, boxes):
        assert np.array_equal(g[0], gl.resized(u[i], v[i], H, W, (y0, x0, hb, wb), (224, 224), bool(flip))), i


def test_refused_calls_write_nothing_and_leave_the_context_clean(some):
    from lrf_amd import _lib
    ld, lib = some, some.ctx._lib
    poison = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    ld.ctx.use_torch_stream()
    U, V, nu, nv = ctypes.c_void_p(ld.U.data_ptr()), ctypes.c_void_p(ld.V.data_ptr()), ld.U.numel(), ld.V.numel()
    out = ctypes.c_void_p(poison.data_ptr())
    two = ld.images[:2]  # 37x53 rank 7 and 64x96 rank 9
    desc = _lib._gray_images(two)
    refused = 0

    def refuse(rc):
        nonlocal refused
        assert rc == -1, rc
        with pytest.raises(ValueError):
            _lib.check(rc)
        ld.ctx.check()
        refused += 1

    # the whole-image entry
    for images, scale, kw in ((two, 3, {}), (two, 0, {}), (two, 1, dict(out_len=37 * 53 + 64 * 96 - 1)), ([(37, 53, 65, 0, 0)], 1, {}), ([(37, 53, 0, 0, 0)], 1, {}),
                              ([(3, 53, 7, 0, 0)], 1, {}), ([(0, 53, 7, 0, 0)], 1, {}), ([(37, 53, 7, -1, 0)], 1, {}), ([(37, 53, 7, 0, -1)], 1, {}),
                              (two, 1, dict(u_len=two[1][3] + 96 * 9 - 1)), (two, 2, dict(v_len=two[1][4] + 64 * 9 - 1)), ([(37, 53, 7, nu - 244, 0)], 1, {})):
        offs = [0, 37 * 53][:len(images)]
        refuse(raw_ragged(ld, scale, poison, offs, images=images, **kw))
    refuse(raw_ragged(ld, 1, poison, [-1, 5000], images=two))
    refuse(raw_ragged(ld, 8, poison, [0, poison.numel() - 8 * 12 + 1], images=two))
    refuse(lib.lrf_qmf_decode_gray_ragged_u8(ld.ctx._h, 0, desc, 1, U, nu, V, nv, out, poison.numel()))
    refuse(lib.lrf_qmf_decode_gray_ragged_u8(ld.ctx._h, 2, desc, 1, None, nu, V, nv, out, poison.numel()))
    # the crops entries
    crop = lambda rows: np.ascontiguousarray(rows, dtype=np.int32).ctypes.data_as(P(_lib.ScaledCrop))
    for rows, h, w, kw in (([(0, 1, 34, 0)], 4, 4, {}), ([(0, 1, 0, 50)], 4, 4, {}), ([(0, 2, 16, 0)], 4, 4, {}), ([(0, 8, 0, 4)], 4, 4, {}), ([(2, 1, 0, 0)], 4, 4, {}),
                           ([(-1, 1, 0, 0)], 4, 4, {}), ([(0, 3, 0, 0)], 4, 4, {}), ([(0, 1, -1, 0)], 4, 4, {}), ([(0, 1, 0, 0)], 0, 4, {}), ([(0, 1, 0, 0)], 38, 4, {}),
                           ([(0, 1, 0, 0)] * 3, 4, 4, dict(out_len=47)), ([(0, 1, 0, 0)], 4, 4, dict(n_crops=0)), ([(0, 1, 0, 0)], 4, 4, dict(n_crops=(1 << 20) + 1))):
        refuse(lib.lrf_qmf_decode_gray_crops_u8(ld.ctx._h, 2, desc, U, nu, V, nv, kw.get("n_crops", len(rows)), crop(rows), h, w, out, kw.get("out_len", poison.numel())))
    fmt = _lib.check_tensor_format(torch.float16, gl.MEAN, gl.STD)
    rows = crop([(0, 1, 0, 0)])
    good = lambda f=fmt, o=out, nb=poison.numel(): lib.lrf_qmf_decode_gray_crops_tensor(ld.ctx._h, 2, desc, U, nu, V, nv, 1, rows, 4, 4, ctypes.byref(f) if f else None, o, nb)
    refuse(good(f=None))
    refuse(good(o=ctypes.c_void_p(poison.data_ptr() + 1)))  # not aligned to the 2-byte elements
    refuse(good(nb=31))  # 16 elements of 2 bytes
    for field, value in (("dtype", 3), ("layout", 2)):
        bad = _lib.check_tensor_format(torch.float16, gl.MEAN, gl.STD)
        setattr(bad, field, value)
        refuse(good(f=bad))
    bad = _lib.check_tensor_format(torch.float16, gl.MEAN, gl.STD)
    bad.scale[2] = float("inf")
    refuse(good(f=bad))
    # the resized entries
    box = lambda rows: np.ascontiguousarray(rows, dtype=np.int32).ctypes.data_as(P(_lib.ResizedCrop))
    for rows, oh, ow, kw in (([(0, 0, 0, 38, 5, 0)], 5, 7, {}), ([(0, 30, 0, 8, 5, 0)], 5, 7, {}), ([(0, 0, 50, 5, 4, 0)], 5, 7, {}), ([(0, 0, 0, 0, 5, 0)], 5, 7, {}),
                             ([(0, 0, 0, 5, 0, 0)], 5, 7, {}), ([(2, 0, 0, 5, 5, 0)], 5, 7, {}), ([(0, -1, 0, 5, 5, 0)], 5, 7, {}), ([(0, 0, 0, 5, 5, 0)], 0, 7, {}),
                             ([(0, 0, 0, 5, 5, 0)], 5, 16385, {}), ([(0, 0, 0, 5, 5, 0)] * 2, 5, 7, dict(out_len=69))):
        refuse(lib.lrf_qmf_decode_gray_resized_crops_u8(ld.ctx._h, 2, desc, U, nu, V, nv, len(rows), box(rows), oh, ow, out, kw.get("out_len", poison.numel())))
    refuse(lib.lrf_qmf_decode_gray_resized_crops_tensor(ld.ctx._h, 2, desc, U, nu, V, nv, 1, box([(0, 0, 0, 5, 5, 0)]), 5, 7, ctypes.byref(fmt), out, 69))
    torch.cuda.synchronize()
    assert refused >= 40 and bool((poison == SENTINEL).all())
    # and the same buffers decode once the arguments are good
    assert lib.lrf_qmf_decode_gray_crops_u8(ld.ctx._h, 2, desc, U, nu, V, nv, 1, crop([(0, 1, 33, 49)]), 4, 4, out, 16) == 0
    assert np.array_equal(poison[:16].cpu().numpy().reshape(4, 4), ld.level(0, 1)[33:37, 49:53]) and bool((poison[16:] == SENTINEL).all())
    ld.ctx.check()


def test_descriptors_stay_resident_and_trim_releases_them(some):
    """the same image list again uploads nothing new; after lrf_ctx_trim the table is gone and the next call brings it back"""
    ld = some
    rows = window_list(ld, 3, 5)
    want = ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (3, 5)).cpu()
    before = ld.ctx.workspace_bytes()
    assert torch.equal(ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (3, 5)).cpu(), want) and ld.ctx.workspace_bytes() == before
    ld.ctx.trim()
    assert ld.ctx.workspace_bytes() == 0
    assert torch.equal(ld.ctx.decode_gray_crops(ld.U, ld.V, ld.images, rows, (3, 5)).cpu(), want)
    sub = ld.images[2:5]  # another list: another table under the same buffer
    got = ld.ctx.decode_gray_ragged(ld.U, ld.V, sub, 2)
    assert all(np.array_equal(g.cpu().numpy()[0], ld.level(2 + k, 2)) for k, g in enumerate(got))
    ld.ctx.check()
