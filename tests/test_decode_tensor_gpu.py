"""GPU suite (-m gpu): the decode entries that write a model's tensor — dtype=, mean=, std=, channels_last=, out= of
Context.decode_crops / decode_scaled_crops / decode_resized_crops, ResidentFactors and lrf_amd.qmf_decode_*crops, and the C entries
lrf_qmf_decode_*_tensor.  The expected value is the definition on the CPU (tests/tensor_format.py: apply_format) applied to
  resized crops           reference_resized over the CPU oracle's levels — this one does not go through the uint8 kernels
  crops, scaled crops     the bytes of the _rgb_u8 entry for the same list, which the existing tests pin to the oracle
with the ImageNet constants; test_decode_tensor_host.py shows that these inputs meet at least 100 byte values per channel on which
a fused multiply-add would differ.  Every comparison is bitwise, on the values viewed as int16 / int32."""
import ctypes

import numpy as np
import pytest
import torch

import tensor_format as tf
from resized_decode import reference_resized, resized_level
from scaled_decode import reference_scaled
from tensor_format import FORMAT_IDS, FORMATS, IMAGENET_MEAN, IMAGENET_STD

pytestmark = pytest.mark.gpu
SCALE, BIAS = tf.constants(IMAGENET_MEAN, IMAGENET_STD)
NORM = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD)


def _ctx():
    from lrf_amd import _lib
    return _lib.context(0)


def _same(got, b, dtype, channels_last, what=None):
    """got: the entry's tensor; b: uint8 [n, 3, h, w] on the CPU (numpy or torch), the bytes the definition is applied to"""
    want = tf.apply_format(b, SCALE, BIAS, dtype)
    assert got.is_cuda and got.dtype == dtype and tuple(got.shape) == tuple(want.shape), what
    assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format), what
    bad = tf.bits(got) != tf.bits(want)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())


class Levels:
    """the level images of one case's factors over the CPU oracle, each made when first asked for"""

    def __init__(self, oracle, H, W, ranks):
        from lrf_amd.codec import split_factors
        self.u, self.v = tf.case_factors(H, W, ranks)
        self.oracle, self.f6, self.H, self.W, self.made = oracle, split_factors(self.u, self.v, (H, W), ranks), H, W, {}

    def __getitem__(self, f):
        if f not in self.made:
            self.made[f] = (self.oracle.planes_to_rgb(self.f6[0::2], self.f6[1::2], self.H, self.W) if f == 1
                            else reference_scaled(self.f6, self.H, self.W, f, self.oracle))
        return self.made[f]

    def resized(self, box, size, flip):
        return reference_resized(self[resized_level(box[2], box[3], *size)], box, size, flip)


_LEVELS = {}


def _levels(oracle, H, W, ranks):
    if (H, W, ranks) not in _LEVELS:
        _LEVELS[(H, W, ranks)] = Levels(oracle, H, W, ranks)
    return _LEVELS[(H, W, ranks)]


@pytest.mark.parametrize("ranks", tf.RESIZED_TRIPLES, ids=lambda r: "r%d_%d_%d" % r)
@pytest.mark.parametrize("H,W", tf.RESIZED_GEOMETRIES)
def test_resized_crops_against_the_definition_over_the_oracle(oracle, H, W, ranks):
    """every format x both output sizes x the box list, flips on and off"""
    ctx, lv = _ctx(), _levels(oracle, H, W, ranks)
    U, V, images = torch.from_numpy(lv.u).cuda(), torch.from_numpy(lv.v).cuda(), [(H, W, ranks, 0, 0)]
    for size in tf.RESIZED_SIZES:
        rows = [(0,) + b + (flip,) for b in tf.boxes_of(H, W, size, seed=H + W + size[0]) for flip in (0, 1)]
        want = np.stack([lv.resized(r[1:5], size, r[5]) for r in rows])
        for dtype, cl in FORMATS:
            _same(ctx.decode_resized_crops(U, V, images, rows, size, dtype=dtype, channels_last=cl, **NORM), want, dtype, cl, (size, dtype, cl))


def test_resized_crops_meet_every_level_and_both_paths(oracle):
    """173x264: the box list meets levels 1, 2, 4, 8 and both the staged and the direct kernels, for bfloat16 NHWC"""
    H, W, ranks = tf.BIG
    ctx, lv = _ctx(), _levels(oracle, H, W, ranks)
    U, V, images = torch.from_numpy(lv.u).cuda(), torch.from_numpy(lv.v).cuda(), [(H, W, ranks, 0, 0)]
    for size in tf.RESIZED_SIZES:
        boxes = tf.boxes_of(H, W, size, seed=H + W + size[0])
        assert {resized_level(b[2], b[3], *size) for b in boxes} == {1, 2, 4, 8} and {tf.staged(b[2], b[3], *size) for b in boxes} == {True, False}
        rows = [(0,) + b + (flip,) for b in boxes for flip in (0, 1)]
        want = np.stack([lv.resized(r[1:5], size, r[5]) for r in rows])
        _same(ctx.decode_resized_crops(U, V, images, rows, size, dtype=torch.bfloat16, channels_last=True, **NORM), want, torch.bfloat16, True, size)


def _origins(Hs, Ws, h, w):
    """window origins in an Hs x Ws image: aligned ((0, 0), (8, 16) where it fits), odd, the far corner"""
    out = [(0, 0), (Hs - h, Ws - w)]
    for y, x in ((8, 16), (1, 3), (7, 9)):
        if y + h <= Hs and x + w <= Ws:
            out.append((y, x))
    return sorted(set(out))


@pytest.mark.parametrize("H,W,ranks", tf.CROP_CASES, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_crops_and_scaled_crops_against_the_uint8_entries(H, W, ranks):
    """every format x the window sizes x scales 1, 2, 4, 8, at odd and aligned origins"""
    from lrf_amd import _lib
    ctx = _ctx()
    u, v = tf.case_factors(H, W, ranks)
    U, V, images = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), [(H, W, ranks, 0, 0)]
    ran = set()
    for f in (1, 2, 4, 8):
        Hs, Ws = (H, W) if f == 1 else _lib.scaled_dims(H, W, f)
        for h, w in tf.WINDOWS:
            if h > Hs or w > Ws:
                continue
            ran.add((f, h, w))
            if f == 1:
                crops = [(0, y, x) for y, x in _origins(Hs, Ws, h, w)]
                call = ctx.decode_crops
            else:
                crops = [(0, f, y, x) for y, x in _origins(Hs, Ws, h, w)]
                call = ctx.decode_scaled_crops
            b = call(U, V, images, crops, (h, w)).cpu()
            for dtype, cl in FORMATS:
                _same(call(U, V, images, crops, (h, w), dtype=dtype, channels_last=cl, **NORM), b, dtype, cl, (f, h, w, dtype, cl))
    assert {(f, 1, 1) for f in (1, 2, 4, 8)} | {(f, 3, 5) for f in (1, 2, 4, 8)} | {(1, 16, 16), (1, 13, 37), (2, 16, 16)} <= ran


class Mixed:
    """the five crop cases as one resident list, made once"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from lrf_amd import _lib
            from lrf_amd.codec import ResidentFactors
            us, vs, images, uo, vo = [], [], [], 0, 0
            for H, W, ranks in tf.CROP_CASES:
                u, v = tf.case_factors(H, W, ranks)
                images.append((H, W, ranks, uo, vo))
                us.append(u)
                vs.append(v)
                uo, vo = uo + u.size, vo + v.size
            U, V = torch.from_numpy(np.concatenate(us)).cuda(), torch.from_numpy(np.concatenate(vs)).cuda()
            cls._made = (ResidentFactors(_lib.context(0), U, V, images), images)
        return cls._made


def test_per_crop_scales_through_resident_factors():
    """ResidentFactors.decode_crops(scale=[1, 2, 8, ...]): the two entries' results merged in call order, in every format"""
    rf, images = Mixed.get()
    crops = [(0, 3, 5), (1, 1, 2), (2, 0, 0), (3, 2, 1), (4, 0, 1), (0, 9, 30), (3, 0, 0)]
    scale = [1, 2, 8, 1, 4, 1, 8]
    size = (3, 5)
    b = rf.decode_crops(crops, size, scale=scale).cpu()
    for dtype, cl in FORMATS:
        _same(rf.decode_crops(crops, size, scale=scale, dtype=dtype, channels_last=cl, **NORM), b, dtype, cl, (dtype, cl))
    _same(rf.decode_crops(crops, size, scale=2, dtype=torch.float16, **NORM), rf.decode_crops(crops, size, scale=2).cpu(), torch.float16, False)
    out = torch.full((9, 3) + size, -7.0, dtype=torch.float32, device="cuda")
    got = rf.decode_crops(crops, size, scale=scale, dtype=torch.float32, out=out[1:8], **NORM)
    assert got.data_ptr() == out[1:8].data_ptr()
    _same(got, b, torch.float32, False)
    assert bool((out[0] == -7.0).all()) and bool((out[8] == -7.0).all())


def _mixed_rows():
    """resized rows over the five images: levels 1 to 8, both paths, flips"""
    _, images = Mixed.get()
    rng = np.random.default_rng(5)
    rows = []
    for i, (H, W, *_rest) in enumerate(images):
        for y0, x0, hb, wb in [(0, 0, H, W), (H - 5, W - 7, 5, 7), (1, 2, 11, 15), (H - 8, 0, 8, W)] + tf.boxes_of(H, W, (5, 7), i)[-2:]:
            rows.append((i, y0, x0, hb, wb, int(rng.integers(0, 2))))
    return rows


def test_a_mixed_list_in_one_call():
    """images of both geometries and all five rank classes in one call of each entry == the definition on the uint8 entry's bytes"""
    import lrf_amd
    rf, images = Mixed.get()
    rows = _mixed_rows()
    boxes, flips = [r[:5] for r in rows], [bool(r[5]) for r in rows]
    b = rf.decode_resized_crops(boxes, (5, 7), flips).cpu()
    for dtype, cl in ((torch.float16, True), (torch.bfloat16, False), (torch.float32, True)):
        _same(rf.decode_resized_crops(boxes, (5, 7), flips, dtype=dtype, channels_last=cl, **NORM), b, dtype, cl)
    _same(lrf_amd.qmf_decode_resized_crops(rf, boxes, (5, 7), flips, dtype=torch.float16, **NORM), b, torch.float16, False)
    crops = [(i, y, x) for i, (H, W, *_r) in enumerate(images) for y, x in ((0, 0), (H - 13, W - 37), (5, 3))]
    b = rf.decode_crops(crops, (13, 37)).cpu()
    for dtype, cl in ((torch.float16, False), (torch.bfloat16, True), (torch.float32, False)):
        _same(rf.decode_crops(crops, (13, 37), dtype=dtype, channels_last=cl, **NORM), b, dtype, cl)
    _same(lrf_amd.qmf_decode_crops(rf, crops, (13, 37), dtype=torch.bfloat16, channels_last=True, **NORM), b, torch.bfloat16, True)
    sc = [(i, f, y, x) for i in range(len(images)) for f, y, x in ((2, 0, 0), (2, 5, 3), (4, 1, 2), (8, 0, 1))]
    b = rf._ctx.decode_scaled_crops(rf.U, rf.V, images, sc, (3, 5)).cpu()
    for dtype, cl in ((torch.float16, True), (torch.bfloat16, False), (torch.float32, True)):
        _same(rf._ctx.decode_scaled_crops(rf.U, rf.V, images, sc, (3, 5), dtype=dtype, channels_last=cl, **NORM), b, dtype, cl)
    # mean / std None and scalars: the plain to-tensor, and one pair for all channels
    got = rf.decode_crops(crops, (13, 37), dtype=torch.float32)
    assert torch.equal(got.cpu(), rf.decode_crops(crops, (13, 37)).cpu().float().mul(float(np.float32(1.0 / 255.0))))
    s1, b1 = tf.constants(0.5, 0.25)
    got = rf.decode_crops(crops, (13, 37), dtype=torch.float16, mean=0.5, std=0.25)
    assert torch.equal(tf.bits(got), tf.bits(tf.apply_format(rf.decode_crops(crops, (13, 37)).cpu(), s1, b1, torch.float16)))


def test_independence_of_order_and_repetition():
    """a crop's bits are the same alone, first or last, for each entry"""
    rf, images = Mixed.get()
    ctx, U, V = rf._ctx, rf.U, rf.V
    rows = _mixed_rows()
    for dtype, cl in ((torch.bfloat16, True), (torch.float32, False)):
        kw = dict(dtype=dtype, channels_last=cl, **NORM)
        for entry, lst, size in ((ctx.decode_resized_crops, rows, (5, 7)),
                                 (ctx.decode_crops, [(i, 1, 2) for i in range(len(images))] + [(0, 8, 16), (3, 0, 0)], (13, 37)),
                                 (ctx.decode_scaled_crops, [(i, f, 1, 1) for i in range(len(images)) for f in (2, 4, 8)], (3, 5))):
            whole = entry(U, V, images, lst, size, **kw)
            for j in (0, len(lst) // 2, len(lst) - 1):
                alone = entry(U, V, images, [lst[j]], size, **kw)
                assert torch.equal(tf.bits(alone[0]), tf.bits(whole[j])), (entry.__name__, j)
                first_last = entry(U, V, images, [lst[j]] + lst[:3] + [lst[j]], size, **kw)
                assert torch.equal(tf.bits(first_last[0]), tf.bits(whole[j])) and torch.equal(tf.bits(first_last[-1]), tf.bits(whole[j])), (entry.__name__, j)
            perm = np.random.default_rng(2).permutation(len(lst))
            assert torch.equal(tf.bits(entry(U, V, images, [lst[j] for j in perm], size, **kw)), tf.bits(whole)[torch.from_numpy(perm)])


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
def test_out_is_written_in_place_and_nothing_around_it(cl):
    rf, images = Mixed.get()
    ctx, U, V = rf._ctx, rf.U, rf.V
    rows = _mixed_rows()[:9]
    fmt = torch.channels_last if cl else torch.contiguous_format
    for dtype, sentinel in ((torch.float16, 1234.0), (torch.float32, -5.5), (torch.bfloat16, 96.0)):
        for entry, lst, size in ((ctx.decode_resized_crops, rows, (5, 7)), (ctx.decode_crops, [(i % 5, 1, 2) for i in range(9)], (3, 5)),
                                 (ctx.decode_scaled_crops, [(i % 5, 2 << (i % 3), 0, 1) for i in range(9)], (3, 5))):
            big = torch.full((len(lst) + 4, 3) + size, sentinel, dtype=dtype, device="cuda").contiguous(memory_format=fmt)
            part = big[2:2 + len(lst)]
            got = entry(U, V, images, lst, size, dtype=dtype, channels_last=cl, out=part, **NORM)
            assert got is part and got.data_ptr() == big[2].data_ptr()
            assert got.is_contiguous(memory_format=fmt) or len(lst) == 1
            fresh = entry(U, V, images, lst, size, dtype=dtype, channels_last=cl, **NORM)
            assert fresh.is_contiguous(memory_format=fmt)
            assert torch.equal(tf.bits(big[2:2 + len(lst)]), tf.bits(fresh))
            assert bool((big[:2] == sentinel).all()) and bool((big[2 + len(lst):] == sentinel).all()), "bytes around the slice were written"
    # anything else is refused before a launch: the output keeps its sentinel
    big = torch.full((9, 3, 5, 7), 3.0, dtype=torch.float16, device="cuda").contiguous(memory_format=fmt)
    other = torch.channels_last if not cl else torch.contiguous_format
    bad = [big[:8], big.float(), big[:, :, :, :5], big.cpu(), big.contiguous(memory_format=other), big[:, :, ::1, :].permute(0, 1, 3, 2), "x"]
    for o in bad:
        with pytest.raises((ValueError, TypeError)):
            ctx.decode_resized_crops(U, V, images, rows, (5, 7), dtype=torch.float16, channels_last=cl, out=o, **NORM)
    with pytest.raises(ValueError):
        ctx.decode_resized_crops(U, V, images, rows, (5, 7), out=big)  # out= goes with a float dtype
    for kw in (dict(mean=0.5), dict(std=0.5), dict(channels_last=True)):
        with pytest.raises(ValueError):
            rf.decode_crops([(0, 0, 0)], (3, 5), dtype=torch.uint8, **kw)
    torch.cuda.synchronize()
    assert bool((big == 3.0).all())


def test_defaults_are_the_uint8_entries(oracle):
    """without the new arguments every Python call returns the uint8 tensor of the old C entry, bit for bit"""
    import lrf_amd
    from lrf_amd import _lib
    rf, images = Mixed.get()
    ctx, U, V, lib = rf._ctx, rf.U, rf.V, _lib.load()
    desc = _lib._ragged_images(_lib.check_ragged_args(U, V, images))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rows = np.ascontiguousarray(_mixed_rows(), dtype=np.int32)
    out = torch.empty((len(rows), 3, 5, 7), dtype=torch.uint8, device="cuda")
    ctx.use_torch_stream()
    assert lib.lrf_qmf_decode_resized_crops_rgb_u8(ctx._h, len(images), desc, ptr(U), U.numel(), ptr(V), V.numel(), len(rows),
                                                   rows.ctypes.data_as(ctypes.POINTER(_lib.ResizedCrop)), 5, 7, ptr(out), out.numel()) == 0
    for got in (ctx.decode_resized_crops(U, V, images, rows, (5, 7)), rf.decode_resized_crops(rows[:, :5], (5, 7), rows[:, 5].astype(bool)),
                lrf_amd.qmf_decode_resized_crops(rf, rows[:, :5], (5, 7), rows[:, 5].astype(bool)),
                ctx.decode_resized_crops(U, V, images, rows, (5, 7), dtype=torch.uint8)):
        assert got.dtype == torch.uint8 and torch.equal(got, out)
    crops = np.ascontiguousarray([(i, 1, 2) for i in range(len(images))], dtype=np.int32)
    out = torch.empty((len(crops), 3, 13, 37), dtype=torch.uint8, device="cuda")
    assert lib.lrf_qmf_decode_crops_rgb_u8(ctx._h, len(images), desc, ptr(U), U.numel(), ptr(V), V.numel(), len(crops),
                                           crops.ctypes.data_as(ctypes.POINTER(_lib.Crop)), 13, 37, ptr(out), out.numel()) == 0
    for got in (ctx.decode_crops(U, V, images, crops, (13, 37)), rf.decode_crops(crops, (13, 37)), lrf_amd.qmf_decode_crops(rf, crops, (13, 37))):
        assert got.dtype == torch.uint8 and torch.equal(got, out)
    sc = np.ascontiguousarray([(i, 2, 1, 2) for i in range(len(images))], dtype=np.int32)
    out = torch.empty((len(sc), 3, 3, 5), dtype=torch.uint8, device="cuda")
    assert lib.lrf_qmf_decode_scaled_crops_rgb_u8(ctx._h, len(images), desc, ptr(U), U.numel(), ptr(V), V.numel(), len(sc),
                                                  sc.ctypes.data_as(ctypes.POINTER(_lib.ScaledCrop)), 3, 5, ptr(out), out.numel()) == 0
    for got in (ctx.decode_scaled_crops(U, V, images, sc, (3, 5)), rf.decode_crops(sc[:, [0, 2, 3]], (3, 5), scale=2)):
        assert got.dtype == torch.uint8 and torch.equal(got, out)
    # and those bytes are the oracle's: the first image's window against the CPU decode
    H, W, ranks = tf.CROP_CASES[0]
    u, v = tf.case_factors(H, W, ranks)
    assert np.array_equal(rf.decode_crops([(0, 1, 2)], (13, 37))[0].cpu().numpy(), tf.oracle_image(oracle, u, v, H, W, ranks)[:, 1:14, 2:39])


def test_c_entries_refuse_on_the_host_and_launch_nothing():
    """every new LRF_EINVAL of the three entries: nothing is launched, a sentinel-filled output stays untouched"""
    from lrf_amd import _lib
    rf, images = Mixed.get()
    ctx, U, V, lib = rf._ctx, rf.U, rf.V, _lib.load()
    desc = _lib._ragged_images(_lib.check_ragged_args(U, V, images))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    n, h, w = 3, 5, 7
    lists = {
        "crops": (lib.lrf_qmf_decode_crops_tensor, np.ascontiguousarray([(0, 0, 0), (3, 1, 2), (4, 40, 54)], dtype=np.int32), _lib.Crop),
        "scaled": (lib.lrf_qmf_decode_scaled_crops_tensor, np.ascontiguousarray([(0, 2, 0, 0), (3, 4, 1, 1), (4, 2, 17, 23)], dtype=np.int32), _lib.ScaledCrop),
        "resized": (lib.lrf_qmf_decode_resized_crops_tensor, np.ascontiguousarray([(0, 0, 0, 64, 96, 0), (3, 1, 2, 11, 15, 1), (4, 37, 0, 8, 61, 0)], dtype=np.int32),
                    _lib.ResizedCrop),
    }
    words = torch.full((n * 3 * h * w + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # room for float32 and a misaligned start

    def fmt(dtype=_lib.T_F16, layout=_lib.T_NCHW, scale=(0.017, 0.017, 0.017), bias=(-2.0, -2.0, -1.8)):
        f = _lib.TensorFormat()
        f.dtype, f.layout = dtype, layout
        for k in range(3):
            f.scale[k], f.bias[k] = scale[k], bias[k]
        return f

    for name, (entry, lst, ctype) in lists.items():
        def call(f=fmt(), out=words.data_ptr(), out_bytes=None, null_fmt=False):
            es = 4 if f.dtype == _lib.T_F32 else 2
            ctx.use_torch_stream()
            return entry(ctx._h, len(images), desc, ptr(U), U.numel(), ptr(V), V.numel(), n, lst.ctypes.data_as(ctypes.POINTER(ctype)), h, w,
                         None if null_fmt else ctypes.byref(f), ctypes.c_void_p(out) if out is not None else None,
                         n * 3 * h * w * es if out_bytes is None else out_bytes)
        nan, inf = float("nan"), float("inf")
        refused = {
            "NULL fmt": call(null_fmt=True), "NULL out": call(out=None),
            "dtype 3": call(fmt(dtype=3)), "dtype -1": call(fmt(dtype=-1)), "layout 2": call(fmt(layout=2)), "layout -1": call(fmt(layout=-1)),
            "nan scale": call(fmt(scale=(0.017, nan, 0.017))), "inf scale": call(fmt(scale=(inf, 0.017, 0.017))), "-inf scale": call(fmt(scale=(0.017, 0.017, -inf))),
            "nan bias": call(fmt(bias=(nan, 0.0, 0.0))), "inf bias": call(fmt(bias=(0.0, 0.0, inf))),
            "f16 at an odd address": call(out=words.data_ptr() + 1), "bf16 at an odd address": call(fmt(dtype=_lib.T_BF16), out=words.data_ptr() + 3),
            "f32 at 2 mod 4": call(fmt(dtype=_lib.T_F32), out=words.data_ptr() + 2), "f32 at 1 mod 4": call(fmt(dtype=_lib.T_F32), out=words.data_ptr() + 1),
            "f16 one byte short": call(out_bytes=n * 3 * h * w * 2 - 1), "f16 one element short": call(out_bytes=n * 3 * h * w * 2 - 2),
            "f32 sized for f16": call(fmt(dtype=_lib.T_F32), out_bytes=n * 3 * h * w * 2), "f32 one byte short": call(fmt(dtype=_lib.T_F32), out_bytes=n * 3 * h * w * 4 - 1),
            "out_bytes 0": call(out_bytes=0), "out_bytes < 0": call(out_bytes=-(2 ** 62)), "out_bytes -1": call(out_bytes=-1),
        }
        assert all(rc == -1 for rc in refused.values()), (name, refused)
        torch.cuda.synchronize()
        assert bool((words == 0x5A5A5A5A).all()), f"{name}: a refused call wrote to its output"
        # and the same call with the arguments right runs, at an address aligned to the element and to nothing more
        for f, off in ((fmt(), 2), (fmt(dtype=_lib.T_BF16, layout=_lib.T_NHWC), 6), (fmt(dtype=_lib.T_F32), 4)):
            es = 4 if f.dtype == _lib.T_F32 else 2
            assert call(f, out=words.data_ptr() + off, out_bytes=2 ** 62 if es == 4 else None) == 0, name
            torch.cuda.synchronize()
            raw = words.view(torch.uint8)
            ne = n * 3 * h * w * es
            assert bool((raw[:off] == 0x5A).all()) and bool((raw[off + ne:] == 0x5A).all()), f"{name}: wrote outside its {ne} bytes"
            assert not bool((raw[off:off + ne].view(torch.int16) == 0x5A5A).all())
            words.fill_(0x5A5A5A5A)


class Busy:
    """a chain of 4096^3 matmuls sized once to about 60 ms (the pattern of test_caller_stream_gpu.py)"""
    MIN_MS = 20.0

    def __init__(self):
        g = torch.Generator(device="cuda").manual_seed(1)
        self.a = torch.randn((4096, 4096), device="cuda", generator=g) / 128.0
        self.b = torch.randn((4096, 4096), device="cuda", generator=g)
        self.c = torch.empty_like(self.b)
        self._timed(4)
        per = min(self._timed(32) for _ in range(3)) / 32
        self.n = int(3 * self.MIN_MS / per) + 1

    def _timed(self, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.queue(n)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def queue(self, n=None):
        x, y = self.b, self.c
        for _ in range(n or self.n):
            torch.mm(self.a, x, out=y)
            x, y = y, x
        self.b, self.c = x, y


def test_on_a_side_stream_behind_queued_work():
    """One call per entry on a side stream: the factor buffers hold a decoy; on the stream a producer of at least 20 ms is queued,
    behind it the copy of the real factors, the call, a clone of its result and the decoy again.  A call that ran ahead of its
    stream, or left work behind on another one, gives the decoy's values."""
    from lrf_amd.codec import ResidentFactors
    rf, images = Mixed.get()
    g = torch.Generator().manual_seed(11)
    decoy = [torch.randint(-16, 16, (t.numel(),), dtype=torch.int8, generator=g).cuda() for t in (rf.U, rf.V)]
    U, V = decoy[0].clone(), decoy[1].clone()
    side = ResidentFactors(rf._ctx, U, V, images)
    rows = _mixed_rows()
    calls = [
        lambda r: r.decode_resized_crops([x[:5] for x in rows], (17, 33), [bool(x[5]) for x in rows], dtype=torch.float16, channels_last=True, **NORM),
        lambda r: r.decode_crops([(i, 1, 2) for i in range(len(images))], (13, 37), dtype=torch.bfloat16, **NORM),
        lambda r: r.decode_crops([(i, 1, 1) for i in range(len(images))], (3, 5), scale=[2, 4, 8, 2, 4], dtype=torch.float32, channels_last=True, **NORM),
    ]
    want = [c(rf) for c in calls]
    wrong = [c(side) for c in calls]
    assert all(not torch.equal(tf.bits(a), tf.bits(b)) for a, b in zip(want, wrong))
    busy = Busy()
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(S):
        e0.record()
        busy.queue()
        e1.record()
        U.copy_(rf.U)
        V.copy_(rf.V)
        snaps = [c(side).clone() for c in calls]
        U.copy_(decoy[0])
        V.copy_(decoy[1])
    S.synchronize()
    assert e0.elapsed_time(e1) >= Busy.MIN_MS
    for got, w in zip(snaps, want):
        assert got.dtype == w.dtype and torch.equal(tf.bits(got), tf.bits(w))
