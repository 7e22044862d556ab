"""GPU suite (-m gpu): buffers that pass 2^31 and 2^32 bytes.  The descriptor-table entry points get hand-made tables whose
u_off / v_off / rgb_off / src_off / dst_off lie at, across and past P31 = 2^31 and P32 = 2^32 (tests/far_offsets.py: `roles`), each
image's three offsets in different regions; the uniform decoder gets a batch whose output passes P32.  The work is eight small
images; only the addresses are large.  Expected bytes: the same entry point on a compact copy of the same items, and the CPU
oracle / the numpy definitions / the host deflate restatement and zlib on every far item.  Every comparison is byte equality,
and the bytes of the output between the placed items must still carry the sentinel pattern.

Memory: the module holds three buffers of P32 + 2^26 bytes (about 13 GB) — one int8 buffer of random factors that serves as U, V
and the deflate source, and two uint8 buffers that carry the sentinel pattern and take the outputs (the second, viewed as int8
where an entry point writes factors or matrices) — and never more than these three; the uniform decoder writes into the first
output buffer.  They are freed when the module ends.

Not reached from here: the crop entry points write [n][3][h][w] back to back from the output pointer (no offset in the table):
their output passes P32 only from 2^20 crops of 37x37 on, the list's limit, so their U and V offsets are far and their output is
small; a uniform decode on the tiled bodies whose U alone passes 2^31 bytes (their factors are at most a fifth of their
pixels: over 10 GB of output, so `(long)blockIdx.y * u_img` in k_decode16 / k_decode_strip / k_decode8 rests on reading) — the
any-size body is given such a U; the host -> host pipe.  test_any_shape_planes_past_p31_floats holds 8.9 GB of X alone, before the
three buffers exist."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import deflate_cases as dc
import far_offsets as fo
from far_offsets import BIG, EIGHT, P31, P32
from resized_decode import reference_resized, resized_level
from scaled_decode import reference_scaled

pytestmark = pytest.mark.gpu


class Far:
    def __init__(self):
        g = torch.Generator(device="cuda").manual_seed(31)
        self.src = torch.randint(-16, 16, (BIG,), dtype=torch.int8, device="cuda", generator=g)
        self.pat = torch.randint(0, 256, (fo.PAT,), dtype=torch.uint8, device="cuda", generator=g)
        self.out = torch.empty((BIG,), dtype=torch.uint8, device="cuda")
        self.aux = torch.empty((BIG,), dtype=torch.uint8, device="cuda")
        fo.fill_pattern(self.out, self.pat)
        fo.fill_pattern(self.aux, self.pat)
        self.cache = {}


@pytest.fixture(scope="module")
def far():
    f = Far()
    yield f
    del f.src, f.out, f.aux, f.pat
    f.cache.clear()
    torch.cuda.empty_cache()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _sizes():
    from lrf_amd import _lib
    usz = [sum(d[4] * r for d, r in zip(_lib.plane_dims(H, W), ranks)) for H, W, ranks in EIGHT]
    vsz = [64 * sum(ranks) for _, _, ranks in EIGHT]
    return usz, vsz, [3 * H * W for H, W, _ in EIGHT]


def _table(uo, vo, ro):
    from lrf_amd import _lib
    desc = (_lib.RaggedImage * len(EIGHT))()
    for d, (H, W, ranks), u, v, r in zip(desc, EIGHT, uo, vo, ro):
        d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, int(u), int(v), int(r)
        d.R[0], d.R[1], d.R[2] = ranks
    return desc


def _gather(buf, offs, sizes, coffs, n, fill=0):
    """the items of `buf` at `offs` copied to `coffs` of a new buffer of n elements"""
    small = torch.full((n,), fill, dtype=buf.dtype, device=buf.device)
    for o, s, c in zip(offs, sizes, coffs):
        small[int(c):int(c) + int(s)] = buf[int(o):int(o) + int(s)]
    return small


def _factors(far, variant):
    """the placement of the eight images' factors in far.src for a variant — U at role i, V at role i + 3 — its compact copy, and
    what the oracle decodes from them: made once per variant"""
    key = ("factors", variant)
    if key not in far.cache:
        from lrf_amd.codec import split_factors
        usz, vsz, _ = _sizes()
        uo, vo = fo.place(usz, variant, 0), fo.place(vsz, variant, 3)
        assert fo.covers(uo, usz) and fo.covers(vo, vsz)
        cu, nu = fo.compact(uo, usz)
        cv, nv = fo.compact(vo, vsz)
        Uc, Vc = _gather(far.src, uo, usz, cu, nu), _gather(far.src, vo, vsz, cv, nv)
        f6 = [split_factors(Uc[int(c):int(c) + s].cpu().numpy(), Vc[int(d):int(d) + t].cpu().numpy(), (H, W), ranks)
              for (H, W, ranks), c, s, d, t in zip(EIGHT, cu, usz, cv, vsz)]
        far.cache[key] = dict(uo=uo, vo=vo, cu=cu, cv=cv, Uc=Uc, Vc=Vc, f6=f6)
    return far.cache[key]


def _full(far, variant, oracle):
    """the oracle's full decode of the eight images of a variant"""
    key = ("full", variant)
    if key not in far.cache:
        far.cache[key] = [oracle.planes_to_rgb(f[0::2], f[1::2], H, W) for f, (H, W, _) in zip(_factors(far, variant)["f6"], EIGHT)]
    return far.cache[key]


def _level(far, variant, i, f, oracle):
    """image i of a variant at 1/f by the numpy definition (f = 1: the oracle's decode)"""
    if f == 1:
        return _full(far, variant, oracle)[i]
    key = ("level", variant, i, f)
    if key not in far.cache:
        H, W, _ = EIGHT[i]
        far.cache[key] = reference_scaled(_factors(far, variant)["f6"][i], H, W, f, oracle)
    return far.cache[key]


def _check_placed(far, buf, offs, sizes, small, coffs, what):
    """the far call's items equal the compact call's, and nothing else of the far buffer was written; puts the pattern back"""
    view = buf.view(small.dtype)  # (buf: one of the uint8 pattern buffers)
    for i, (o, s, c) in enumerate(zip(offs, sizes, coffs)):
        assert torch.equal(view[int(o):int(o) + int(s)], small[int(c):int(c) + int(s)]), (what, i, int(o))
    ranges = [(int(o), int(o) + int(s)) for o, s in zip(offs, sizes)]
    ok = fo.gaps_untouched(buf, far.pat, ranges)
    fo.restore(buf, far.pat, ranges)
    assert ok, f"{what}: bytes outside the placed items were written"


def _tile16_kept(ro):
    """does an image with sides multiples of 16 sit at a multiple of 8, so that the 16-aligned body takes part in the call?"""
    return any(int(r) % 8 == 0 for (H, W, _), r in zip(EIGHT, ro) if H % 16 == 0 and W % 16 == 0)


def test_any_shape_planes_past_p31_floats(oracle):
    """lrf_qmf_planes_any_hw_u8 with X past 2^31 floats (8.9 GB).  The entry point takes the chroma plane's size apart from the
    image's: 65,535 images of 9x11 (19 MB) with a chroma plane of 182x183 and 4x4 patches (padded to 184x184) give 33,856 floats an
    image, 2.22e9 in all; image 63,430 lies across 2^31 floats and across 2^33 bytes.  Stands first in the module and does not ask
    for `far`: X is alone in memory and freed before the three buffers are made.  Eight random images repeated cyclically: every
    image's matrix has the bits of its twin's in a call of eight, and the images 0, middle, last and the one across 2^31 floats
    equal oracle.anyshape_matrices.  Refusals: a matrix or an image whose launch would need more than 2^31 - 1 workgroups."""
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    H, W, chroma, patch, B = 9, 11, (182, 183), (4, 4), 65535
    d = _lib.plane_dims_any(H, W, patch, chroma)[1]
    per = d[4] * d[5]
    assert (d[2], d[3]) == (184, 184) and per == 33856 and B * per > P31 and P31 % per
    g = torch.Generator(device="cuda").manual_seed(12)
    rgb8 = torch.randint(0, 256, (8, 3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    rgb = rgb8.repeat(-(-B // 8), 1, 1, 1)[:B].contiguous()
    X8 = ctx.planes_any(rgb8, patch, 1, chroma).view(8, per)
    X = rows = None
    try:
        X = ctx.planes_any(rgb, patch, 1, chroma)
        rows = X.view(B, per)
        twins = X8.repeat(512, 1).view(torch.int32)
        for k in range(0, B, 4096):
            n = min(4096, B - k)
            same = torch.equal(rows[k:k + n].view(torch.int32), twins[:n])
            assert same, k
        del twins
        across = P31 // per
        assert across * per < P31 < (across + 1) * per
        want = {s: oracle.anyshape_matrices(rgb8[s].cpu().numpy(), patch, chroma)[1] for s in range(8)}
        for b in sorted({0, B // 2, across - 1, across, across + 1, B - 1}):
            got = rows[b].cpu().numpy().reshape(d[4], d[5])
            assert got.dtype == want[b % 8].dtype and np.array_equal(got.view(np.int32), want[b % 8].view(np.int32)), b
        X2 = ctx.planes_any(rgb[B - 16:], patch, 2, chroma)  # Cr, the last images
        for j in (0, 15):
            w2 = oracle.anyshape_matrices(rgb8[(B - 16 + j) % 8].cpu().numpy(), patch, chroma)[2]
            assert np.array_equal(X2[j].cpu().numpy().view(np.int32), w2.view(np.int32)), j
    finally:
        del X, rows
        torch.cuda.empty_cache()
    # limits that are stated: nothing is launched, so small buffers stand in
    tiny = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    ctx.use_torch_stream()
    rc = lib.lrf_qmf_planes_any_hw_u8(ctx._h, _ptr(tiny), 1, 2 ** 20, 2 ** 20, 0, 0, 0, 0, 0, _ptr(tiny))
    assert rc == -2 and b"more than 2^31 - 1 workgroups" in lib.lrf_last_error()
    R = (ctypes.c_int * 3)(1, 1, 1)
    rc = lib.lrf_qmf_decode_any_hw_u8(ctx._h, *([_ptr(tiny)] * 6), 1, 2 ** 20, 2 ** 20, 0, 0, 0, 0, R, _ptr(tiny))
    assert rc == -2 and b"more than 2^31 - 1 workgroups" in lib.lrf_last_error()


@pytest.mark.parametrize("variant", [0, 1])
def test_decode_ragged(far, oracle, variant):
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    fx = _factors(far, variant)
    _, _, rsz = _sizes()
    ro = fo.place(rsz, variant, 5)
    assert fo.covers(ro, rsz) and _tile16_kept(ro)
    cr, nr = fo.compact(ro, rsz)
    small = torch.full((nr,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.use_torch_stream()
    _lib.check(lib.lrf_qmf_decode_ragged_rgb_u8(ctx._h, 8, _table(fx["cu"], fx["cv"], cr), _ptr(fx["Uc"]), fx["Uc"].numel(), _ptr(fx["Vc"]),
                                                fx["Vc"].numel(), _ptr(small), nr))
    _lib.check(lib.lrf_qmf_decode_ragged_rgb_u8(ctx._h, 8, _table(fx["uo"], fx["vo"], ro), _ptr(far.src), BIG, _ptr(far.src), BIG, _ptr(far.out), BIG))
    for i, ((H, W, _), o, s) in enumerate(zip(EIGHT, ro, rsz)):  # the oracle on every far item
        assert np.array_equal(far.out[int(o):int(o) + s].cpu().numpy().reshape(3, H, W), _full(far, variant, oracle)[i]), (i, int(o))
    _check_placed(far, far.out, ro, rsz, small, cr, "decode_ragged")


@pytest.mark.parametrize("variant,scale", [(0, 2), (1, 4), (1, 8)])
def test_decode_scaled(far, oracle, variant, scale):
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    fx = _factors(far, variant)
    dims = [_lib.scaled_dims(H, W, scale) for H, W, _ in EIGHT]
    rsz = [3 * h * w for h, w in dims]
    ro = fo.place(rsz, variant, 5)
    assert fo.covers(ro, rsz)
    cr, nr = fo.compact(ro, rsz)
    small = torch.full((nr,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.use_torch_stream()
    _lib.check(lib.lrf_qmf_decode_scaled_rgb_u8(ctx._h, 8, _table(fx["cu"], fx["cv"], cr), scale, _ptr(fx["Uc"]), fx["Uc"].numel(), _ptr(fx["Vc"]),
                                                fx["Vc"].numel(), _ptr(small), nr))
    _lib.check(lib.lrf_qmf_decode_scaled_rgb_u8(ctx._h, 8, _table(fx["uo"], fx["vo"], ro), scale, _ptr(far.src), BIG, _ptr(far.src), BIG, _ptr(far.out),
                                                BIG))
    for i, ((h, w), o, s) in enumerate(zip(dims, ro, rsz)):
        assert np.array_equal(far.out[int(o):int(o) + s].cpu().numpy().reshape(3, h, w), _level(far, variant, i, scale, oracle)), (i, int(o))
    _check_placed(far, far.out, ro, rsz, small, cr, "decode_scaled")


def _crop_call(fn, ctx, table, U, V, boxes, box_type, size, guard=4096):
    from lrf_amd import _lib
    n, (h, w) = boxes.shape[0], size
    out = torch.full((n * 3 * h * w + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.use_torch_stream()
    _lib.check(fn(ctx._h, 8, table, _ptr(U), U.numel(), _ptr(V), V.numel(), n, boxes.ctypes.data_as(ctypes.POINTER(box_type)), h, w, _ptr(out),
                  n * 3 * h * w))
    assert bool((out[n * 3 * h * w:] == 0xA5).all())
    return out[:n * 3 * h * w].view(n, 3, h, w)


@pytest.mark.parametrize("variant", [0, 1])
def test_decode_crops(far, oracle, variant):
    """far u_off / v_off; the output is the crops back to back (see the module's docstring)"""
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    fx = _factors(far, variant)
    h, w = 24, 48  # the smallest image: every image gives its first and its last window
    boxes = np.array([b for i, (H, W, _) in enumerate(EIGHT) for b in ((i, 0, 0), (i, H - h, W - w))], dtype=np.int32)
    near = _crop_call(lib.lrf_qmf_decode_crops_rgb_u8, ctx, _table(fx["cu"], fx["cv"], [0] * 8), fx["Uc"], fx["Vc"], boxes, _lib.Crop, (h, w))
    got = _crop_call(lib.lrf_qmf_decode_crops_rgb_u8, ctx, _table(fx["uo"], fx["vo"], [0] * 8), far.src, far.src, boxes, _lib.Crop, (h, w))
    assert torch.equal(got, near)
    got = got.cpu().numpy()
    for j, (i, y0, x0) in enumerate(boxes.tolist()):
        assert np.array_equal(got[j], _full(far, variant, oracle)[i][:, y0:y0 + h, x0:x0 + w]), (j, i)


@pytest.mark.parametrize("variant", [0, 1])
def test_decode_scaled_crops(far, oracle, variant):
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    fx = _factors(far, variant)
    h, w = 3, 6  # 24x48 at 1/8
    boxes = []
    for i, (H, W, _) in enumerate(EIGHT):
        for f in (2, 4, 8):
            hs, ws = _lib.scaled_dims(H, W, f)
            boxes.append((i, f, (hs - h) if (i + f) % 3 else 0, (ws - w) if (i + f) % 2 else 0))
    boxes = np.array(boxes, dtype=np.int32)
    fn = lib.lrf_qmf_decode_scaled_crops_rgb_u8
    near = _crop_call(fn, ctx, _table(fx["cu"], fx["cv"], [0] * 8), fx["Uc"], fx["Vc"], boxes, _lib.ScaledCrop, (h, w))
    got = _crop_call(fn, ctx, _table(fx["uo"], fx["vo"], [0] * 8), far.src, far.src, boxes, _lib.ScaledCrop, (h, w))
    assert torch.equal(got, near)
    got = got.cpu().numpy()
    for j, (i, f, y0, x0) in enumerate(boxes.tolist()):
        assert np.array_equal(got[j], _level(far, variant, i, f, oracle)[:, y0:y0 + h, x0:x0 + w]), (j, i, f)


@pytest.mark.parametrize("variant", [0, 1])
def test_decode_resized_crops(far, oracle, variant):
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    fx = _factors(far, variant)
    oh, ow = 10, 12  # the whole of 24x48 comes from level 2, of 173x264 from level 8; the small boxes from level 1
    boxes = []
    for i, (H, W, _) in enumerate(EIGHT):
        boxes += [(i, 0, 0, H, W, i & 1), (i, H - 13, W - 17, 13, 17, 1 - (i & 1)), (i, 1, 2, H - 1, W - 2, 0)]
    boxes = np.array(boxes, dtype=np.int32)
    fn = lib.lrf_qmf_decode_resized_crops_rgb_u8
    near = _crop_call(fn, ctx, _table(fx["cu"], fx["cv"], [0] * 8), fx["Uc"], fx["Vc"], boxes, _lib.ResizedCrop, (oh, ow))
    got = _crop_call(fn, ctx, _table(fx["uo"], fx["vo"], [0] * 8), far.src, far.src, boxes, _lib.ResizedCrop, (oh, ow))
    assert torch.equal(got, near)
    got = got.cpu().numpy()
    levels = set()
    for j, (i, y0, x0, hb, wb, flip) in enumerate(boxes.tolist()):
        f = resized_level(hb, wb, oh, ow)
        levels.add(f)
        assert np.array_equal(got[j], reference_resized(_level(far, variant, i, f, oracle), (y0, x0, hb, wb), (oh, ow), bool(flip))), (j, i, f)
    assert levels == {1, 2, 4, 8}


@pytest.mark.parametrize("variant", [0, 1])
def test_sse_ragged(far, oracle, variant):
    """the sources are the sentinel bytes of the first output buffer at far rgb_off: nothing is written there"""
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    fx = _factors(far, variant)
    _, _, rsz = _sizes()
    ro = fo.place(rsz, variant, 5)
    assert fo.covers(ro, rsz)
    cr, nr = fo.compact(ro, rsz)
    small = _gather(far.out, ro, rsz, cr, nr)
    near = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    got = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(lib.lrf_qmf_sse_ragged_rgb_u8(ctx._h, 8, _table(fx["cu"], fx["cv"], cr), _ptr(fx["Uc"]), fx["Uc"].numel(), _ptr(fx["Vc"]), fx["Vc"].numel(),
                                             _ptr(small), nr, _ptr(near)))
    _lib.check(lib.lrf_qmf_sse_ragged_rgb_u8(ctx._h, 8, _table(fx["uo"], fx["vo"], ro), _ptr(far.src), BIG, _ptr(far.src), BIG, _ptr(far.out), BIG,
                                             _ptr(got)))
    want = [int(((_full(far, variant, oracle)[i].astype(np.int64).reshape(-1) - far.out[int(o):int(o) + s].cpu().numpy().astype(np.int64)) ** 2).sum())
            for i, (o, s) in enumerate(zip(ro, rsz))]
    assert got.tolist() == near.tolist() == want
    assert fo.gaps_untouched(far.out, far.pat, [])


# (rows, cols): columns of one tile and of several, one column and 33, a stored-block length
MATS = [(300, 7), (4096, 3), (65, 33), (1000, 1), (2048, 16), (33, 5), (700, 9), (70000, 2)]


@pytest.mark.parametrize("variant", [0, 1])
def test_deflate_and_inflate_columns(far, variant):
    """lrf_deflate_columns_i8 with far src_off and dst_off, lrf_deflate_sizes_i8 with far src_off, then lrf_inflate_columns_i8 on
    the far streams (its src offsets) into far dst_off of the second buffer: the host restatement's bytes, zlib's round trip, and
    the matrices back."""
    from lrf_amd import _lib
    ctx = _lib.context(0)
    msz = [r * c for r, c in MATS]
    ssz = [c * int(_lib.deflate_bound(r)) for r, c in MATS]
    so, do = fo.place(msz, variant, 0), fo.place(ssz, variant, 3)
    assert fo.covers(so, msz) and fo.covers(do, ssz)
    cs, ns = fo.compact(so, msz)
    cd, nd = fo.compact(do, ssz)
    ncols = sum(c for _, c in MATS)
    len_off = np.cumsum([c for _, c in MATS]) - np.array([c for _, c in MATS])
    table = np.array([(s, r, c, d, lo) for s, (r, c), d, lo in zip(so, MATS, do, len_off)], dtype=np.int64)
    ctable = np.array([(s, r, c, d, lo) for s, (r, c), d, lo in zip(cs, MATS, cd, len_off)], dtype=np.int64)
    src_c = _gather(far.src, so, msz, cs, ns)
    slots_c = torch.full((nd,), 0xA5, dtype=torch.uint8, device="cuda")
    lens_c = torch.full((ncols,), -1, dtype=torch.int32, device="cuda")
    lens = torch.full((ncols,), -1, dtype=torch.int32, device="cuda")
    sizes = torch.full((ncols,), -1, dtype=torch.int32, device="cuda")
    ctx.deflate_columns_into(src_c, ctable, slots_c, lens_c)
    ctx.deflate_columns_into(far.src, table, far.out, lens)
    ctx.deflate_sizes_into(far.src, table, sizes)
    assert torch.equal(lens, lens_c) and torch.equal(sizes, lens_c)
    lens_h = lens.cpu().numpy()
    offs, coffs = _lib.deflate_column_offsets(table), _lib.deflate_column_offsets(ctable)
    k = 0
    for (rows, cols), s, o in zip(MATS, msz, so):  # the host restatement and zlib on every far column
        m = far.src[int(o):int(o) + s].cpu().numpy().reshape(rows, cols)
        for j in range(cols):
            col = np.ascontiguousarray(m[:, j])
            stream = far.out[int(offs[k]):int(offs[k]) + int(lens_h[k])].cpu().numpy().tobytes()
            assert stream == dc.host_stream(col), (rows, cols, j)
            assert zlib.decompress(stream) == col.tobytes()
            assert torch.equal(far.out[int(offs[k]):int(offs[k]) + int(lens_h[k])], slots_c[int(coffs[k]):int(coffs[k]) + int(lens_h[k])])
            k += 1
    # inflate: the streams where deflate left them (far col_off), the matrices to other far places of the second buffer
    io = fo.place(msz, variant, 6)
    assert fo.covers(io, msz)
    itable = np.array([(d, r, c, f) for d, (r, c), f in zip(io, MATS, len_off)], dtype=np.int64)
    status = torch.full((ncols,), -1, dtype=torch.int32, device="cuda")
    ctx.inflate_columns_into(far.out, itable, offs, lens_h, far.aux.view(torch.int8), status)
    assert status.tolist() == [0] * ncols
    _check_placed(far, far.aux, io, msz, src_c, cs, "inflate_columns")
    # deflate wrote the streams and nothing past a slot's stream but inside its slot: outside the slots the pattern stands
    ranges = [(int(o), int(o) + s) for o, s in zip(do, ssz)]
    ok = fo.gaps_untouched(far.out, far.pat, ranges)
    fo.restore(far.out, far.pat, ranges)
    assert ok, "deflate_columns wrote outside its slots"


@pytest.mark.parametrize("hw", [(1365, 2048), (1024, 2048)])
def test_uniform_decode_past_p32(far, oracle, hw):
    """lrf_qmf_decode_rgb_u8 on B = ceil(P32 / (3 H W)) + 2 images, written into the first far buffer: 1365x2048 is the strip body
    (image 256 straddles P31, image 512 P32), 1024x2048 the 16-aligned tile.  Eight random factor sets, U over the full int8
    range, repeated cyclically: every image equals its set decoded alone, and the images at the edges equal the oracle's."""
    from lrf_amd import _lib
    from lrf_amd.codec import split_factors
    ctx, lib = _lib.context(0), _lib.load()
    H, W = hw
    ranks = (7, 3, 3)
    px = 3 * H * W
    B = -(-P32 // px) + 2
    assert B * px > P32 and B * px <= BIG and B % 8 != 0
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    g = torch.Generator(device="cuda").manual_seed(H)
    U8 = torch.randint(-128, 128, (8, nu), dtype=torch.int8, device="cuda", generator=g)
    V8 = torch.randint(-16, 16, (8, nv), dtype=torch.int8, device="cuda", generator=g)
    alone = ctx.decode_rgb(U8, V8, H, W, list(ranks)).reshape(8, px)
    U = U8.repeat(-(-B // 8), 1)[:B].contiguous()
    V = V8.repeat(-(-B // 8), 1)[:B].contiguous()
    R = (ctypes.c_int * 3)(*ranks)
    ctx.use_torch_stream()
    _lib.check(lib.lrf_qmf_decode_rgb_u8(ctx._h, _ptr(U), _ptr(V), B, H, W, R, _ptr(far.out)))
    imgs = far.out[:B * px].view(B, px)
    want64 = alone.repeat(8, 1)
    for b0 in range(0, B, 64):
        n = min(64, B - b0)
        assert torch.equal(imgs[b0:b0 + n], want64[:n]), b0
    del want64
    edge = sorted({0, P31 // px - 1, P31 // px, P31 // px + 1, P32 // px - 1, P32 // px, B - 1})
    assert P31 // px * px < P31 < (P31 // px + 1) * px and P32 // px * px < P32 < (P32 // px + 1) * px  # those two straddle
    if hw == (1365, 2048):
        assert edge == [0, 255, 256, 257, 511, 512, B - 1]
    f8 = [split_factors(U8[s].cpu().numpy(), V8[s].cpu().numpy(), (H, W), ranks) for s in range(8)]
    want8 = {}
    for b in edge:
        s = b % 8
        if s not in want8:
            want8[s] = oracle.planes_to_rgb(f8[s][0::2], f8[s][1::2], H, W)
        assert np.array_equal(imgs[b].cpu().numpy().reshape(3, H, W), want8[s]), b
    ranges = [(0, B * px)]
    ok = fo.gaps_untouched(far.out, far.pat, ranges)
    fo.restore(far.out, far.pat, ranges)
    assert ok, "the decoder wrote past its batch"


# the images of the ragged encodes: EIGHT with the rank above 32 (which those entry points refuse) replaced
ENC8 = EIGHT[:7] + [(24, 48, (26, 13, 13))]
ENC_K = 4


def _enc_sizes():
    from lrf_amd import _lib
    usz = [sum(d[4] * r for d, r in zip(_lib.plane_dims(H, W), ranks)) for H, W, ranks in ENC8]
    return usz, [64 * sum(ranks) for _, _, ranks in ENC8], [3 * H * W for H, W, _ in ENC8]


def _oracle_factors(oracle, img, ranks):
    X = oracle.rgb_to_planes(img)
    out = []
    for c in range(3):
        u, v = oracle.qmf_decompose(X[c], ranks[c], ENC_K, (-16, 15))
        out += [u.astype(np.int8), v.astype(np.int8)]
    return out


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("sweep", [False, True])
def test_encode_ragged(far, oracle, variant, sweep):
    """lrf_qmf_encode_ragged_rgb_u8 and lrf_qmf_encode_ragged_sweep_rgb_u8 (one candidate per image, the candidates in another
    order than the images): the pixels are bytes of the random buffer at far rgb_off, U goes to far u_off of the first pattern
    buffer and V to far v_off of the second.  Far equals compact, every image's factors equal the oracle's, and both output
    buffers keep their pattern between the factors."""
    from lrf_amd import _lib
    from lrf_amd.codec import split_factors
    ctx, lib = _lib.context(0), _lib.load()
    usz, vsz, rsz = _enc_sizes()
    ro, uo, vo = fo.place(rsz, variant, 5), fo.place(usz, variant, 0), fo.place(vsz, variant, 3)
    assert fo.covers(ro, rsz) and fo.covers(uo, usz) and fo.covers(vo, vsz)
    cr, nr = fo.compact(ro, rsz)
    cu, nu = fo.compact(uo, usz)
    cv, nv = fo.compact(vo, vsz)
    rgb_far = far.src.view(torch.uint8)
    rgb_c = _gather(rgb_far, ro, rsz, cr, nr)
    Uc = torch.full((nu,), 99, dtype=torch.int8, device="cuda")
    Vc = torch.full((nv,), 99, dtype=torch.int8, device="cuda")
    order = [5, 2, 7, 0, 3, 6, 1, 4]  # candidate k belongs to image order[k]

    def call(rgb, rgb_len, r_off, U, u_len, u_off, V, v_len, v_off):
        ctx.use_torch_stream()
        if not sweep:
            desc = (_lib.RaggedEncodeImage * 8)()
            for d, (H, W, ranks), r, u, v in zip(desc, ENC8, r_off, u_off, v_off):
                d.H, d.W, d.rgb_off, d.u_off, d.v_off, d.sign_off = H, W, int(r), int(u), int(v), -1
                d.R[0], d.R[1], d.R[2] = ranks
            _lib.check(lib.lrf_qmf_encode_ragged_rgb_u8(ctx._h, 8, desc, _ptr(rgb), rgb_len, ENC_K, -16, 15, None, 0, _ptr(U), u_len, _ptr(V), v_len))
            return
        idesc, cdesc = (_lib.RaggedSweepImage * 8)(), (_lib.RaggedSweepCandidate * 8)()
        for d, (H, W, _), r in zip(idesc, ENC8, r_off):
            d.H, d.W, d.rgb_off, d.sign_off = H, W, int(r), -1
        for d, i in zip(cdesc, order):
            d.image, d.u_off, d.v_off = i, int(u_off[i]), int(v_off[i])
            d.R[0], d.R[1], d.R[2] = ENC8[i][2]
        _lib.check(lib.lrf_qmf_encode_ragged_sweep_rgb_u8(ctx._h, 8, idesc, 8, cdesc, _ptr(rgb), rgb_len, ENC_K, -16, 15, None, 0, _ptr(U), u_len, _ptr(V),
                                                          v_len))

    call(rgb_c, nr, cr, Uc, nu, cu, Vc, nv, cv)
    call(rgb_far, BIG, ro, far.out.view(torch.int8), BIG, uo, far.aux.view(torch.int8), BIG, vo)
    for i, (H, W, ranks) in enumerate(ENC8):  # the oracle on every far item
        img = rgb_far[int(ro[i]):int(ro[i]) + rsz[i]].cpu().numpy().reshape(3, H, W)
        got = split_factors(far.out.view(torch.int8)[int(uo[i]):int(uo[i]) + usz[i]].cpu().numpy(),
                            far.aux.view(torch.int8)[int(vo[i]):int(vo[i]) + vsz[i]].cpu().numpy(), (H, W), ranks)
        for a, b in zip(got, _oracle_factors(oracle, img, ranks)):
            assert np.array_equal(a, b), (i, H, W, ranks)
    _check_placed(far, far.out, uo, usz, Uc, cu, "encode_ragged U")
    _check_placed(far, far.aux, vo, vsz, Vc, cv, "encode_ragged V")


def _cyclic(far, B, px, base):
    """the first B * px bytes of the first pattern buffer := base's eight rows repeated -> the view [B, px]"""
    imgs = far.out[:B * px].view(B, px)
    n8 = B // 8 * 8
    imgs[:n8].view(B // 8, 8, px).copy_(base[None].expand(B // 8, 8, px))
    imgs[n8:].copy_(base[:B - n8])
    return imgs


def _sse_by_torch(a, b):
    """int64 [B]: the squared error of the rows of two uint8 tensors [B, n], 16 rows at a time"""
    out = []
    for k in range(0, a.shape[0], 16):
        d = a[k:k + 16].to(torch.int16) - b[k:k + 16].to(torch.int16)
        out.append((d.to(torch.int32) ** 2).sum(dim=1, dtype=torch.int64))
    return torch.cat(out)


def test_uniform_metrics_past_p32(far):
    """lrf_image_metrics_u8 (the squared error alone, and with the SSIM) on B = ceil(P32 / (3 H W)) + 2 images of 1365x2048, both
    operands past P32: the squared errors are the integers torch sums, and the SSIM of an image has the bits of the single-image
    call wherever it stands.  Not the cyclic construction: the operands are the sentinel pattern and the random buffer, so no two
    images are equal and every image's error has a reference of its own; the SSIM is compared on the edge images and every 37th
    (about twenty single-image calls), not on all."""
    from lrf_amd import _lib
    ctx = _lib.context(0)
    H, W = 1365, 2048
    px = 3 * H * W
    B = -(-P32 // px) + 2
    a = far.out[:B * px].view(B, 3, H, W)                  # the pattern: a period of 2^24 bytes, so no two images are equal
    b = far.src.view(torch.uint8)[:B * px].view(B, 3, H, W)
    want = _sse_by_torch(a.view(B, px), b.view(B, px))
    assert torch.equal(ctx.image_metrics(a, b, want_ssim=False)[0], want)
    sse, ssim = ctx.image_metrics(a, b)
    assert torch.equal(sse, want)
    for i in sorted({0, 255, 256, 257, 511, 512, B - 1} | set(range(3, B, 37))):
        s1, q1 = ctx.image_metrics(a[i:i + 1], b[i:i + 1])
        assert int(s1[0]) == int(want[i]) and torch.equal(q1.view(torch.int64), ssim[i:i + 1].view(torch.int64)), i
    assert fo.gaps_untouched(far.out, far.pat, [])


def test_uniform_sweep_sse_past_p32(far):
    """lrf_qmf_sweep_sse_rgb_u8 on the same batch with seven triples whose factors, triple after triple, are the first
    B * sum(u_img) bytes of the random buffer: the U of the third triple straddles P31, the last triple's straddles P32.  The
    errors equal those of one call per triple with the pointers advanced, and the last triple's equal torch's sums over the
    images the uniform decoder writes (into the second pattern buffer).  Only that last triple has a reference outside this entry
    point; the others check the triple's base offset against the same kernels at base 0."""
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    H, W = 1365, 2048
    px = 3 * H * W
    B = -(-P32 // px) + 2
    rgb = far.out[:B * px].view(B, 3, H, W)
    triples = [(32, 16, 16)] * 4 + [(16, 8, 8), (7, 3, 3), (3, 1, 1)]
    dims = _lib.plane_dims(H, W)
    nus = [sum(d[4] * r for d, r in zip(dims, t)) for t in triples]
    nvs = [64 * sum(t) for t in triples]
    u0 = np.cumsum([0] + [B * n for n in nus])
    v0 = np.cumsum([0] + [B * n for n in nvs])
    assert u0[2] < P31 < u0[3] and u0[6] < P32 < u0[7] <= BIG
    V = far.src[P31:P31 + int(v0[7])]
    factors = [(far.src[int(u0[q]):int(u0[q + 1])].view(B, nus[q]), V[int(v0[q]):int(v0[q + 1])].view(B, nvs[q])) for q in range(7)]
    got = ctx.sweep_sse(rgb, factors, triples)
    assert _lib.flat_views([f[0] for f in factors]).data_ptr() == far.src.data_ptr()  # (views of the far buffer, no copy)
    for q in range(7):
        assert torch.equal(ctx.sweep_sse(rgb, [factors[q]], [triples[q]])[0], got[q]), q
    R = (ctypes.c_int * 3)(*triples[6])
    ctx.use_torch_stream()
    _lib.check(lib.lrf_qmf_decode_rgb_u8(ctx._h, _ptr(factors[6][0]), _ptr(factors[6][1]), B, H, W, R, _ptr(far.aux)))
    want = _sse_by_torch(rgb.view(B, px), far.aux[:B * px].view(B, px))
    fo.restore(far.aux, far.pat, [(0, B * px)])
    assert torch.equal(got[6], want)
    assert fo.gaps_untouched(far.out, far.pat, [])


def test_uniform_decode_factors_past_p31(far, oracle):
    """lrf_qmf_decode_rgb_u8 with a U batch past 2^31 bytes: 30,600 images of 173x264 at ranks (64, 64, 64) — the any-size body, the
    one whose factors are large next to its pixels — read their U from the first 30,600 x 70,400 bytes of the random buffer (image
    30,504 straddles P31) and write 4.19 GB.  The images of five chunks of up to 1,000 — the first, the one across P31 (the last) among them —
    equal the same call on the chunk alone (no product in it passes 2^31), and the images at the edges equal the oracle's."""
    from lrf_amd import _lib
    from lrf_amd.codec import split_factors
    ctx, lib = _lib.context(0), _lib.load()
    H, W, ranks, B = 173, 264, (64, 64, 64), 30600
    px = 3 * H * W
    dims = _lib.plane_dims(H, W)
    nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
    assert nu == 70400 and B * nu > P31 and P31 // nu == 30504 and P31 % nu and P31 < B * px <= BIG
    U = far.src[:B * nu].view(B, nu)
    V = far.src[P31 + 2 ** 30:P31 + 2 ** 30 + B * nv].view(B, nv)
    R = (ctypes.c_int * 3)(*ranks)
    ctx.use_torch_stream()
    _lib.check(lib.lrf_qmf_decode_rgb_u8(ctx._h, _ptr(U), _ptr(V), B, H, W, R, _ptr(far.out)))
    imgs = far.out[:B * px].view(B, px)
    for k in (0, 9000, 19000, 29000, 30000):
        n = min(1000, B - k)
        assert torch.equal(imgs[k:k + n], ctx.decode_rgb(U[k:k + n], V[k:k + n], H, W, list(ranks)).view(n, px)), k
    for b in (0, 30503, 30504, 30505, B - 1):
        f = split_factors(U[b].cpu().numpy(), V[b].cpu().numpy(), (H, W), ranks)
        assert np.array_equal(imgs[b].cpu().numpy().reshape(3, H, W), oracle.planes_to_rgb(f[0::2], f[1::2], H, W)), b
    ok = fo.gaps_untouched(far.out, far.pat, [(0, B * px)])
    fo.restore(far.out, far.pat, [(0, B * px)])
    assert ok, "the decoder wrote past its batch"


def test_uniform_encode_past_p32(far, oracle):
    """lrf_qmf_encode_rgb_u8 on B = ceil(P32 / (3 H W)) + 2 = 515 images of 1365x2048: the input passes P32 (and the X workspace 2^31
    floats).  Eight random images repeated cyclically: every image's factors equal its twin's of the eight encoded alone, and
    the images 0, 256, 512 and B - 1 equal the oracle's at ranks (7, 3, 3), computed on host threads."""
    import lrf_amd
    from concurrent.futures import ThreadPoolExecutor
    from lrf_amd.codec import split_factors
    H, W, ranks = 1365, 2048, [7, 3, 3]
    px = 3 * H * W
    B = -(-P32 // px) + 2
    g = torch.Generator(device="cuda").manual_seed(45)
    base = torch.randint(0, 256, (8, px), dtype=torch.uint8, device="cuda", generator=g)
    imgs = _cyclic(far, B, px, base).view(B, 3, H, W)
    try:
        U8, V8 = lrf_amd.qmf_factorize_batch(base.view(8, 3, H, W), ranks)
        U, V = lrf_amd.qmf_factorize_batch(imgs, ranks)
        for k in range(0, B, 8):
            n = min(8, B - k)
            assert torch.equal(U[k:k + n], U8[:n]) and torch.equal(V[k:k + n], V8[:n]), k
        sample = [0, 256, 512, B - 1]
        sets = sorted({b % 8 for b in sample})
        host = {s: base[s].cpu().numpy().reshape(3, H, W) for s in sets}

        def one(s):
            X = oracle.rgb_to_planes(host[s])
            out = []
            for c in range(3):
                u, v = oracle.qmf_decompose(X[c], ranks[c], 10, (-16, 15))
                out += [u.astype(np.int8), v.astype(np.int8)]
            return out
        with ThreadPoolExecutor(max_workers=4) as pool:
            want = dict(zip(sets, pool.map(one, sets)))
        for b in sample:
            got = split_factors(U[b].cpu().numpy(), V[b].cpu().numpy(), (H, W), ranks)
            assert all(np.array_equal(x, y) for x, y in zip(got, want[b % 8])), b
        lrf_amd._lib.context(0).check()
    finally:
        fo.restore(far.out, far.pat, [(0, B * px)])
        lrf_amd._lib.context(0).trim()  # the 8.6 GB of patch matrices


def test_any_shape_decode_past_p32(far, oracle):
    """lrf_qmf_decode_any_hw_u8 with 4x4 patches on B = ceil(P32 / (3 H W)) + 2 images of 498x514 (both planes padded), written into
    the first pattern buffer; the six factor batches are slices of the random buffer, two of them across P31 and P32.  The images
    0, middle, last and those across P31 and P32 equal the oracle's, and three chunks of 500 images equal the same call on the
    chunk alone."""
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    H, W, patch, ranks = 498, 514, (4, 4), (5, 3, 2)
    px = 3 * H * W
    B = -(-P32 // px) + 2
    assert P32 < B * px <= BIG
    dims = _lib.plane_dims_any(H, W, patch, None)
    starts = [(0, 2 ** 30), (P31 - 1000, 3 * 2 ** 29), (P32 - 12345, 5 * 2 ** 28)]  # where (U_c, V_c) start in the random buffer
    Us, Vs = [], []
    for d, r, (us, vs) in zip(dims, ranks, starts):
        M, N = d[4], d[5]
        assert N == 16 and us + B * M * r <= BIG and vs + B * N * r <= BIG
        Us.append(far.src[us:us + B * M * r].view(B, M, r))
        Vs.append(far.src[vs:vs + B * N * r].view(B, N, r))
    assert starts[1][0] < P31 < starts[1][0] + Us[1].numel() and starts[2][0] < P32 < starts[2][0] + Us[2].numel()
    R = (ctypes.c_int * 3)(*ranks)
    ctx.use_torch_stream()
    _lib.check(lib.lrf_qmf_decode_any_hw_u8(ctx._h, _ptr(Us[0]), _ptr(Vs[0]), _ptr(Us[1]), _ptr(Vs[1]), _ptr(Us[2]), _ptr(Vs[2]), B, H, W, 0, 0, 4, 4, R,
                                            _ptr(far.out)))
    imgs = far.out[:B * px].view(B, 3, H, W)
    for b in sorted({0, B // 2, B - 1, P31 // px, P32 // px}):
        f = [(Us[c][b].cpu().numpy(), Vs[c][b].cpu().numpy()) for c in range(3)]
        assert np.array_equal(imgs[b].cpu().numpy(), oracle.qmf_anyshape_decode(f, H, W, patch)), b
    for k in (0, P31 // px - 250, B - 500):
        assert torch.equal(imgs[k:k + 500], ctx.decode_any([u[k:k + 500] for u in Us], [v[k:k + 500] for v in Vs], H, W, patch)), k
    ok = fo.gaps_untouched(far.out, far.pat, [(0, B * px)])
    fo.restore(far.out, far.pat, [(0, B * px)])
    assert ok, "the decoder wrote past its batch"
