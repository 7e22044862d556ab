"""GPU suite (-m gpu): the squared error of a list of items that differ in size and ranks straight from their factors
(Context.sse_ragged, lrf_qmf_sse_ragged_rgb_u8) against Context.decode_ragged on the same descriptors followed by the sum of
squared differences in int64.  Random int8 factors in [-16, 15] and random uint8 sources: no encoder is involved.  Everything is
compared as integers."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
TILE16, STRIP, R8, ANY = range(4)

# 64x64: the 16-aligned body in all five classes; 40x64 (12 chroma patches): the strip body in all five; 33x47: the rank <= 8
# kernel and the general kernel; 96x96: beyond the tiled rank bounds; 16x16: one tile, one chroma patch
ITEMS = ([(64, 64, t) for t in ((8, 4, 4), (8, 8, 8), (16, 8, 8), (16, 16, 16), (32, 16, 16))]
         + [(40, 64, t) for t in ((8, 4, 4), (8, 8, 8), (16, 8, 8), (16, 12, 12), (32, 12, 12))]
         + [(33, 47, (8, 6, 6)), (33, 47, (20, 6, 6)), (96, 96, (40, 20, 20)), (96, 96, (64, 36, 36)), (16, 16, (4, 1, 1))])


def classify(H, W, ranks):
    """(kind, cls) of an item: the rule of decode_plan's comment (lrf_amd/csrc/lrf_plan.cpp), restated as in
    tests/test_decode_ragged_plan.py, which compares its restatement with the library's function on the CPU.  The scorer only loads its source, so a 16-aligned item keeps the 16-aligned body wherever
    the source starts.  Planes: luma H x W, chroma floor(H/2) x floor(W/2), reflect-padded to multiples of 8 with the smaller
    half of the padding on the left / top."""
    w = [W, W // 2]
    wp = [-(-x // 8) * 8 for x in w]
    left = [(p - x) // 2 for p, x in zip(wp, w)]
    rcm = max(ranks[1], ranks[2])
    tiled_ranks = ranks[0] <= 32 and rcm <= 16
    sides16 = H % 16 == 0 and W % 16 == 0
    strip_ok = W % 2 == 0 and left[0] % 2 == 0 and (left[1] - left[0] // 2) % 4 == 0
    if tiled_ranks and (sides16 or strip_ok):
        rl = 8 if ranks[0] <= 8 else (16 if ranks[0] <= 16 else 32)
        rc = 4 if rcm <= 4 else (8 if rcm <= 8 else 16)
        cls = {(8, 4): 0, (8, 8): 1, (16, 4): 2, (16, 8): 2, (8, 16): 3, (16, 16): 3}.get((rl, rc), 4)
        return (TILE16 if sides16 else STRIP), cls
    return (R8 if max(ranks) <= 8 else ANY), 0


def test_the_list_covers_every_kernel_and_every_class():
    kinds = [classify(*it) for it in ITEMS]
    assert {k for k, _ in kinds} == {TILE16, STRIP, R8, ANY}
    assert {c for k, c in kinds if k == TILE16} == set(range(5)) and {c for k, c in kinds if k == STRIP} == set(range(5))
    assert classify(33, 47, (8, 6, 6))[0] == R8 and classify(33, 47, (20, 6, 6))[0] == ANY
    assert classify(96, 96, (40, 20, 20))[0] == ANY and classify(96, 96, (64, 36, 36))[0] == ANY and classify(16, 16, (4, 1, 1)) == (TILE16, 0)


class Made:
    """factors, sources, the decoded images and the expected values: made once, left unchanged"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from lrf_amd import _lib
            ctx = _lib.context(0)
            g = torch.Generator().manual_seed(11)
            u_off, v_off, uo, vo = [], [], 3, 5  # (factors at odd offsets, gaps between the items)
            for H, W, t in ITEMS:
                u_off.append(uo)
                v_off.append(vo)
                uo += sum(d[4] * r for d, r in zip(_lib.plane_dims(H, W), t)) + 7
                vo += 64 * sum(t) + 3
            U = torch.randint(-16, 16, (uo,), dtype=torch.int8, generator=g).cuda()
            V = torch.randint(-16, 16, (vo,), dtype=torch.int8, generator=g).cuda()
            # one source per distinct size: the items of a size share it; sources at odd byte offsets
            src_off, so = {}, 1
            for H, W, _ in ITEMS:
                if (H, W) not in src_off:
                    src_off[(H, W)] = so
                    so += 3 * H * W + 1
            rgb = torch.randint(0, 256, (so,), dtype=torch.uint8, generator=g).cuda()
            dec = ctx.decode_ragged(U, V, [(H, W, t, a, b) for (H, W, t), a, b in zip(ITEMS, u_off, v_off)])
            want = []
            for (H, W, _), a in zip(ITEMS, dec):
                s = rgb[src_off[(H, W)]:src_off[(H, W)] + 3 * H * W].view(3, H, W)
                want.append(int(((a.long() - s.long()) ** 2).sum()))
            items = [(H, W, t, a, b, src_off[(H, W)]) for (H, W, t), a, b in zip(ITEMS, u_off, v_off)]
            cls._made = (ctx, U, V, rgb, items, dec, want)
        return cls._made


def test_every_item_equals_decode_then_squared_error():
    ctx, U, V, rgb, items, dec, want = Made.get()
    got = ctx.sse_ragged(rgb, items, U, V)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (len(items),)
    assert got.tolist() == want
    assert min(want) > 0 and len({it[5] for it in items}) < len(items)  # sources are shared, and nothing is trivially zero


def test_order_and_neighbours_do_not_matter():
    ctx, U, V, rgb, items, dec, want = Made.get()
    perm = torch.randperm(len(items), generator=torch.Generator().manual_seed(3)).tolist()
    assert perm != sorted(perm)
    got = ctx.sse_ragged(rgb, [items[i] for i in perm], U, V).tolist()
    assert got == [want[i] for i in perm]
    for i in (0, 7, 10, 11, 13, 14):  # one item alone, of every kind
        assert ctx.sse_ragged(rgb, [items[i]], U, V).tolist() == [want[i]]
    twice = ctx.sse_ragged(rgb, items + items[::-1], U, V).tolist()  # the same items (and sources) twice in one call
    assert twice == want + want[::-1]


def test_an_item_scored_against_its_own_decode_is_zero():
    ctx, U, V, rgb, items, dec, want = Made.get()
    offs, parts, at = [], [], rgb.numel()
    for a in dec:
        offs.append(at)
        parts.append(a.reshape(-1))
        at += a.numel()
    both = torch.cat([rgb] + parts)
    mixed = [it[:5] + (o,) for it, o in zip(items, offs)] + items
    got = ctx.sse_ragged(both, mixed, U, V).tolist()
    assert got == [0] * len(items) + want


def _entry(ctx, lib, n, descs, U, V, rgb, sse, u_len=None, v_len=None, rgb_len=None):
    from lrf_amd import _lib
    desc = (_lib.RaggedImage * max(1, len(descs or [])))()
    for d, (H, W, t, uo, vo, ro) in zip(desc, descs or []):
        d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, uo, vo, ro
        d.R[0], d.R[1], d.R[2] = t
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ctx.use_torch_stream()
    return lib.lrf_qmf_sse_ragged_rgb_u8(ctx._h, n, desc if descs is not None else None, ptr(U), U.numel() if u_len is None else u_len, ptr(V),
                                         V.numel() if v_len is None else v_len, ptr(rgb), rgb.numel() if rgb_len is None else rgb_len, ptr(sse))


def test_a_garbage_output_buffer_does_not_change_the_result():
    from lrf_amd import _lib
    ctx, U, V, rgb, items, dec, want = Made.get()
    sse = torch.full((len(items) + 2,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    assert _entry(ctx, _lib.load(), len(items), items, U, V, rgb, sse[1:]) == 0
    out = sse.tolist()
    assert out[1:-1] == want and out[0] == out[-1] == -0x0123456789ABCDEF  # the call zeroes its n entries, no more


def test_c_entry_refuses_on_the_host_and_launches_nothing():
    from lrf_amd import _lib
    ctx, U, V, rgb, items, dec, want = Made.get()
    lib = _lib.load()
    sse = torch.full((len(items),), 0x5A5A, dtype=torch.int64, device="cuda")
    ok = items[:3]
    last = lambda **kw: ok[:2] + [tuple(kw.get(k, x) for k, x in zip(("H", "W", "R", "u", "v", "rgb"), ok[2]))]
    call = lambda n, d, **kw: _entry(ctx, lib, n, d, kw.pop("U", U), kw.pop("V", V), kw.pop("rgb", rgb), kw.pop("sse", sse), **kw)
    H, W, t = ok[2][:3]
    nu, nv = sum(d[4] * r for d, r in zip(_lib.plane_dims(H, W), t)), 64 * sum(t)
    einval = {
        "u range": call(3, last(u=U.numel() - nu + 1)),
        "v range": call(3, last(v=V.numel() - nv + 1)),
        "source range": call(3, last(rgb=rgb.numel() - 3 * H * W + 1)),
        "u_len short": call(3, ok, u_len=ok[2][3] + nu - 1),
        "v_len short": call(3, ok, v_len=ok[2][4] + nv - 1),
        "rgb_len short": call(3, ok, rgb_len=ok[2][5] + 3 * H * W - 1),
        "negative u": call(3, last(u=-1)),
        "negative v": call(3, last(v=-1)),
        "negative source": call(3, last(rgb=-1)),
        "offset near 2^63": call(3, last(u=2 ** 63 - 1)),
        "rank 0": call(3, last(R=(8, 0, 8))),
        "rank 65": call(3, last(R=(65, 8, 8))),
        "no size": call(3, last(H=0)),
        "1x1": call(3, last(H=1, W=1)),
        "n = 0": call(0, ok),
        "n = 65536": call(65536, ok),
        "NULL items": call(3, None),
        "NULL U": _entry(ctx, lib, 3, ok, None, V, rgb, sse, u_len=U.numel()),
        "NULL V": _entry(ctx, lib, 3, ok, U, None, rgb, sse, v_len=V.numel()),
        "NULL rgb": _entry(ctx, lib, 3, ok, U, V, None, sse, rgb_len=rgb.numel()),
        "NULL sse": call(3, ok, sse=None),
    }
    assert all(rc == -1 for rc in einval.values()), einval
    torch.cuda.synchronize()
    assert bool((sse == 0x5A5A).all()), "a refused call wrote to its output"
    assert call(3, ok) == 0 and sse[:3].tolist() == want[:3] and bool((sse[3:] == 0x5A5A).all())
    for bad in ([it[:5] for it in ok], [ok[0][:5] + (rgb.numel(),)], []):
        with pytest.raises(ValueError):
            ctx.sse_ragged(rgb, bad, U, V)
    with pytest.raises(TypeError):
        ctx.sse_ragged(rgb.float(), ok, U, V)
    with pytest.raises(TypeError):
        ctx.sse_ragged(rgb, ok, U.float(), V)
