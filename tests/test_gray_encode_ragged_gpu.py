"""Gray image lists on the encode side (-m gpu): lrf_qmf_encode_gray_ragged_u8, lrf_qmf_encode_gray_ragged_sweep_u8 and
lrf_qmf_sse_gray_ragged_u8 (Context.encode_gray_ragged, encode_gray_ragged_sweep, sse_gray_ragged).  The factors bit for bit against
the oracle's 64-column path and against lrf_qmf_encode_gray_u8 at B = 1, whatever else the list holds and in whatever order; a
sweep candidate against the ragged encode of (image, R) alone; the squared error against its numpy definition and against
decode-then-lrf_image_metrics_u8; refusals that leave the outputs untouched; one call of each entry on a caller's side stream."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from scaled_decode import int_plane
from test_channels_gpu import smooth

pytestmark = pytest.mark.gpu

# M = 1, 6, 35, 96, 385 (past one 384-row block), 726, 300; W % 16 == 0 (the 16-byte planes body) at 64x96 and 48x400
SIZES = [(8, 8), (16, 24), (37, 53), (64, 96), (56, 440), (173, 264), (48, 400)]
RANKS = [1, 4, 7, 8, 9, 16, 17, 32]  # every rank family of the 64-column kernels
CONFIGS = [((-16, 15), 1), ((-16, 15), 10), ((-128, 127), 1), ((-128, 127), 10)]
SWEEP_RANKS = [1, 3, 8, 9, 20, 32]


def _ctx():
    from lrf_amd import _lib
    return _lib.context(0)


def patches(H, W):
    return ((H + (-H) % 8) // 8) * ((W + (-W) % 8) // 8)


@functools.lru_cache(maxsize=None)
def images():
    """one randint and one smooth image per size, uint8 [H, W]; read-only: every test shares them"""
    out = []
    for H, W in SIZES:
        rng = np.random.default_rng(H * 1000 + W)
        for im in (rng.integers(0, 256, (H, W), dtype=np.uint8), smooth(rng, 1, H, W)[0]):
            im.setflags(write=False)
            out.append(im)
    return tuple(out)


def pack(ims, base=0):
    """the images back to back, each at a multiple of 16 bytes from the buffer's start, the buffer sliced `base` bytes past
    a 16-byte aligned address -> (flat uint8 CUDA tensor, offsets)"""
    offs, off = [], 0
    for im in ims:
        offs.append(off)
        off += (im.size + 15) // 16 * 16
    buf = torch.zeros(off + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    flat = buf[base:base + off]
    for im, o in zip(ims, offs):
        flat[o:o + im.size].copy_(torch.from_numpy(im.reshape(-1).copy()))
    return flat, offs


def signs_of(i, R):
    """image i's column signs [R] (the leading R of one fixed draw of 32), or None: every third image keeps the default signs"""
    if i % 3 == 2:
        return None
    return np.random.default_rng(77 + i).choice(np.array([-1, 1], dtype=np.int8), size=32)[:R]


def sign_buffer(per_image):
    """[signs or None] -> (flat int8 CUDA tensor or None, sign_off per image with -1 for None)"""
    offs, parts, off = [], [], 3  # (a sign buffer that does not start at its first image)
    for s in per_image:
        offs.append(-1 if s is None else off)
        if s is not None:
            parts.append(s)
            off += len(s)
    if not parts:
        return None, offs
    return torch.from_numpy(np.concatenate([np.zeros(3, np.int8)] + parts)).cuda(), offs


def ranks_of(cfg):
    return [RANKS[(i + 3 * cfg) % len(RANKS)] for i in range(len(images()))]


def split(U, V, u_off, v_off, dims):
    """(flat U, flat V, offsets, [(M, R)]) -> [(u [M, R], v [64, R]) numpy]"""
    U, V = U.cpu().numpy(), V.cpu().numpy()
    return [(U[uo:uo + M * R].reshape(M, R), V[vo:vo + 64 * R].reshape(64, R)) for uo, vo, (M, R) in zip(u_off, v_off, dims)]


def encode_list(ctx, ims, ranks, signs, bounds, K, base=0):
    """Context.encode_gray_ragged of the list -> [(u, v) numpy] per image"""
    flat, offs = pack(ims, base)
    sg, soffs = sign_buffer(signs)
    out = ctx.encode_gray_ragged(flat, [(im.shape[0], im.shape[1], R, o, so) for im, R, o, so in zip(ims, ranks, offs, soffs)], K, bounds[0], bounds[1], sg)
    return split(*out, [(patches(*im.shape), R) for im, R in zip(ims, ranks)])


@functools.lru_cache(maxsize=None)
def encoded(cfg):
    """the ragged encode of the whole list under CONFIGS[cfg], computed once"""
    bounds, K = CONFIGS[cfg]
    ranks = ranks_of(cfg)
    return encode_list(_ctx(), images(), ranks, [signs_of(i, R) for i, R in enumerate(ranks)], bounds, K)


def same(a, b, what):
    assert len(a) == len(b)
    for i, ((ua, va), (ub, vb)) in enumerate(zip(a, b)):
        assert ua.shape == ub.shape and va.shape == vb.shape, (what, i)
        assert np.array_equal(ua, ub) and np.array_equal(va, vb), (what, i)


@pytest.mark.parametrize("cfg", range(len(CONFIGS)), ids=[f"{b}-K{k}" for b, k in CONFIGS])
def test_ragged_equals_oracle_and_encode_gray_at_batch_one(cfg, oracle):
    """every image of one list: oracle.qmf_decompose(oracle.pad_patchify(img), R, K, bounds, sign) and ctx.encode_gray(img[None]) bit for bit"""
    ctx = _ctx()
    bounds, K = CONFIGS[cfg]
    ranks = ranks_of(cfg)
    got = encoded(cfg)
    for i, (im, R) in enumerate(zip(images(), ranks)):
        sg = signs_of(i, R)
        u, v = oracle.qmf_decompose(oracle.pad_patchify(im[None].astype(np.float32)), R, K, bounds, sg)
        assert np.array_equal(got[i][0], u.astype(np.int8)) and np.array_equal(got[i][1], v.astype(np.int8)), ("oracle", i, im.shape, R)
        U1, V1 = ctx.to_host(*ctx.encode_gray(torch.from_numpy(im[None].copy()).cuda(), R, K, bounds, None if sg is None else torch.from_numpy(sg[None].copy())))
        assert np.array_equal(got[i][0], U1[0].numpy()) and np.array_equal(got[i][1], V1[0].numpy()), ("encode_gray", i, im.shape, R)


def test_ragged_bytes_do_not_depend_on_order_neighbours_or_alignment():
    """the list reversed, with a decoy image inserted, and from a base one byte past 16-byte alignment (the general planes body
    for every image): the same bytes per image"""
    ctx = _ctx()
    cfg = 1
    bounds, K = CONFIGS[cfg]
    ims, ranks = list(images()), ranks_of(cfg)
    signs = [signs_of(i, R) for i, R in enumerate(ranks)]
    want = encoded(cfg)
    same(encode_list(ctx, ims[::-1], ranks[::-1], signs[::-1], bounds, K)[::-1], want, "reversed")
    decoy = np.random.default_rng(9).integers(0, 256, (40, 72), dtype=np.uint8)
    got = encode_list(ctx, ims[:5] + [decoy] + ims[5:], ranks[:5] + [13] + ranks[5:], signs[:5] + [None] + signs[5:], bounds, K)
    same(got[:5] + got[6:], want, "decoy")
    flat, _ = pack(ims, 1)
    assert flat.data_ptr() % 16 == 1
    same(encode_list(ctx, ims, ranks, signs, bounds, K, base=1), want, "base + 1")


def _raw_encode(ctx, lib, items, flat, U, V, K=10, lo=-16, hi=15):
    from lrf_amd import _lib
    desc = (_lib.GrayEncodeImage * len(items))()
    for d, (H, W, R, go, uo, vo) in zip(desc, items):
        d.H, d.W, d.R, d.gray_off, d.u_off, d.v_off, d.sign_off = H, W, R, go, uo, vo, -1
    return lib.lrf_qmf_encode_gray_ragged_u8(ctx._h, len(items), desc, ctypes.c_void_p(flat.data_ptr()), flat.numel(), K, lo, hi, None, 0,
                                             ctypes.c_void_p(U.data_ptr()), U.numel(), ctypes.c_void_p(V.data_ptr()), V.numel())


def test_refusals_leave_the_outputs_untouched():
    """rank 33 is LRF_ENOTSUP; that and the LRF_EINVAL refusals of a list whose first image is fine leave canary-filled U and V as they were"""
    from lrf_amd import _lib
    ctx, lib = _ctx(), _lib.load()
    ims = [images()[4], images()[7]]  # 37x53, 64x96
    flat, offs = pack(ims)
    M = [patches(*im.shape) for im in ims]
    U = torch.full((M[0] * 4 + M[1] * 33,), 0x5A, dtype=torch.int8, device="cuda")
    V = torch.full((64 * 4 + 64 * 33,), 0x5A, dtype=torch.int8, device="cuda")
    ok = (37, 53, 4, offs[0], 0, 0)

    def second(R=4, go=offs[1], uo=M[0] * 4, vo=64 * 4, H=64, W=96):
        return (H, W, R, go, uo, vo)
    ENOTSUP, EINVAL = -2, -1  # LRF_ENOTSUP, LRF_EINVAL (include/lrf_hip.h)
    cases = [(ENOTSUP, second(R=33)), (EINVAL, second(R=0)), (EINVAL, second(go=-1)), (EINVAL, second(go=flat.numel() - 64 * 96 + 1)),
             (EINVAL, second(uo=M[0] * 4 - 1)), (EINVAL, second(vo=V.numel() - 64 * 4 + 1)), (EINVAL, second(uo=-1)), (EINVAL, second(H=1 << 21)),
             (EINVAL, second(H=9, W=2))]
    for want, item in cases:
        assert _raw_encode(ctx, lib, [ok, item], flat, U, V) == want, item
    assert _raw_encode(ctx, lib, [ok, second()], flat, U, V, K=0) == ENOTSUP
    assert _raw_encode(ctx, lib, [ok, second()], flat, U, V, lo=5, hi=4) == EINVAL
    ctx.synchronize()
    assert bool((U == 0x5A).all()) and bool((V == 0x5A).all())
    assert _raw_encode(ctx, lib, [ok, second()], flat, U, V) == 0  # (and the list itself is accepted)
    ctx.synchronize()
    assert not bool((U[:M[0] * 4] == 0x5A).all())
    with pytest.raises(ValueError, match="rank 33"):
        ctx.encode_gray_ragged(flat, [(64, 96, 33, offs[1])], 10, -16, 15)


def test_sweep_candidates_equal_the_ragged_encode_alone():
    """each image at ranks {1, 3, 8, 9, 20, 32}, the candidates interleaved across images; with signs [32] per image a candidate of
    rank R uses the leading R; every candidate = the ragged encode of (image, R) alone"""
    ctx = _ctx()
    ims = images()
    flat, offs = pack(ims)
    signs = [signs_of(i, 32) for i in range(len(ims))]
    sg, soffs = sign_buffer(signs)
    cands = [(i, R) for R in SWEEP_RANKS[::-1] for i in range(len(ims))][::-1]  # rank by rank, so an image's candidates lie apart
    cands = cands[1::2] + cands[0::2]
    out = ctx.encode_gray_ragged_sweep(flat, [(im.shape[0], im.shape[1], o, so) for im, o, so in zip(ims, offs, soffs)], cands, 10, -16, 15, sg)
    got = split(*out, [(patches(*ims[i].shape), R) for i, R in cands])
    for j, (i, R) in enumerate(cands):
        want = encode_list(ctx, [ims[i]], [R], [None if signs[i] is None else signs[i][:R]], (-16, 15), 10)
        same([got[j]], want, (j, i, R))


def sse_numpy(u, v, src):
    P = int_plane(u, v, *src.shape)
    return int(((np.clip(P, 0, 255) - src.astype(np.int64)) ** 2).sum())


def sse_items():
    """(u, v, source index): the factors of the encode at K = 10, (-16,15), and random int8 factors at ranks 1, 5, 33, 64 whose
    planes pass 255 and fall below 0; two items per source at least"""
    ims = images()
    items = [(u, v, i) for i, (u, v) in enumerate(encoded(1))]
    rng = np.random.default_rng(21)
    for k, R in enumerate([1, 5, 33, 64] * 2):
        i = (3 * k + 1) % len(ims)
        a = 40 if R == 1 else 12
        items.append((rng.integers(-a, a, (patches(*ims[i].shape), R), dtype=np.int8), rng.integers(-a, a, (64, R), dtype=np.int8), i))
    order = np.random.default_rng(3).permutation(len(items))
    return [items[j] for j in order]


def sse_call(ctx, items, flat, offs):
    ims = images()
    U = torch.from_numpy(np.concatenate([u.reshape(-1) for u, _, _ in items])).cuda()
    V = torch.from_numpy(np.concatenate([v.reshape(-1) for _, v, _ in items])).cuda()
    desc, uo, vo = [], 0, 0
    for u, v, i in items:
        desc.append((ims[i].shape[0], ims[i].shape[1], u.shape[1], uo, vo, offs[i]))
        uo += u.size
        vo += v.size
    return U, V, desc, ctx.sse_gray_ragged(flat, desc, U, V)


def test_sse_equals_numpy_and_decode_then_metrics():
    ctx = _ctx()
    ims = images()
    items = sse_items()
    flat, offs = pack(ims)
    U, V, desc, sse = sse_call(ctx, items, flat, offs)
    got = sse.cpu().tolist()
    want = [sse_numpy(u, v, ims[i]) for u, v, i in items]
    assert got == want
    planes = [np.clip(int_plane(u, v, *ims[i].shape), 0, 255) for u, v, i in items]
    assert any((int_plane(u, v, *ims[i].shape) > 255).any() for u, v, i in items) and any((int_plane(u, v, *ims[i].shape) < 0).any() for u, v, i in items)
    assert all(p.shape == ims[i].shape for p, (_, _, i) in zip(planes, items))
    dec = ctx.decode_gray_ragged(U, V, [d[:5] for d in desc])
    for j, (d, (_, _, i)) in enumerate(zip(dec, items)):
        s, _ = ctx.image_metrics(d[None].contiguous(), torch.from_numpy(ims[i][None, None].copy()).cuda(), want_ssim=False)
        assert int(s[0]) == got[j], j
    # a second call of the same list lands on zeroed sums again
    assert ctx.sse_gray_ragged(flat, desc, U, V).cpu().tolist() == want


def test_the_three_entries_on_a_callers_side_stream():
    """one call of each entry on a side stream behind a busy producer that writes the inputs: the bytes of the context's stream"""
    ctx = _ctx()
    ims = images()
    flat, offs = pack(ims)
    ranks = ranks_of(1)
    enc_list = [(im.shape[0], im.shape[1], R, o) for im, R, o in zip(ims, ranks, offs)]
    sw_ims = [(im.shape[0], im.shape[1], o) for im, o in zip(ims, offs)]
    cands = [(i, R) for R in (3, 20) for i in range(len(ims))]
    want_enc = ctx.encode_gray_ragged(flat, enc_list, 10, -16, 15)
    want_sw = ctx.encode_gray_ragged_sweep(flat, sw_ims, cands, 10, -16, 15)
    items = [(im.shape[0], im.shape[1], R, uo, vo, o) for im, R, uo, vo, o in zip(ims, ranks, want_enc[2], want_enc[3], offs)]
    want_sse = ctx.sse_gray_ragged(flat, items, want_enc[0], want_enc[1])
    torch.cuda.synchronize()
    real, decoy = flat.clone(), torch.full_like(flat, 0x33)
    Ureal, Udecoy = want_enc[0].clone(), torch.zeros_like(want_enc[0])
    Ubuf = want_enc[0].clone()
    a = torch.randn(2048, 2048, device="cuda")
    flat.copy_(decoy)
    Ubuf.copy_(Udecoy)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        b = a
        for _ in range(40):
            b = torch.mm(a, b) * 1e-3
        flat.copy_(real)
        Ubuf.copy_(Ureal)
        got_enc = ctx.encode_gray_ragged(flat, enc_list, 10, -16, 15)
        got_sw = ctx.encode_gray_ragged_sweep(flat, sw_ims, cands, 10, -16, 15)
        got_sse = ctx.sse_gray_ragged(flat, items, Ubuf, want_enc[1])
        snaps = [t.clone() for t in (got_enc[0], got_enc[1], got_sw[0], got_sw[1], got_sse)]
        flat.copy_(decoy)
        Ubuf.copy_(Udecoy)
    S.synchronize()
    for g, w in zip(snaps, (want_enc[0], want_enc[1], want_sw[0], want_sw[1], want_sse)):
        assert torch.equal(g, w)
    assert got_enc[2:] == want_enc[2:] and got_sw[2:] == want_sw[2:]
