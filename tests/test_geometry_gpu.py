"""GPU suite (-m gpu): the geometry sweep.  The planes kernels, the uniform and ragged encoders, the uniform and ragged decoders,
the squared error from the factors, crops, scaled decodes and the any-shape path at every size residue modulo 16 (the 256 sizes of
RESIDUES), at sizes wider than one 32-patch column group (WIDE), and at scale factors and patch settings other than the default
(ANY).  Expected values come from the definition in tests/geometry_cases.py — torch's CPU operators, gated against the CPU oracle
and the reference's pixels by tests/test_geometry.py — computed on the host, once per (size, ranks), shared and never written to.
The decoders run on factors whose pixels stay clear of the clamp (midrange_factors), so a sample taken one row or column off shows.
Every comparison is bit for bit; a failure names its (H, W, ranks)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _geometry_worker as GW
import geometry_cases as G
import scaled_decode as SD

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ENC_RANKS, ENC_K, LO, HI = (3, 2, 2), 2, -16, 15
ALL_SIZES = G.RESIDUES + G.WIDE


def _ctx():
    from lrf_amd import _lib
    return _lib.context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the host first -----------------------------------------------------------------------------------------------------------
def test_definition_equals_the_oracle_on_this_host(oracle):
    """ten sizes: a host whose torch sums an einsum or pools an area in another order fails HERE, not as a kernel mismatch below"""
    for H, W in G.RESIDUES[::29] + [G.WIDE[3]]:
        for got, want in zip(oracle.rgb_to_planes(G.image(H, W).numpy()), G.planes(H, W)):
            assert np.array_equal(_bits(got), _bits(want)), ("planes: this host's torch differs from the oracle", H, W)
        f6 = G.factors(H, W, (7, 3, 3))
        assert np.array_equal(oracle.planes_to_rgb(f6[0::2], f6[1::2], H, W), G.decoded(H, W, (7, 3, 3))), ("decode: this host's torch differs", H, W)
    assert len(G.RESIDUES[::29]) == 9


# ---- 1. planes -----------------------------------------------------------------------------------------------------------------
def _want_planes(H, W, ks=(0, 1)):
    return np.stack([np.concatenate([x.reshape(-1) for x in G.planes(H, W, k)]) for k in ks])


def _batch(H, W):
    return torch.stack([G.image(H, W, 0), G.image(H, W, 1)])


def test_planes_at_every_residue():
    ctx = _ctx()
    bad = []
    for H, W in ALL_SIZES:
        X = ctx.planes_from_rgb(_batch(H, W).cuda()).cpu().numpy()
        want = _want_planes(H, W)
        if X.shape != want.shape or not np.array_equal(_bits(X), _bits(want)):
            bad.append((H, W, "body", G.planes_body(H, W), int(np.sum(_bits(X) != _bits(want))) if X.shape == want.shape else X.shape))
    assert not bad, f"{len(bad)} of {len(ALL_SIZES)} sizes differ: {bad[:12]}"


def test_planes_from_a_view_one_byte_off_alignment():
    """the diagonal sizes from bytes that start at 1 mod 8: sides that are multiples of 16 leave k_planes16 for the strip body"""
    ctx = _ctx()
    for H, W in G.DIAGONAL:
        imgs = _batch(H, W)
        flat = torch.empty(imgs.numel() + 8, dtype=torch.uint8, device="cuda")
        off = (1 - flat.data_ptr()) % 8
        shifted = flat[off:off + imgs.numel()].view(imgs.shape)
        shifted.copy_(imgs)
        assert shifted.data_ptr() % 8 == 1 and shifted.is_contiguous()
        X = ctx.planes_from_rgb(shifted).cpu().numpy()
        assert np.array_equal(_bits(X), _bits(_want_planes(H, W))), (H, W, "body", G.planes_body(H, W, aligned8=False))


# ---- 2. uniform encode ---------------------------------------------------------------------------------------------------------
_want_rows = {}


def _oracle_rows(oracle, planes, ranks, K):
    """the oracle's int8 rows (U, V) of one image from the definition's planes"""
    f6 = []
    for X, R in zip(planes, ranks):
        u, v = oracle.qmf_decompose(X, R, K, (LO, HI))
        f6 += [u.astype(np.int8), v.astype(np.int8)]
    return G.flat_rows(f6)


def _want_encode(oracle, H, W, ranks=ENC_RANKS, K=ENC_K, k=0):
    key = (H, W, ranks, K, k)
    if key not in _want_rows:
        _want_rows[key] = _oracle_rows(oracle, G.planes(H, W, k), ranks, K)
    return _want_rows[key]


def _encode_mismatches(oracle, sizes, ranks):
    import lrf_amd
    bad = []
    for H, W in sizes:
        U, V = lrf_amd.qmf_factorize_batch(_batch(H, W).cuda(), ranks, num_iters=ENC_K, bounds=(LO, HI))
        U, V = U.cpu().numpy(), V.cpu().numpy()
        for k in (0, 1):
            wu, wv = _want_encode(oracle, H, W, ranks, ENC_K, k)
            if U[k].shape != wu.shape or V[k].shape != wv.shape or not (np.array_equal(U[k], wu) and np.array_equal(V[k], wv)):
                bad.append((H, W, ranks, "image", k))
    return bad


def test_uniform_encode_at_every_residue(oracle):
    bad = _encode_mismatches(oracle, ALL_SIZES, ENC_RANKS)
    assert not bad, f"{len(bad)} images differ from the oracle: {bad[:12]}"


def test_uniform_encode_at_ranks_7_3_3(oracle):
    bad = _encode_mismatches(oracle, [(32, 32), (48, 48), (32, 48), (47, 47)], (7, 3, 3))
    assert not bad, bad


def test_uniform_encode_of_a_large_batch_reads_luma_from_the_bytes(oracle, tmp_path):
    """tests/_geometry_worker.py under LRF_PERSIST=1 and LRF_FUSED_GRAM_MIN_CHUNKS=1: one child, three sizes, a batch of 1024
    blocks each — the patch matrices from k_planes16_gram, luma from the image bytes — every image against the oracle on the
    definition's planes"""
    from _luma_bytes_worker import batch_size
    out = str(tmp_path / "geometry.npz")
    env = dict(os.environ, LRF_PERSIST="1", LRF_FUSED_GRAM_MIN_CHUNKS="1")
    env.pop("LRF_LUMA_BYTES", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_geometry_worker.py"), out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "DONE" in r.stdout, r.stdout[-2000:]
    with np.load(out) as z:
        res = {k: z[k] for k in z.files}
    bad = []
    for H, W in GW.SIZES:
        key = f"{H}x{W}"
        imgs, U, V = res[key + "_images"], res[key + "_U"], res[key + "_V"]
        assert imgs.shape[0] == batch_size(H, W, GW.MIN_BLOCKS) and U.shape[0] == imgs.shape[0]
        persist, planes_gram, planes_plain = (int(x) for x in res[key + "_launches"])
        assert (persist, planes_gram, planes_plain) == (1, 1, 0), (key, persist, planes_gram, planes_plain)
        assert str(res[key + "_source"]) == "bytes", (key, str(res[key + "_source"]))
        for b in range(imgs.shape[0]):
            wu, wv = _oracle_rows(oracle, G.ref_planes(imgs[b]), GW.RANKS, GW.K)
            if not (np.array_equal(U[b], wu) and np.array_equal(V[b], wv)):
                bad.append((H, W, "image", b))
    assert not bad, f"{len(bad)} images differ from the oracle: {bad[:12]}"


# ---- 3. ragged encode ----------------------------------------------------------------------------------------------------------
def _encode_ragged(sizes):
    """encode_ragged of image(H, W) for the sizes in this order -> [(U, V) numpy rows]"""
    ctx = _ctx()
    offs, off = [], 0
    for H, W in sizes:
        offs.append(off)
        off = (off + 3 * H * W + 15) // 16 * 16
    flat = torch.zeros((off,), dtype=torch.uint8)
    for (H, W), o in zip(sizes, offs):
        flat[o:o + 3 * H * W] = G.image(H, W).reshape(-1)
    U, V, u_off, v_off = ctx.encode_ragged(flat.cuda(), [(H, W, ENC_RANKS, o) for (H, W), o in zip(sizes, offs)], ENC_K, LO, HI)
    Uh, Vh = (x.numpy() for x in ctx.to_host(U, V))
    return [(Uh[a:b], Vh[c:d]) for a, b, c, d in zip(u_off, u_off[1:] + [Uh.size], v_off, v_off[1:] + [Vh.size])]


def _ragged_encode_mismatches(oracle, sizes):
    bad = []
    for (H, W), (u, v) in zip(sizes, _encode_ragged(sizes)):
        wu, wv = _want_encode(oracle, H, W)
        if u.shape != wu.shape or v.shape != wv.shape or not (np.array_equal(u, wu) and np.array_equal(v, wv)):
            bad.append((H, W, ENC_RANKS, "body", G.planes_body(H, W)))
    return bad


def test_ragged_encode_of_all_residues_in_one_call(oracle):
    bad = _ragged_encode_mismatches(oracle, G.RESIDUES)
    assert not bad, f"{len(bad)} of 256 images differ from the oracle: {bad[:12]}"


def test_ragged_encode_of_the_wide_sizes(oracle):
    bad = _ragged_encode_mismatches(oracle, G.WIDE)
    assert not bad, bad


def test_ragged_encode_in_reversed_order_gives_the_same_bytes(oracle):
    bad = _ragged_encode_mismatches(oracle, G.RESIDUES[::-1])
    assert not bad, f"{len(bad)} of 256 images differ from the oracle: {bad[:12]}"


# ---- 4. uniform decode ---------------------------------------------------------------------------------------------------------
def _sizes_of(ranks):
    return G.RESIDUES + (G.WIDE if ranks in G.WIDE_TRIPLES else [])


@pytest.mark.parametrize("ranks", G.DECODE_TRIPLES, ids=str)
def test_uniform_decode_at_every_residue(ranks):
    ctx = _ctx()
    bad = []
    for H, W in _sizes_of(ranks):
        rows = [G.flat_rows(G.factors(H, W, ranks, k)) for k in (0, 1)]
        U = torch.from_numpy(np.stack([r[0] for r in rows])).cuda()
        V = torch.from_numpy(np.stack([r[1] for r in rows])).cuda()
        got = ctx.decode_rgb(U, V, H, W, list(ranks)).cpu().numpy()
        for k in (0, 1):
            if not np.array_equal(got[k], G.decoded(H, W, ranks, k)):
                bad.append((H, W, ranks, "image", k, "group", G.decode_group(H, W, ranks), int(np.sum(got[k] != G.decoded(H, W, ranks, k)))))
    assert not bad, f"{len(bad)} images differ: {bad[:12]}"


# ---- 5. ragged decode ----------------------------------------------------------------------------------------------------------
class Ragged:
    """a list of (H, W, ranks): the factors of geometry_cases.factors back to back in two device buffers"""

    def __init__(self, items):
        self.items = items
        rows = [G.flat_rows(G.factors(H, W, t)) for H, W, t in items]
        self.U = torch.from_numpy(np.concatenate([r[0] for r in rows])).cuda()
        self.V = torch.from_numpy(np.concatenate([r[1] for r in rows])).cuda()
        uo = np.cumsum([0] + [r[0].size for r in rows])
        vo = np.cumsum([0] + [r[1].size for r in rows])
        self.images = [(H, W, t, int(a), int(b)) for (H, W, t), a, b in zip(items, uo, vo)]


_lists = {}


def _list_of(key):
    if key not in _lists:
        _lists[key] = Ragged(mixed_items() if key == "mixed" else [(H, W, key) for H, W in _sizes_of(key)])
    return _lists[key]


def mixed_items():
    """every size of RESIDUES and of WIDE once, the triples dealt so that every triple meets every kind of size and neighbours are
    of different launch groups"""
    items = [(H, W, G.DECODE_TRIPLES[(3 * i + i // 16) % 8]) for i, (H, W) in enumerate(G.RESIDUES)]
    for j, (H, W) in enumerate(G.WIDE):
        items.insert(17 * j + 5, (H, W, G.WIDE_TRIPLES[j % 3]))
    return items


def _launch_group(H, W, t):
    kind, cls = G.decode_group(H, W, t)
    return kind, (cls if kind == G.DEC_STRIP else 0)


def test_the_mixed_list_mixes():
    items = mixed_items()
    assert len(items) == 272 and len(set(items)) == 272
    groups = [_launch_group(*it) for it in items]
    assert set(groups) == {(G.DEC_TILE16, 0), (G.DEC_R8, 0), (G.DEC_ANY, 0)} | {(G.DEC_STRIP, c) for c in range(5)}  # all eight launches
    assert sum(a != b for a, b in zip(groups, groups[1:])) >= 136, sum(a != b for a, b in zip(groups, groups[1:]))
    assert {t for _, _, t in items} == set(G.DECODE_TRIPLES)


def _ragged_decode_mismatches(lst):
    out = _ctx().decode_ragged(lst.U, lst.V, lst.images)
    assert len(out) == len(lst.items)
    bad = []
    for o, (H, W, t) in zip(out, lst.items):
        got = o.cpu().numpy()
        if got.shape != (3, H, W) or not np.array_equal(got, G.decoded(H, W, t)):
            bad.append((H, W, t, "group", G.decode_group(H, W, t)))
    return bad


@pytest.mark.parametrize("ranks", G.DECODE_TRIPLES, ids=str)
def test_ragged_decode_of_all_residues_in_one_call(ranks):
    bad = _ragged_decode_mismatches(_list_of(ranks))
    assert not bad, f"{len(bad)} images differ: {bad[:12]}"


def test_ragged_decode_of_the_mixed_list():
    bad = _ragged_decode_mismatches(_list_of("mixed"))
    assert not bad, f"{len(bad)} images differ: {bad[:12]}"


# ---- 6. squared error from the factors -----------------------------------------------------------------------------------------
def test_squared_error_of_the_mixed_list():
    lst = _list_of("mixed")
    offs, off = [], 0
    for H, W, _ in lst.items:
        offs.append(off)
        off += 3 * H * W  # back to back: sources at any alignment
    flat = torch.cat([G.image(H, W).reshape(-1) for H, W, _ in lst.items])
    assert flat.numel() == off
    sse = _ctx().sse_ragged(flat.cuda(), [im + (o,) for im, o in zip(lst.images, offs)], lst.U, lst.V).cpu().numpy()
    bad = []
    for s, (H, W, t) in zip(sse, lst.items):
        want = int(((G.decoded(H, W, t).astype(np.int64) - G.image(H, W).numpy().astype(np.int64)) ** 2).sum())
        if int(s) != want:
            bad.append((H, W, t, int(s), want))
    assert not bad, f"{len(bad)} sums differ: {bad[:12]}"


# ---- 7. crops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [(7, 3, 3), (26, 13, 13)], ids=str)
def test_crops_at_every_residue(ranks):
    """the whole image, its last 9 x 11 corner, and a 17 x 19 window from the odd (7, 9)"""
    ctx = _ctx()
    lst = _list_of(ranks)
    n = len(G.RESIDUES)
    images, items = lst.images[:n], lst.items[:n]
    bad = []
    for i, (H, W, t) in enumerate(items):  # the whole image: one size a call
        got = ctx.decode_crops(lst.U, lst.V, [images[i]], np.array([[0, 0, 0]]), (H, W)).cpu().numpy()
        if not np.array_equal(got[0], G.decoded(H, W, t)):
            bad.append((H, W, t, "whole"))
    corner = ctx.decode_crops(lst.U, lst.V, images, np.array([[i, H - 9, W - 11] for i, (H, W, _) in enumerate(items)]), (9, 11)).cpu().numpy()
    window = ctx.decode_crops(lst.U, lst.V, images, np.array([[i, 7, 9] for i in range(n)]), (17, 19)).cpu().numpy()
    for i, (H, W, t) in enumerate(items):
        full = G.decoded(H, W, t)
        if not np.array_equal(corner[i], full[:, H - 9:, W - 11:]):
            bad.append((H, W, t, "corner"))
        if not np.array_equal(window[i], full[:, 7:24, 9:28]):
            bad.append((H, W, t, "window at (7, 9)"))
    assert not bad, f"{len(bad)} crops differ: {bad[:12]}"


# ---- 8. scaled decode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [(7, 3, 3), (26, 13, 13), (64, 64, 64)], ids=str)
def test_scaled_decode_at_every_residue(ranks, oracle):
    ctx = _ctx()
    lst = _list_of(ranks)
    n = len(G.RESIDUES)
    bad = []
    for f in SD.SCALES:
        out = ctx.decode_scaled(lst.U, lst.V, lst.images[:n], f)
        for o, (H, W, t) in zip(out, lst.items[:n]):
            want = SD.reference_scaled(list(G.factors(H, W, t)), H, W, f, oracle)
            got = o.cpu().numpy()
            if got.shape != want.shape or not np.array_equal(got, want):
                bad.append((H, W, t, "scale", f))
    assert not bad, f"{len(bad)} images differ: {bad[:12]}"


# ---- 9. the any-shape path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf", G.SCALE_FACTORS, ids=[f"{a:.3g}x{b:.3g}" for a, b in G.SCALE_FACTORS])
def test_anyshape_planes_and_decode(sf):
    import lrf_amd
    from lrf_amd.codec import pack_anyshape
    ctx = _ctx()
    bad = []
    for H, W, ps, chroma in G.any_cases(sf):
        dev = _batch(H, W).cuda()
        want = [G.ref_planes(G.image(H, W, k), sf, ps) for k in (0, 1)]
        for ch in range(3):
            X = ctx.planes_any(dev, ps, ch, chroma).cpu().numpy()
            for k in (0, 1):
                if X[k].shape != want[k][ch].shape or not np.array_equal(_bits(X[k]), _bits(want[k][ch])):
                    bad.append((H, W, sf, ps, "planes", ch, "image", k))
        f6 = G.midrange_factors(np.random.default_rng([H, W, 9]), H, W, G.ANY_RANKS, ps, chroma)
        stream = pack_anyshape(f6 if ps is not None else [f[None] for f in f6], (H, W), list(G.ANY_RANKS), (LO, HI), ps, "uint8", chroma)
        got = lrf_amd.qmf_decode(stream).numpy()
        if not np.array_equal(got, G.ref_decode(f6, H, W, ps, chroma)):
            bad.append((H, W, sf, ps, "decode"))
    assert not bad, f"{len(bad)} differ: {bad[:12]}"
