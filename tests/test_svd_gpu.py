"""The kernels of lrf_svd_kernels.hip and the host code at the top of lrf_any.hip on the tables of tests/svd_cases.py: long
matrices (partial last chunks, chunk counts off the fold's unrolling, both sides of the LRF_G192_MAX_ROWS switch), batches
whose factor tensors are not multiples of 16 bytes, every size residue of every patch setting down to the smallest legal
sizes, full-range decoder factors that clamp on both sides, constant tensors, refusals.  Everything bit for bit — bytes and
fp32 bit patterns — against the definitions tests/test_svd_cases.py holds to the reference's fixtures."""
import ctypes

import numpy as np
import pytest
import torch

import svd_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lrf_amd import _lib
    return _lib.context(0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_encode(got, want, what):
    (U, V, qp), (qu, qv, wp) = got, want
    assert np.array_equal(qp.cpu().numpy().view(np.int32), wp.view(np.int32)), f"{what}: quantisation parameters {qp.cpu().numpy()} != {wp}"
    assert np.array_equal(V.cpu().numpy(), qv), f"{what}: V codes differ"
    assert np.array_equal(U.cpu().numpy(), qu), f"{what}: U codes differ"


def _encode_batch_equals_oracle(ctx, oracle, imgs, R, what):
    U, V, qp = ctx.svd_encode_rgb(_dev(imgs), R)
    for b in range(len(imgs)):
        u, v = oracle.svd_topr_u8(oracle.rgb_matrix_any(imgs[b], (8, 8)), R)
        _same_encode((U[b], V[b], qp[b]), sc.quantised(oracle, u, v), f"{what} image {b}")


# ---- encode -----------------------------------------------------------------------------------------------------------------
DENSE = [(name, R) for name in sc.DENSE for R in sc.ENC_RANKS]


@pytest.mark.parametrize("name,R", DENSE, ids=[f"{n}-R{R}" for n, R in DENSE])
def test_svd_encode_dense(name, R, ctx, oracle):
    """k_gram192_u8<uint8_t|float> + k_gram192_fold with a partial last chunk behind full ones and 2, 3, 5, 6, 7 chunks"""
    U, V, qp = ctx.svd_encode_rgb(_dev(sc.dense_image(name)[None]), R)
    _same_encode((U[0], V[0], qp[0]), sc.quantised(oracle, *sc.dense_factors(oracle, name, R)), name)


@pytest.mark.parametrize("name,R", DENSE, ids=[f"{n}-R{R}" for n, R in DENSE])
def test_float_form_dense(name, R, ctx, oracle):
    """svd_encode's float-dtype form: rgbspace_matrix_any + svd_init on the same matrices"""
    img = sc.dense_image(name)
    X = ctx.rgbspace_matrix_any(_dev(img[None]), (8, 8))
    assert np.array_equal(sc.bits(X[0].cpu().numpy()), sc.bits(oracle.rgb_matrix_any(img, (8, 8))))
    u0, v0 = ctx.svd_init(X, R)
    u, v = sc.dense_factors(oracle, name, R)
    assert np.array_equal(sc.bits(v0[0].cpu().numpy()), sc.bits(v)) and np.array_equal(sc.bits(u0[0].cpu().numpy()), sc.bits(u))


SCATTERED = [(name, R) for name in sc.SCATTERED for R in sc.SCATTERED_RANKS]


@pytest.mark.parametrize("name,R", SCATTERED, ids=[f"{n}-R{R}" for n, R in SCATTERED])
def test_svd_encode_scattered(name, R, ctx, oracle):
    """M = LRF_G192_MAX_ROWS (66 chunks, the byte matrix for R = 5, the fp32 one for R = 12) and one row more (k_gram_blk)"""
    Xc, rows, M = sc.scattered_case(name)
    img = _dev(sc.scattered_image(name)[None])
    X = ctx.rgbspace_matrix_any(img, (8, 8))[0]
    assert tuple(X.shape) == (M, 192) and np.array_equal(X[torch.from_numpy(rows).cuda()].cpu().numpy(), Xc) and float(X.sum(dtype=torch.float64)) == float(Xc.sum(dtype=np.float64))
    del X
    U, V, qp = ctx.svd_encode_rgb(img, R)
    u, v = oracle.svd_topr_u8(Xc, R)
    _same_encode((U[0], V[0], qp[0]), sc.quantised(oracle, sc.scatter_rows(u, M, rows), v), name)


@pytest.mark.parametrize("H,W,R", sc.BATCH, ids=[f"{H}x{W}-R{R}" for H, W, R in sc.BATCH])
def test_svd_encode_batch_off_alignment(H, W, R, ctx, oracle):
    """three different images in one call; image 1's u tensor starts off 16-byte alignment (k_minmax's scalar path beside the
    vector path with a tail), and everything per image is indexed by blockIdx.y"""
    _encode_batch_equals_oracle(ctx, oracle, sc.batch_images(H, W), R, f"{H}x{W}")


RES8 = [(H, W, R) for H, W in sc.RESIDUES[(8, 8)] for R in sc.ENC_RANKS]


@pytest.mark.parametrize("H,W,R", RES8, ids=[f"{H}x{W}-R{R}" for H, W, R in RES8])
def test_svd_encode_residues(H, W, R, ctx, oracle):
    """k_patchify_rgb<uint8_t|float> at every size residue and at the smallest legal sizes, three images per call"""
    _encode_batch_equals_oracle(ctx, oracle, sc.residue_images(H, W), R, f"{H}x{W}")


QMF = [("m3135", 3), ("m3135", 12)] + [(f"{H}x{W}", R) for H, W, R in sc.BATCH]


@pytest.mark.parametrize("name,R", QMF, ids=[f"{n}-R{R}" for n, R in QMF])
def test_qmf_rgbspace_encode_own_initialisation(name, R, ctx, oracle):
    """lrf_qmf_rgbspace_encode_u8: k_patchify_rgb<float>, k_gram192_u8<float> + fold, the any-shape solver, ten iterations"""
    imgs = sc.dense_image(name)[None] if name in sc.DENSE else sc.batch_images(*map(int, name.split("x")))
    U, V = ctx.qmf_rgbspace_encode(_dev(imgs), R, 10, (-16, 15))
    for b in range(len(imgs)):
        u, v = oracle.qmf_rgbspace_decompose(imgs[b], R, 10, (-16, 15))
        assert np.array_equal(V[b].cpu().numpy(), v.astype(np.int8)) and np.array_equal(U[b].cpu().numpy(), u.astype(np.int8)), (name, b)


# ---- matrix and decode --------------------------------------------------------------------------------------------------------
CASE_IDS = [sc.case_id(*c) for c in sc.RESIDUE_CASES]


@pytest.mark.parametrize("ps,H,W", sc.RESIDUE_CASES, ids=CASE_IDS)
def test_rgbspace_matrix(ps, H, W, ctx, oracle):
    imgs = sc.residue_images(H, W)
    X = ctx.rgbspace_matrix_any(_dev(imgs), ps).cpu().numpy()
    for b in range(3):
        assert np.array_equal(sc.bits(X[b]), sc.bits(oracle.rgb_matrix_any(imgs[b], ps))), b


def _stack(parts):
    return _dev(np.stack(parts))


@pytest.mark.parametrize("ps,H,W", sc.RESIDUE_CASES, ids=CASE_IDS)
def test_decoders(ps, H, W, ctx, oracle):
    """every decoder of the two files on three images with different factors per call, at ranks 1, 7 and the widest.  At the
    widest rank these sizes have at most 4 patch rows, where the order of the reference's fp32 product is not known
    (svd_cases.product_is_pinned): there the float decoders are held to the oracle's stated order, and test_decoders_wide
    holds the wide ranks to the reference's.  The integer decoders are exact in any order."""
    for R in sorted(set(sc.decoder_ranks("svd_decode_any", H, W, ps))):
        q = [sc.quant_factors(H, W, ps, R, b) for b in range(3)]
        qp6 = _dev(np.array([[pu[0], pu[1], qu.min(), pv[0], pv[1], qv.min()] for qu, qv, pu, pv in q], np.float32))
        want = [oracle.svd_decode_any(qu, qv, H, W, ps, pu, pv) for qu, qv, pu, pv in q]
        got = ctx.svd_decode_any(_stack([x[0] for x in q]), _stack([x[1] for x in q]), H, W, ps, qp6).cpu().numpy()
        for b in range(3):
            assert np.array_equal(got[b], want[b]), ("svd_decode_any, quantised", R, b)
        if ps == (8, 8) and R <= sc.ENTRY_MAX_RANK["svd_decode_rgb"]:
            got = ctx.svd_decode_rgb(_stack([x[0] for x in q]), _stack([x[1] for x in q]), qp6, H, W).cpu().numpy()
            for b in range(3):
                assert np.array_equal(got[b], want[b]), ("svd_decode_rgb", R, b)
        f = [sc.float_factors(H, W, ps, R, b) for b in range(3)]
        got = ctx.svd_decode_any(_stack([x[0] for x in f]), _stack([x[1] for x in f]), H, W, ps).cpu().numpy()
        for b in range(3):
            assert np.array_equal(got[b], oracle.svd_decode_any(f[b][0], f[b][1], H, W, ps)), ("svd_decode_any, float", R, b)
    for R in sorted(set(sc.decoder_ranks("qmf_rgbspace_decode_any", H, W, ps))):
        i8 = [sc.int8_factors(H, W, ps, R, b) for b in range(3)]
        want = [oracle.rgb_decode_any(u, v, H, W, ps) for u, v in i8]
        U, V = _stack([x[0] for x in i8]), _stack([x[1] for x in i8])
        got = ctx.qmf_rgbspace_decode_any(U, V, H, W, ps).cpu().numpy()
        for b in range(3):
            assert np.array_equal(got[b], want[b]), ("qmf_rgbspace_decode_any", R, b)
        if ps == (8, 8) and R <= sc.ENTRY_MAX_RANK["qmf_rgbspace_decode"]:
            got = ctx.qmf_rgbspace_decode(U, V, H, W).cpu().numpy()
            for b in range(3):
                assert np.array_equal(got[b], want[b]), ("qmf_rgbspace_decode", R, b)


@pytest.mark.parametrize("ps,H,W,R", sc.WIDE, ids=[sc.case_id(ps, H, W) + f"-R{R}" for ps, H, W, R in sc.WIDE])
def test_decoders_wide(ps, H, W, R, ctx, oracle):
    """the widest rank of every patch setting (and 500 and 385 ranks: the two halves) on images of 20 patch rows, where
    tests/test_svd_cases.py holds the definition's product to torch's own; the widest-rank cases of test_decoders (M <= 4)
    are held to the oracle's statement of the order only (svd_cases.product_is_pinned)"""
    q = [sc.quant_factors(H, W, ps, R, b) for b in range(2)]
    qp6 = _dev(np.array([[pu[0], pu[1], qu.min(), pv[0], pv[1], qv.min()] for qu, qv, pu, pv in q], np.float32))
    want = [oracle.svd_decode_any(qu, qv, H, W, ps, pu, pv) for qu, qv, pu, pv in q]
    got = ctx.svd_decode_any(_stack([x[0] for x in q]), _stack([x[1] for x in q]), H, W, ps, qp6).cpu().numpy()
    assert np.array_equal(got, np.stack(want)), "svd_decode_any, quantised"
    if ps == (8, 8):
        got = ctx.svd_decode_rgb(_stack([x[0] for x in q]), _stack([x[1] for x in q]), qp6, H, W).cpu().numpy()
        assert np.array_equal(got, np.stack(want)), "svd_decode_rgb"
    f = [sc.float_factors(H, W, ps, R, b) for b in range(2)]
    got = ctx.svd_decode_any(_stack([x[0] for x in f]), _stack([x[1] for x in f]), H, W, ps).cpu().numpy()
    assert np.array_equal(got, np.stack([oracle.svd_decode_any(u, v, H, W, ps) for u, v in f])), "svd_decode_any, float"


# ---- quantize_u8 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 2, 3, 5, 7, 255, 1025, 4099, 5003])
def test_quantize_u8_batches(per, ctx, oracle):
    """k_minmax + k_quantize_u8 on four tensors per call: per odd or below 4 puts tensors 1 and 3 (or all but 0) off 16-byte
    alignment; tensor 1 is constant (scale 0: codes 0, scale 0.0, min the value) between regular ones"""
    rng = np.random.default_rng(per)
    T = (rng.normal(size=(4, per)) * np.array([[3.0], [0.0], [200.0], [0.01]]) + np.array([[0.0], [-2.25], [50.0], [7.0]])).astype(np.float32)
    Q, qp = ctx.quantize_u8(_dev(T))
    Q, qp = Q.cpu().numpy(), qp.cpu().numpy()
    for b in range(4):
        q, s, m = oracle.quantize_u8(T[b])
        assert np.array_equal(qp[b].view(np.int32), np.array([s, m], np.float32).view(np.int32)), (b, qp[b], s, m)
        assert np.array_equal(Q[b], q), b
    assert not Q[1].any() and qp[1, 0] == 0.0 and qp[1, 1] == np.float32(-2.25)


@pytest.mark.parametrize("size,value,R", sc.CONSTANT_IMAGES)
def test_constant_image(size, value, R, ctx, oracle):
    """every row of u the same fma chain: max == min, scale 0 — and the decoders on what comes out"""
    H, W = size
    img = np.full((1, 3, H, W), value, np.uint8)
    U, V, qp = ctx.svd_encode_rgb(_dev(img), R)
    u, v = oracle.svd_topr_u8(oracle.rgb_matrix_any(img[0], (8, 8)), R)
    qu, qv, wp = sc.quantised(oracle, u, v)
    _same_encode((U[0], V[0], qp[0]), (qu, qv, wp), "constant image")
    want = oracle.svd_decode_any(qu, qv, H, W, (8, 8), (wp[0], wp[1]), (wp[2], wp[3]))
    qp6 = _dev(np.array([[wp[0], wp[1], qu.min(), wp[2], wp[3], qv.min()]], np.float32))
    assert np.array_equal(ctx.svd_decode_rgb(U, V, qp6, H, W)[0].cpu().numpy(), want)
    assert np.array_equal(ctx.svd_decode_any(U, V, H, W, (8, 8), qp6)[0].cpu().numpy(), want)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
REFUSED = [(ps, H, W) for ps in sc.PATCH_SETTINGS if ps is not None for H, W in sc.refused_sizes(ps)]


@pytest.mark.parametrize("ps,H,W", REFUSED, ids=[sc.case_id(*c) for c in REFUSED])
def test_refused_sizes_leave_the_output_untouched(ps, H, W, ctx):
    """a side whose reflect padding is not smaller than the side: LRF_EINVAL with the reflect-padding message from every entry
    that pads, before anything is launched — the poisoned outputs stay as they were"""
    from lrf_amd._lib import _dptr
    lib, h = ctx._lib, ctx._h
    p, q = ps
    R, n = 2, 1 << 16
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    qp6 = torch.ones(6, dtype=torch.float32, device="cuda")
    outs = [torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3)]
    a, b, c = (_dptr(o) for o in outs)
    s = _dptr(src)
    calls = [("lrf_qmf_rgbspace_matrix_u8", lambda: lib.lrf_qmf_rgbspace_matrix_u8(h, s, 1, H, W, p, q, a)),
             ("lrf_qmf_rgbspace_decode_any_u8", lambda: lib.lrf_qmf_rgbspace_decode_any_u8(h, s, s, 1, H, W, p, q, R, a)),
             ("lrf_svd_decode_any_u8 (quantised)", lambda: lib.lrf_svd_decode_any_u8(h, s, s, 0, 1, H, W, p, q, R, _dptr(qp6), a)),
             ("lrf_svd_decode_any_u8 (float)", lambda: lib.lrf_svd_decode_any_u8(h, s, s, 1, 1, H, W, p, q, R, None, a))]
    if ps == (8, 8):
        calls += [("lrf_svd_encode_rgb_u8", lambda: lib.lrf_svd_encode_rgb_u8(h, s, 1, H, W, R, None, a, b, c)),
                  ("lrf_svd_decode_rgb_u8", lambda: lib.lrf_svd_decode_rgb_u8(h, s, s, 1, H, W, R, _dptr(qp6), a)),
                  ("lrf_qmf_rgbspace_encode_u8", lambda: lib.lrf_qmf_rgbspace_encode_u8(h, s, 1, H, W, R, 10, -16, 15, None, None, None, a, b)),
                  ("lrf_qmf_rgbspace_decode_u8", lambda: lib.lrf_qmf_rgbspace_decode_u8(h, s, s, 1, H, W, R, a))]
    ctx.use_torch_stream()
    for name, call in calls:
        assert call() == -1, name  # LRF_EINVAL
        msg = lib.lrf_last_error().decode()
        assert "reflect padding larger than the image" in msg and f"{H}x{W}" in msg, (name, msg)
    dims = [ctypes.c_int64() for _ in range(4)]
    assert lib.lrf_rgbspace_dims_any(H, W, p, q, *[ctypes.byref(d) for d in dims]) == -1
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 0xA5).all())
