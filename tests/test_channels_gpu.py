"""Gray and n-channel images through qmf_encode / qmf_decode on the GPU (-m gpu): the gray planes kernels at every size residue,
lrf_qmf_encode_gray_u8 bit for bit against the oracle's 64-column path over every rank family, the integer decoder against its
numpy definition, the general route, the reference's fixtures, the batch calls and one call at production size."""
import numpy as np
import pytest
import torch

from test_channels import CHAN_CASES, GRAY8_CASES, ChanCase, chan_decode_numpy

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (16, 24), (37, 53), (64, 96), (56, 440), (173, 264)]  # M = 1, 6, 35, 96, 385 (past one 384-row block), 726
RANKS = [1, 4, 7, 8, 9, 16, 17, 32, 33, 64]  # every rank family, R > M on the small sizes


def smooth(rng, C, H, W):
    """bilinear-upsampled noise plus N(0, 4), uint8 [C,H,W]"""
    base = torch.from_numpy(rng.random((1, C, max(H // 8, 1), max(W // 8, 1)), dtype=np.float32) * 255)
    sm = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    return np.clip(sm + rng.normal(size=sm.shape) * 4, 0, 255).astype(np.uint8)


def _psnr(a, b):
    mse = np.mean((np.asarray(a, np.float32) - np.asarray(b, np.float32)) ** 2)
    return 20 * np.log10(255 / np.sqrt(mse))


def _ctx():
    from lrf_amd import _lib
    return _lib.context(0)


# ---------------------------------------------------------------- gray planes
PLANE_SIZES = [(24 + i, 40 + j) for i in range(8) for j in range(8)] + [(8, 8), (16, 16), (32, 48)]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "base+1"])
def test_gray_planes_equal_pad_patchify_at_every_residue(offset, oracle):
    """X of the gray route (lrf_qmf_chan_matrix_u8 with C = 1 and 8x8 patches runs lrf_qmf_encode_gray_u8's planes stage): all 64
    (H, W) residues mod 8, one patch, and sizes of the 16-byte body; batch of 3; once more from a base one byte past alignment"""
    ctx = _ctx()
    rng = np.random.default_rng(5)
    for H, W in PLANE_SIZES:
        img = rng.integers(0, 256, (3, 1, H, W), dtype=np.uint8)
        buf = torch.zeros(img.size + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        dev = buf[offset:offset + img.size].view(3, 1, H, W)
        dev.copy_(torch.from_numpy(img))
        assert dev.data_ptr() % 16 == offset
        X = ctx.chan_matrix(dev, (8, 8)).cpu().numpy()
        for b in range(3):
            assert np.array_equal(X[b], oracle.pad_patchify(img[b].astype(np.float32))), (H, W, b)


# ---------------------------------------------------------------- gray encode
@pytest.mark.parametrize("H, W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_gray_encode_equals_oracle_bit_for_bit(H, W, oracle):
    """lrf_qmf_encode_gray_u8 = oracle.qmf_decompose(oracle.pad_patchify(img)): a randint image (X is integer: quotients land
    exactly on k + 0.5) and a smooth one per call, with and without column signs"""
    ctx = _ctx()
    rng = np.random.default_rng(H * 1000 + W)
    img = np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8), smooth(rng, 1, H, W)[0]])
    dev = torch.from_numpy(img).cuda()
    X = [oracle.pad_patchify(im[None].astype(np.float32)) for im in img]
    for R in RANKS:
        sign = rng.choice(np.array([-1, 1], dtype=np.int8), size=(2, R))
        for bounds in [(-16, 15), (-128, 127)]:
            for K in (1, 10):
                for sg in (None, sign):
                    U, V = ctx.to_host(*ctx.encode_gray(dev, R, K, bounds, None if sg is None else torch.from_numpy(sg)))
                    for b in range(2):
                        u, v = oracle.qmf_decompose(X[b], R, K, bounds, None if sg is None else sg[b])
                        assert np.array_equal(U[b].numpy(), u.astype(np.int8)) and np.array_equal(V[b].numpy(), v.astype(np.int8)), \
                            (H, W, R, bounds, K, sg is not None, b)


@pytest.mark.parametrize("H, W", [(37, 53), (56, 440)])
def test_gray_encode_from_given_factors_equals_oracle_bcd(H, W, oracle):
    ctx = _ctx()
    rng = np.random.default_rng(H + W)
    img = np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8), smooth(rng, 1, H, W)[0]])
    dev = torch.from_numpy(img).cuda()
    for R, K in [(4, 3), (16, 2), (32, 2), (40, 2)]:  # 40: the hand-over to the any-shape iteration
        X = [oracle.pad_patchify(im[None].astype(np.float32)) for im in img]
        u0 = (rng.normal(size=(2, X[0].shape[0], R)) * 3).astype(np.float32)
        v0 = (rng.normal(size=(2, 64, R)) * 3).astype(np.float32)
        U, V = ctx.to_host(*ctx.encode_gray(dev, R, K, (-16, 15), None, (torch.from_numpy(u0), torch.from_numpy(v0))))
        for b in range(2):
            u, v = oracle.bcd(X[b], u0[b], v0[b], K, (-16, 15))
            assert np.array_equal(U[b].numpy(), u.astype(np.int8)) and np.array_equal(V[b].numpy(), v.astype(np.int8)), (R, K, b)


# ---------------------------------------------------------------- gray decode
DEC_SIZES = SIZES + [(9, w) for w in range(1, 20)]


@pytest.mark.parametrize("H, W", DEC_SIZES, ids=[f"{h}x{w}" for h, w in DEC_SIZES])
def test_gray_decode_equals_numpy_definition(H, W, oracle):
    """clamp(u @ v.T) with depatchify and the centre crop, exact integers; widths 1..19 at H = 9 walk the store tails.  Widths
    1..3 have no reflect padding to 8 (pad // 2 or the rest reaches the image width): the geometry refuses them, as the reference's
    pad does."""
    from lrf_amd import _lib
    ctx = _ctx()
    if W < 4:
        with pytest.raises(ValueError, match="reflect padding"):
            _lib.chan_dims(H, W, 1, (8, 8))
        return
    _, _, M, _ = _lib.chan_dims(H, W, 1, (8, 8))
    rng = np.random.default_rng(H * 100 + W)
    for R in (1, 3, 8, 9, 32, 64):
        for lo, hi in [(-16, 15), (-128, 127)]:
            u = rng.integers(lo, hi + 1, (3, M, R), dtype=np.int8)
            v = rng.integers(lo, hi + 1, (3, 64, R), dtype=np.int8)
            out = ctx.decode_gray(torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(), H, W).cpu().numpy()
            for b in range(3):
                want = chan_decode_numpy(oracle, u[b], v[b], 1, H, W, (8, 8))[0]
                assert np.array_equal(out[b], want), (H, W, R, lo, b)
            assert R < 8 or (out.min() == 0 and out.max() == 255)  # both clamps are reached


# ---------------------------------------------------------------- the general route
@pytest.mark.parametrize("C", [1, 2, 4, 5])
@pytest.mark.parametrize("patch_size", [(8, 8), (4, 4), (8, 4), None], ids=["8x8", "4x4", "8x4", "nopatch"])
def test_general_route_matrix_decode_and_encode(C, patch_size, oracle):
    import lrf_amd
    from lrf_amd import _lib
    from lrf_amd.container import decode_tensor, separate_bytes
    ctx = _ctx()
    H, W, R, K = 37, 53, 3, 10
    rng = np.random.default_rng(C * 10 + (0 if patch_size is None else patch_size[0] + patch_size[1]))
    img = smooth(rng, C, H, W)
    Xo = oracle.rgb_matrix_any(img, patch_size)
    X = ctx.chan_matrix(torch.from_numpy(img).cuda().unsqueeze(0), patch_size)[0].cpu().numpy()
    assert np.array_equal(X, Xo)
    _, _, M, N = _lib.chan_dims(H, W, C, patch_size)
    us, vs = ((C, H, 5), (C, W, 5)) if patch_size is None else ((M, 5), (N, 5))
    u, v = rng.integers(-128, 128, us, dtype=np.int8), rng.integers(-128, 128, vs, dtype=np.int8)
    dec = ctx.chan_decode(torch.from_numpy(u).cuda().unsqueeze(0), torch.from_numpy(v).cuda().unsqueeze(0), C, H, W, patch_size)[0]
    assert np.array_equal(dec.cpu().numpy(), chan_decode_numpy(oracle, u, v, C, H, W, patch_size))
    # full encode with own initialisation: the oracle run the same way
    kw = dict(patch=False) if patch_size is None else dict(patch_size=patch_size)
    enc = lrf_amd.qmf_encode(torch.from_numpy(img), rank=R, color_space="RGB", **kw)
    uh, vh = (decode_tensor(f) for f in separate_bytes(separate_bytes(enc, 2)[1], 2))
    uo, vo = [], []
    for Xm in ([Xo] if patch_size is not None else list(Xo)):
        if Xm.shape[1] == 64:  # C p q = 64: the tuned route
            a, b = oracle.qmf_decompose(Xm, R, K, (-16, 15))
        else:
            a, b = oracle.bcd(Xm, *oracle.svd_topr_any(Xm, R), K, (-16, 15))
        uo.append(a.astype(np.int8)); vo.append(b.astype(np.int8))
    uo, vo = (uo[0], vo[0]) if patch_size is not None else (np.stack(uo), np.stack(vo))
    assert np.array_equal(uh, uo) and np.array_equal(vh, vo)
    back = lrf_amd.qmf_decode(enc)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (C, H, W) and not back.is_cuda
    assert np.array_equal(back.numpy(), chan_decode_numpy(oracle, uo, vo, C, H, W, patch_size))


# ---------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize("name", CHAN_CASES)
def test_fixture_decode_and_encode_from_reference_init(name):
    import lrf_amd
    c = ChanCase(name)
    dec = lrf_amd.qmf_decode(c.encoded)
    assert dec.dtype == torch.uint8 and np.array_equal(dec.numpy(), c.decoded)
    enc = lrf_amd.qmf_encode(c.image, color_space="RGB", init=(c.z["u0"], c.z["v0"]), **c.kwargs)
    assert enc == c.encoded, "from the reference's initial factors the encoder must emit the reference's bytes"


@pytest.mark.parametrize("name", GRAY8_CASES)
def test_gray_fixture_own_init_with_reference_signs_gives_reference_bytes(name):
    import lrf_amd
    c = ChanCase(name)
    assert lrf_amd.qmf_encode(c.image, color_space="RGB", init_sign=torch.from_numpy(c.z["sign"]), **c.kwargs) == c.encoded


@pytest.mark.parametrize("name", [n for n in CHAN_CASES if n not in GRAY8_CASES])
def test_other_fixtures_own_init_reaches_reference_quality(name):
    """own initialisation: equal metadata, PSNR and size within tests/test_rgbspace.py's bars for this branch (8x8 patches with
    iterations: 0.1 dB and 3 % + 16 bytes; the other forms: 0.3 dB, 1.5 dB without iterations, and 8 %)"""
    import lrf_amd
    from lrf_amd.container import bytes_to_dict, separate_bytes
    c = ChanCase(name)
    enc = lrf_amd.qmf_encode(c.image, color_space="RGB", init_sign=torch.from_numpy(c.z["sign"]), **c.kwargs)
    assert bytes_to_dict(separate_bytes(enc, 2)[0]) == c.metadata()
    d = abs(_psnr(c.image.numpy(), lrf_amd.qmf_decode(enc).numpy()) - c.psnr)
    print(name, "psnr difference", d, "bytes", len(enc), "reference", len(c.encoded))
    if c.patch_size == (8, 8) and c.K >= 1:
        assert d < 0.1 and abs(len(enc) - len(c.encoded)) <= 0.03 * len(c.encoded) + 16
    else:
        assert d < (1.5 if c.K == 0 else 0.3) and abs(len(enc) / len(c.encoded) - 1) < 0.08


# ---------------------------------------------------------------- batch calls
def test_batch_calls_equal_the_single_image_calls():
    import lrf_amd
    rng = np.random.default_rng(77)
    images = torch.from_numpy(np.stack([smooth(rng, 1, 37, 53) for _ in range(5)]))
    streams = lrf_amd.qmf_encode_batch(images, color_space="RGB", quality=10)
    assert len(streams) == 5
    for i in range(5):
        assert streams[i] == lrf_amd.qmf_encode(images[i], color_space="RGB", quality=10)
    assert lrf_amd.qmf_encode_batch(images.cuda(), color_space="RGB", quality=10, pack_workers=1) == streams
    dec = lrf_amd.qmf_decode_batch(streams)
    assert dec.is_cuda and dec.dtype == torch.uint8 and tuple(dec.shape) == (5, 1, 37, 53)
    assert torch.equal(dec.cpu(), torch.stack([lrf_amd.qmf_decode(s) for s in streams]))
    other = lrf_amd.qmf_encode(images[0], color_space="RGB", quality=20)
    with pytest.raises(ValueError, match="differ"):
        lrf_amd.qmf_decode_batch([streams[0], other])
    colour = lrf_amd.qmf_encode(images[:3, 0], color_space="RGB", quality=10)
    with pytest.raises(ValueError, match="mixes"):
        lrf_amd.qmf_decode_batch([streams[0], colour])
    with pytest.raises(NotImplementedError, match="inflate"):
        lrf_amd.qmf_decode_batch(streams, inflate="device")
    with pytest.raises(NotImplementedError, match="deflate"):
        lrf_amd.qmf_encode_batch(images, color_space="RGB", quality=10, deflate="device")
    with pytest.raises(NotImplementedError, match="8x8"):
        lrf_amd.qmf_encode_batch(images, color_space="RGB", quality=10, patch_size=(4, 4))
    with pytest.raises(NotImplementedError, match="gray"):
        lrf_amd.qmf_encode_batch(images.expand(5, 2, 37, 53).contiguous(), color_space="RGB", quality=10)
    with pytest.raises(NotImplementedError, match="2"):
        lrf_amd.qmf_encode(images.expand(5, 2, 37, 53)[0], quality=10)


def test_three_channel_calls_keep_their_bytes():
    """the colour paths are untouched: a fixture of the RGB colour space and one of the default branch still come out byte for byte"""
    import os

    import lrf_amd
    from conftest import GOLDEN, make_image
    import json
    z = np.load(os.path.join(GOLDEN, "rgbsp_tiny_q4.npz"))
    img = make_image(json.loads(str(z["spec"])))
    init = (torch.from_numpy(z["u0"]).unsqueeze(0), torch.from_numpy(z["v0"]).unsqueeze(0))
    assert lrf_amd.qmf_encode(img, color_space="RGB", init=init, **json.loads(str(z["kwargs"]))) == z["encoded"].tobytes()
    z = np.load(os.path.join(GOLDEN, "tiny_q7.npz"))
    img = make_image(json.loads(str(z["spec"])))
    sign = np.concatenate([z[f"sign{c}"] for c in range(3)])
    one = lrf_amd.qmf_encode(img, quality=7, init_sign=sign)
    batch = lrf_amd.qmf_encode_batch(torch.stack([img, img]), quality=7, init_sign=np.stack([sign, sign]))
    assert batch == [one, one] and batch == lrf_amd.qmf_encode_batch(torch.stack([img, img]), quality=7, init_sign=np.stack([sign, sign]),
                                                                     color_space="YCbCr")
    assert torch.equal(lrf_amd.qmf_decode_batch(batch).cpu()[0], lrf_amd.qmf_decode(one))


# ---------------------------------------------------------------- at size
def test_production_batch_256_gray_images(oracle):
    """256 x 512x768 gray at rank 7 on the default thresholds: bit for bit Context.decompose on the X of lrf_qmf_chan_matrix_u8, ONE
    LRF_K_BCD_PERSIST launch (counted as tests/test_persist_at_size.py counts), three images against the oracle"""
    from lrf_amd import _lib
    ctx = _ctx()
    g = torch.Generator(device="cuda").manual_seed(3)
    base = torch.rand((256, 1, 64, 96), device="cuda", generator=g) * 255
    img = torch.nn.functional.interpolate(base, size=(512, 768), mode="bilinear", align_corners=False)
    img = (img + torch.randn(img.shape, device="cuda", generator=g) * 4).clamp(0, 255).to(torch.uint8)
    ctx.profile_kernels([_lib.LRF_K_BCD, _lib.LRF_K_BCD_PERSIST])
    ctx.profile_reset()
    U, V = ctx.encode_gray(img[:, 0], 7, 10, (-16, 15))
    torch.cuda.synchronize()
    npersist, nbcd = ctx.kernel_time(_lib.LRF_K_BCD_PERSIST)[1], ctx.kernel_time(_lib.LRF_K_BCD)[1]
    ctx.profile(False)
    assert (npersist, nbcd) == (1, 0), (npersist, nbcd)
    X = ctx.chan_matrix(img, (8, 8))
    assert tuple(X.shape) == (256, 6144, 64)
    U2, V2 = ctx.decompose(X, 7, 10, -16, 15)
    assert torch.equal(U, U2) and torch.equal(V, V2)
    Uh, Vh = ctx.to_host(U, V)
    for b in (0, 101, 255):
        u, v = oracle.qmf_decompose(oracle.pad_patchify(img[b].cpu().numpy().astype(np.float32)), 7, 10, (-16, 15))
        assert np.array_equal(Uh[b].numpy(), u.astype(np.int8)) and np.array_equal(Vh[b].numpy(), v.astype(np.int8)), b
