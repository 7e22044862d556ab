"""Gray and n-channel images through qmf_encode / qmf_decode (color_space="RGB"; the reference infers the channel count:
lrf/compression/qmf.py:43-56, 164-212, 309-323), CPU part: the numpy / oracle definition of the feature against the reference's
fixtures (tools/gen_golden_channels.py, reference run at one thread), the geometry entry lrf_chan_dims and the header walk."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

GRAY8_CASES = ["chan_g_odd_q10", "chan_g_tiny_r7", "chan_g_big_q7", "chan_g_q20", "chan_g_r9_m6", "chan_g_r3_it2", "chan_g_one_patch"]
OTHER_CASES = ["chan_g_p4_q10", "chan_g_nopatch_q8", "chan_g_it0_q6", "chan_c2_q5", "chan_c4_r4", "chan_c4_nopatch_r3"]
CHAN_CASES = GRAY8_CASES + OTHER_CASES


class ChanCase:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.z, self.name = z, name
        self.kwargs = json.loads(str(z["kwargs"]))
        self.encoded = z["encoded"].tobytes()
        self.image = torch.from_numpy(z["image"])
        self.decoded = z["decoded"]
        self.C = int(z["channels"])
        self.R, self.psnr = int(z["rank"]), float(z["psnr"])
        self.K = self.kwargs.get("num_iters", 10)
        self.bounds = tuple(self.kwargs.get("bounds", (-16, 15)))
        self.patch_size = tuple(self.kwargs.get("patch_size", (8, 8))) if self.kwargs.get("patch", True) else None

    def ref_factors(self):
        from lrf_amd.container import decode_tensor, separate_bytes
        return [decode_tensor(f) for f in separate_bytes(separate_bytes(self.encoded, 2)[1], 2)]

    def metadata(self):
        from lrf_amd.container import bytes_to_dict, separate_bytes
        return bytes_to_dict(separate_bytes(self.encoded, 2)[0])


def chan_decode_numpy(oracle, u, v, C, H, W, patch_size):
    """the definition of the decoders: int64 u @ v.T, depatchify + centre crop for C channels, clip"""
    if patch_size is None:
        x = np.einsum("chr,cwr->chw", u.astype(np.int64), v.astype(np.int64))
    else:
        p, q = patch_size
        Hp, Wp = H + (p - H % p) % p, W + (q - W % q) % q
        x = oracle.depatchify_unpad((u.astype(np.int64) @ v.astype(np.int64).T).astype(np.float32), C, Hp, Wp, H, W, p, q)
    return np.clip(x, 0, 255).astype(np.uint8)


def chan_matrix_numpy(oracle, img, patch_size):
    """the definition of the matrices: oracle.pad_patchify where its top = pad // 2 convention applies (any C), the numpy
    restatement oracle.rgb_matrix_any (written for any channel count) beside it"""
    X = oracle.rgb_matrix_any(img, patch_size)
    if patch_size is not None:
        assert np.array_equal(X, oracle.pad_patchify(img.astype(np.float32), *patch_size))
    return X


def factors_from_init(oracle, c):
    """the oracle's BCD from the reference's own (u0, v0) on the numpy matrices -> int8 (u, v) in the container's shapes"""
    X = chan_matrix_numpy(oracle, c.image.numpy(), c.patch_size)
    mats = [X] if c.patch_size is not None else list(X)
    us, vs = [], []
    for Xm, a, b in zip(mats, c.z["u0"], c.z["v0"]):
        if c.K == 0:
            u, v = torch.from_numpy(a).to(torch.int8).numpy(), torch.from_numpy(b).to(torch.int8).numpy()  # the truncating cast
        else:
            u, v = oracle.bcd(Xm, a, b, c.K, c.bounds)
        us.append(u.astype(np.int8)); vs.append(v.astype(np.int8))
    return (us[0], vs[0]) if c.patch_size is not None else (np.stack(us), np.stack(vs))


@pytest.mark.parametrize("name", CHAN_CASES)
def test_numpy_definition_gives_reference_pixels_and_factors(name, oracle):
    c = ChanCase(name)
    u_ref, v_ref = c.ref_factors()
    _, H, W = c.image.shape
    assert tuple(c.decoded.shape) == (c.C, H, W)
    assert np.array_equal(chan_decode_numpy(oracle, u_ref, v_ref, c.C, H, W, c.patch_size), c.decoded)
    u, v = factors_from_init(oracle, c)
    assert np.array_equal(u, u_ref) and np.array_equal(v, v_ref)


@pytest.mark.parametrize("name", GRAY8_CASES)
def test_oracle_64_column_path_with_reference_signs_gives_reference_factors(name, oracle):
    """gray 8x8 is one [M,64] matrix: oracle.qmf_decompose, fed the reference's LAPACK column signs, gives its int8 factors"""
    c = ChanCase(name)
    u_ref, v_ref = c.ref_factors()
    X = oracle.pad_patchify(c.image.numpy().astype(np.float32))
    assert X.shape[1] == 64
    u, v = oracle.qmf_decompose(X, c.R, c.K, c.bounds, c.z["sign"][0])
    assert np.array_equal(u.astype(np.int8), u_ref) and np.array_equal(v.astype(np.int8), v_ref)


@pytest.mark.parametrize("name", CHAN_CASES)
def test_chan_dims_against_metadata_and_rank_rule(name):
    from lrf_amd import _lib
    c = ChanCase(name)
    meta = c.metadata()
    _, H, W = c.image.shape
    Hp, Wp, M, N = _lib.chan_dims(H, W, c.C, c.patch_size)
    u_ref, v_ref = c.ref_factors()
    if c.patch_size is not None:
        p, q = c.patch_size
        assert meta["original size"] == [H, W] and meta["padded size"] == [Hp, Wp] and list(meta["patch size"]) == [p, q]
        assert (Hp % p, Wp % q) == (0, 0) and 0 <= Hp - H < p and 0 <= Wp - W < q
        assert (M, N) == ((Hp // p) * (Wp // q), c.C * p * q) and u_ref.shape == (M, c.R) and v_ref.shape == (N, c.R)
    else:
        assert (Hp, Wp, M, N) == (H, W, H, W) and u_ref.shape == (c.C, H, c.R) and v_ref.shape == (c.C, W, c.R)
    assert meta["color space"] == "RGB" and meta["rank"] == c.R
    if "quality" in c.kwargs:
        assert max(round(min(M, N) * c.kwargs["quality"] / 100), 1) == c.R == _lib.chan_rank(M, N, None, c.kwargs["quality"])
    assert _lib.chan_stream_geometry(meta, u_ref.shape, v_ref.shape) == (c.C, H, W, c.patch_size, c.R)


def test_chan_dims_values_and_refusals():
    from lrf_amd import _lib
    assert _lib.chan_dims(173, 264, 1, (8, 8)) == (176, 264, 726, 64)
    assert _lib.chan_dims(512, 768, 1, (8, 8)) == (512, 768, 6144, 64)
    assert _lib.chan_dims(37, 53, 5, (8, 4)) == (40, 56, 70, 160)
    assert _lib.chan_dims(37, 53, 4, None) == (37, 53, 37, 53)
    for C in (1, 3, 16):  # three channels: the numbers of lrf_rgbspace_dims_any
        assert _lib.chan_dims(61, 45, C, (4, 4))[:3] == _lib.rgbspace_dims_any(61, 45, (4, 4))[:3]
    for bad in [(0, 8, 1, (8, 8)), (8, 8, 0, (8, 8)), (8, 8, 17, (8, 8)), (3, 3, 1, (8, 8)), (8, 8, 1, (8, 0)), (8, 8, 1, (-8, -8))]:
        with pytest.raises(ValueError):
            _lib.chan_dims(*bad)


def test_header_walk_infers_channels_and_refuses_crafted_streams():
    from lrf_amd import _lib
    from lrf_amd.codec import _two_factor_parts
    from lrf_amd.container import combine_bytes, dict_to_bytes, encode_tensor
    c = ChanCase("chan_c2_q5")
    meta, u, v, geom = _two_factor_parts(c.encoded)
    assert geom == (2, 61, 45, (8, 8), c.R)
    g = ChanCase("chan_g_odd_q10")
    assert _two_factor_parts(g.encoded)[3] == (1, 37, 53, (8, 8), g.R)
    assert _two_factor_parts(ChanCase("chan_c4_nopatch_r3").encoded)[3] == (4, 37, 53, None, 3)
    gm, (gu, gv) = g.metadata(), g.ref_factors()

    def stream(m, a, b):
        return combine_bytes([dict_to_bytes(m), combine_bytes([encode_tensor(np.ascontiguousarray(a)), encode_tensor(np.ascontiguousarray(b))])])

    assert _two_factor_parts(stream(gm, gu, gv))[3] == (1, 37, 53, (8, 8), g.R)
    with pytest.raises(ValueError, match="not a multiple"):  # N not divisible by p q
        _two_factor_parts(stream(gm, gu, np.zeros((65, g.R), np.int8)))
    with pytest.raises(ValueError, match="geometry"):  # u against the padded size
        _two_factor_parts(stream(gm, gu[:-1], gv))
    with pytest.raises(ValueError, match="geometry"):  # padded size against the original size
        _two_factor_parts(stream(dict(gm, **{"padded size": [40, 64]}), gu, gv))
    with pytest.raises(ValueError, match="geometry"):  # rank against the factors
        _two_factor_parts(stream(dict(gm, rank=g.R + 1), gu, gv))
    with pytest.raises(ValueError):  # more channels than are served
        _two_factor_parts(stream(gm, gu, np.zeros((64 * 17, g.R), np.int8)))
    with pytest.raises(ValueError, match="int8"):
        _two_factor_parts(stream(gm, gu.astype(np.int16), gv))
    nm = ChanCase("chan_c4_nopatch_r3")
    nu, nv = nm.ref_factors()
    with pytest.raises(ValueError, match=r"\[C, H, R\]"):  # patch=False: u and v disagree on C
        _two_factor_parts(stream(nm.metadata(), nu, nv[:3]))
    assert _lib.chan_stream_geometry(nm.metadata(), nu.shape, nv.shape) == (4, 37, 53, None, 3)


def test_mixed_lists_are_refused_on_the_host():
    """a list that mixes gray and colour streams raises ValueError before anything reaches the device"""
    import lrf_amd
    gray = ChanCase("chan_g_odd_q10").encoded
    rgb = np.load(os.path.join(GOLDEN, "rgbsp_tiny_q4.npz"))["encoded"].tobytes()
    ycc = np.load(os.path.join(GOLDEN, "tiny_q7.npz"))["encoded"].tobytes()
    for streams in ([gray, rgb], [rgb, gray], [gray, ycc]):
        with pytest.raises(ValueError, match="mixes"):
            lrf_amd.qmf_decode_batch(streams)
    with pytest.raises(NotImplementedError, match="inflate"):
        lrf_amd.qmf_decode_batch([gray, gray], inflate="device")


def test_encode_refusals_name_what_is_missing():
    import lrf_amd
    img = torch.zeros((1, 16, 16), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="1"):
        lrf_amd.qmf_encode(img, rank=1)  # color_space="YCbCr" with one channel
    with pytest.raises(NotImplementedError, match="l2"):
        lrf_amd.qmf_encode(img, rank=1, color_space="RGB", l2=0.1)
    with pytest.raises(NotImplementedError, match="eps"):
        lrf_amd.qmf_encode(torch.zeros((4, 16, 16), dtype=torch.uint8), rank=1, color_space="RGB", eps=1e-8)
    batch = torch.zeros((2, 1, 16, 16), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="deflate"):
        lrf_amd.qmf_encode_batch(batch, rank=1, color_space="RGB", deflate="device")
    with pytest.raises(NotImplementedError, match="8x8"):
        lrf_amd.qmf_encode_batch(batch, rank=1, color_space="RGB", patch_size=(4, 4))
    with pytest.raises(NotImplementedError, match="8x8"):
        lrf_amd.qmf_encode_batch(batch, rank=1, color_space="RGB", patch=False)
    with pytest.raises(NotImplementedError, match="gray"):
        lrf_amd.qmf_encode_batch(torch.zeros((2, 3, 16, 16), dtype=torch.uint8), rank=1, color_space="RGB")
