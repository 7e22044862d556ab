"""GPU suite: the decoders' inflate="device" path (the columns' zlib streams inflated by lrf_inflate_columns_i8) gives what the
default inflate="host" path gives, for the reference's zlib-9 streams and for deflate="device" streams."""
import numpy as np
import pytest
import torch

from conftest import Case, config3_image

pytestmark = pytest.mark.gpu


def batch_inputs():  # (the list of tests/test_deflate_gpu.py)
    nat = Case("nat_q7").image
    crops = torch.stack([nat[:, y:y + 64, x:x + 96] for y, x in ((0, 0), (100, 40), (17, 333), (300, 500))]).contiguous()
    return [("tiny_q7", Case("tiny_q7").image[None], {"quality": 7}), ("odd_q7", Case("odd_q7").image[None], {"quality": 7}),
            ("zero_q7", Case("zero_q7").image[None], {"quality": 7}), ("crops_q7", crops, {"quality": 7}), ("crops_q20", crops, {"quality": 20}),
            ("big_r26", config3_image(0)[None], {"rank": [26, 13, 13]})]


def ragged_images():
    img = Case("nat_q7").image
    return [img, img[:, :173, :264].contiguous(), img[:, 40:48, 80:88].contiguous()]


@pytest.fixture(scope="module")
def ragged_streams():
    import lrf_amd
    return {d: lrf_amd.qmf_encode_ragged(ragged_images(), quality=[7, 12, 30], deflate=d) for d in ("host", "device")}


@pytest.mark.parametrize("deflate", ["host", "device"])
@pytest.mark.parametrize("name", [b[0] for b in batch_inputs()])
def test_decode_batch(name, deflate):
    import lrf_amd
    _, images, kw = next(b for b in batch_inputs() if b[0] == name)
    s = lrf_amd.qmf_encode_batch(images, deflate=deflate, **kw)
    assert torch.equal(lrf_amd.qmf_decode_batch(s, inflate="device").cpu(), lrf_amd.qmf_decode_batch(s).cpu())


@pytest.mark.parametrize("deflate", ["host", "device"])
def test_decode_ragged(ragged_streams, deflate):
    import lrf_amd
    s = ragged_streams[deflate]
    got, want = lrf_amd.qmf_decode_ragged(s, inflate="device"), lrf_amd.qmf_decode_ragged(s, inflate="host")
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("deflate", ["host", "device"])
def test_resident_factors_and_crops(ragged_streams, deflate):
    import lrf_amd
    s = ragged_streams[deflate]
    dev, host = lrf_amd.qmf_load_factors(s, inflate="device"), lrf_amd.qmf_load_factors(s)
    assert dev.images == host.images and torch.equal(dev.U.cpu(), host.U.cpu()) and torch.equal(dev.V.cpu(), host.V.cpu())
    crops = [(0, 0, 0), (0, 100, 333), (1, 141, 232), (2, 0, 0), (1, 7, 9)]
    want = host.decode_crops(crops, (8, 8)).cpu()
    assert torch.equal(dev.decode_crops(crops, (8, 8)).cpu(), want)
    assert torch.equal(lrf_amd.qmf_decode_crops(s, crops, (8, 8), inflate="device").cpu(), want)
    assert torch.equal(lrf_amd.qmf_decode_crops(dev, crops, (8, 8), inflate="device").cpu(), want)


def default_branch_cases():
    """[(name, stream, sha256 of the reference's decoded pixels)]: the golden fixtures of the default branch (YCbCr, 8x8 patches,
    chroma (0.5, 0.5), uint8) with ranks <= 64; fixtures without a stream, or whose stream is no JSON-headed container, are
    other codecs' and are passed over"""
    import glob
    import json
    import os
    from conftest import GOLDEN
    from lrf_amd.codec import _ragged_branch
    from lrf_amd.container import bytes_to_dict, separate_bytes
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        z = np.load(path)
        if "encoded" not in z.files or "decoded_sha256" not in z.files:
            continue
        try:
            meta = bytes_to_dict(separate_bytes(z["encoded"].tobytes(), 2)[0])
        except (ValueError, UnicodeDecodeError, json.JSONDecodeError):  # another codec's container
            continue
        if not {"color space", "patch", "patch size", "original size", "padded size", "dtype", "rank"} <= set(meta):
            continue
        if _ragged_branch(meta) == "" and max(int(r) for r in meta["rank"]) <= 64:
            out.append((os.path.basename(path)[:-4], z["encoded"].tobytes(), str(z["decoded_sha256"])))
    return out


def test_reference_streams_decode_to_the_fixtures_pixels():
    import hashlib

    import lrf_amd
    cases = default_branch_cases()
    assert {"tiny_q7", "odd_q7", "zero_q7", "nat_q7"} <= {name for name, _, _ in cases} and len(cases) >= 20
    got = lrf_amd.qmf_decode_ragged([enc for _, enc, _ in cases], inflate="device")
    for (name, enc, sha), g in zip(cases, got):
        assert hashlib.sha256(g.cpu().numpy().tobytes()).hexdigest() == sha, name
        assert torch.equal(lrf_amd.qmf_decode_batch([enc], inflate="device")[0].cpu(), g.cpu())


def test_a_broken_stream_in_a_list_is_named(ragged_streams):
    import lrf_amd
    from lrf_amd.codec import index_columns_native
    from lrf_amd.container import separate_bytes
    s = list(ragged_streams["host"])
    meta, blob = (bytes(x) for x in separate_bytes(s[1], 2))
    ranks = [int(r) for r in lrf_amd.container.bytes_to_dict(meta)["rank"]]
    M = [d[4] for d in lrf_amd._lib.plane_dims(173, 264)]
    off, ln, rc = index_columns_native([blob], [M], [ranks])
    assert rc == 0
    at = s[1].index(blob) + int(off[2]) + int(ln[2]) // 2  # a bit in the middle of the third column's stream
    broken = bytearray(s[1])
    broken[at] ^= 0x10
    import zlib
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(broken[s[1].index(blob) + int(off[2]):][:int(ln[2])]))
    for call in (lrf_amd.qmf_decode_ragged, lrf_amd.qmf_load_factors):
        with pytest.raises(ValueError, match=r"stream 1: column 2 of factor u_Y"):
            call([s[0], bytes(broken), s[2]], inflate="device")
    for a, b in zip(lrf_amd.qmf_decode_ragged(s, inflate="device"), lrf_amd.qmf_decode_ragged(s)):  # a later good call works
        assert torch.equal(a.cpu(), b.cpu())


def test_keyword_checks(ragged_streams):
    import lrf_amd
    s = ragged_streams["host"]
    for call in (lrf_amd.qmf_decode_batch, lrf_amd.qmf_decode_ragged, lrf_amd.qmf_load_factors):
        with pytest.raises(ValueError, match="inflate"):
            call(s[:1], inflate="gpu")
    with pytest.raises(ValueError, match="inflate"):
        lrf_amd.qmf_decode_crops(s, [(0, 0, 0)], (8, 8), inflate="gpu")
    whole = lrf_amd.qmf_encode(ragged_images()[1], quality=7, patch=False)
    with pytest.raises(NotImplementedError):
        lrf_amd.qmf_decode_ragged([whole], inflate="device")
    assert torch.equal(lrf_amd.qmf_decode_batch([whole], inflate="device")[0].cpu(), lrf_amd.qmf_decode(whole).cpu())  # one by one, as today
