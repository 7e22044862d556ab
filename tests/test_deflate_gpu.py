"""GPU suite: lrf_deflate_columns_i8 gives the host restatement's bytes, column by column, and the encoders' deflate="device"
streams carry the default path's factors."""
import zlib

import numpy as np
import pytest
import torch

import deflate_cases as dc
from conftest import Case, config3_image

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def mixed():
    """one source buffer holding a matrix per ((rows, content), cols): back to back, so that the matrices start at every
    alignment; column j of a matrix is the content drawn with seed j -> (src, [(src_off, rows, cols)], expected stream per column)"""
    mats, parts, expected, at = [], [], [], 0
    for rows, content in dc.pairs():
        for cols in (1, 3, 7, 32, 33):
            if rows >= 65535 and cols > 3:
                continue
            m = np.stack([dc.column(content, rows, seed=j) for j in range(cols)], axis=1)
            mats.append((at, rows, cols))
            parts.append(m.reshape(-1))
            expected += [dc.host_stream(np.ascontiguousarray(m[:, j])) for j in range(cols)]
            at += m.size
    return np.concatenate(parts), mats, expected


def test_device_bytes_equal_the_host_restatement(mixed):
    from lrf_amd import _lib
    src, mats, expected = mixed
    ctx = _lib.context()
    table, nbytes, ncols = _lib.deflate_table(mats)
    assert ncols == len(expected)
    src_d = torch.from_numpy(src).cuda()
    slots = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.full((ncols,), -1, dtype=torch.int32, device="cuda")
    ctx.deflate_columns_into(src_d, table, slots, lens)
    first, first_len = (t.numpy() for t in ctx.to_host(slots, lens))
    ctx.deflate_columns_into(src_d, table, slots, lens)  # (staging memory that was never zeroed would show here)
    second, second_len = (t.numpy() for t in ctx.to_host(slots, lens))
    want = np.full(nbytes + GUARD, 0xA5, dtype=np.uint8)  # every byte of every slot: the stream, then 0xA5 to the slot's end; then the guard
    offs = _lib.deflate_column_offsets(table)
    for o, s in zip(offs, expected):
        want[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    want_len = np.array([len(s) for s in expected], dtype=np.int32)
    assert np.array_equal(first_len, want_len), np.flatnonzero(first_len != want_len)[:8]
    bad = np.flatnonzero(first != want)
    assert bad.size == 0, f"first differing byte {bad[0]}: column {np.searchsorted(offs, bad[0], side='right') - 1}"
    assert np.array_equal(second_len, want_len) and np.array_equal(second, want)
    k = 0
    for at, rows, cols in mats:  # and every stream inflates to its column
        m = src[at:at + rows * cols].reshape(rows, cols)
        for j in range(cols):
            assert zlib.decompress(first[offs[k]:offs[k] + first_len[k]].tobytes()) == np.ascontiguousarray(m[:, j]).tobytes()
            k += 1


def test_argument_checks_launch_nothing():
    from lrf_amd import _lib
    ctx = _lib.context()
    src = torch.zeros((64 * 3,), dtype=torch.int8, device="cuda")
    need = 3 * dc.bound(64)
    slots = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    lens = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    good = np.array([[0, 64, 3, 0, 0]], dtype=np.int64)
    for table, sl in ((good, slots[:need - 1]),                       # a slot range past dst_len
                      (np.array([[0, 0, 3, 0, 0]], dtype=np.int64), slots),   # rows < 1
                      (np.zeros((0, 5), dtype=np.int64), slots),            # n < 1
                      (np.array([[1, 64, 3, 0, 0]], dtype=np.int64), slots),  # the matrix leaves src
                      (np.array([[0, 64, 3, 0, 4]], dtype=np.int64), slots),  # its lengths leave out_len
                      (np.array([[0, 32, 3, 0, 0], [96, 32, 3, 40, 3]], dtype=np.int64), slots)):  # overlapping slots
        with pytest.raises(ValueError):
            ctx.deflate_columns_into(src, table, sl, lens)
    torch.cuda.synchronize()
    assert bool((slots == 0xA5).all()) and bool((lens == -1).all())
    assert _lib.load().lrf_deflate_bound(0) == -1 and _lib.load().lrf_deflate_bound(65536) == dc.bound(65536)
    ctx.deflate_columns_into(src, good, slots, lens)  # the good table does run
    assert ctx.to_host(lens)[0].tolist() == [len(dc.host_stream(np.zeros(64, dtype=np.int8)))] * 3 + [-1] * 3


def same_factors(device_streams, default_streams):
    from lrf_amd.codec import parse_stream
    assert len(device_streams) == len(default_streams)
    for a, b in zip(device_streams, default_streams):
        (ma, fa), (mb, fb) = parse_stream(a), parse_stream(b)
        assert ma == mb and len(fa) == len(fb) == 6
        for x, y in zip(fa, fb):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def batch_inputs():
    nat = Case("nat_q7").image
    crops = torch.stack([nat[:, y:y + 64, x:x + 96] for y, x in ((0, 0), (100, 40), (17, 333), (300, 500))]).contiguous()
    return [("tiny_q7", Case("tiny_q7").image[None], {"quality": 7}), ("odd_q7", Case("odd_q7").image[None], {"quality": 7}),
            ("zero_q7", Case("zero_q7").image[None], {"quality": 7}), ("crops_q7", crops, {"quality": 7}), ("crops_q20", crops, {"quality": 20}),
            ("big_r26", config3_image(0)[None], {"rank": [26, 13, 13]})]


@pytest.mark.parametrize("name", [b[0] for b in batch_inputs()])
def test_encode_batch_device_deflate(name):
    import lrf_amd
    _, images, kw = next(b for b in batch_inputs() if b[0] == name)
    for imgs in (images, images.cuda()) if name == "crops_q7" else (images,):  # (a host tensor takes the context path too)
        dev = lrf_amd.qmf_encode_batch(imgs, deflate="device", **kw)
        ref = lrf_amd.qmf_encode_batch(imgs, **kw)
        assert ref == lrf_amd.qmf_encode_batch(imgs, deflate="host", **kw)
        same_factors(dev, ref)
        assert torch.equal(lrf_amd.qmf_decode_batch(dev).cpu(), lrf_amd.qmf_decode_batch(ref).cpu())
    assert torch.equal(lrf_amd.qmf_decode(dev[0]), lrf_amd.qmf_decode(ref[0]))


def test_encode_ragged_device_deflate():
    import lrf_amd
    img = Case("nat_q7").image
    images = [img, img[:, :173, :264].contiguous(), img[:, 40:48, 80:88].contiguous()]
    dev = lrf_amd.qmf_encode_ragged(images, quality=[7, 12, 30], deflate="device")
    ref = lrf_amd.qmf_encode_ragged(images, quality=[7, 12, 30])
    same_factors(dev, ref)
    for a, b in zip(lrf_amd.qmf_decode_ragged(dev), lrf_amd.qmf_decode_ragged(ref)):
        assert torch.equal(a.cpu(), b.cpu())


def test_encode_target_device_deflate():
    import lrf_amd
    nat = Case("nat_q7").image
    batch = torch.stack([nat[:, y:y + 64, x:x + 96] for y, x in ((0, 0), (100, 40), (17, 333), (300, 500))]).contiguous()
    dev = lrf_amd.qmf_encode_target(batch, 32.0, deflate="device")
    ref = lrf_amd.qmf_encode_target(batch, 32.0)
    assert dev["quality"] == ref["quality"]
    for key in ("psnr", "reached", "table"):
        assert torch.equal(dev[key], ref[key]), key
    same_factors(dev["streams"], ref["streams"])
