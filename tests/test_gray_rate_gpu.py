"""Gray image lists through the codec (-m gpu): qmf_encode_ragged, qmf_encode_target and qmf_encode_budget with color_space="RGB"
against brute-force loops over the per-image calls — encode per quality, qmf_decode, squared error, len — and the device coder's
two-factor containers against Python's zlib."""
import functools
import zlib

import numpy as np
import pytest
import torch

from lrf_amd.container import bytes_to_dict, separate_bytes
from test_channels_gpu import smooth

pytestmark = pytest.mark.gpu

SIZES = [(16, 24), (37, 53), (64, 96), (56, 440), (173, 264), (48, 400)]
QUALITIES = list(range(1, 33, 3))


@functools.lru_cache(maxsize=None)
def images():
    """one image per size, randint and smooth in turn, uint8 [1,H,W] host tensors; read-only: every test shares them"""
    out = []
    for k, (H, W) in enumerate(SIZES):
        rng = np.random.default_rng(H * 1000 + W + 1)
        out.append(torch.from_numpy(rng.integers(0, 256, (1, H, W), dtype=np.uint8) if k % 2 else smooth(rng, 1, H, W)))
    return tuple(out)


def inflate_factors(stream):
    """a two-factor container read with Python's zlib alone -> (metadata, u [M,R], v [64,R])"""
    meta, body = separate_bytes(stream, 2)
    factors = []
    for f in separate_bytes(body, 2):
        header, cols = separate_bytes(f, 2)
        h = bytes_to_dict(header)
        assert h["mode"] == "col" and h["dtype"] == "int8"
        factors.append(np.stack([np.frombuffer(zlib.decompress(c), dtype=np.int8) for c in separate_bytes(cols, h["num_fibers"])], axis=1))
    return bytes_to_dict(meta), factors[0], factors[1]


@functools.lru_cache(maxsize=None)
def brute():
    """per image and quality of QUALITIES, by the per-image calls: the zlib-9 stream, the device coder's stream, the exact squared
    error of qmf_decode against the source"""
    import lrf_amd
    host, device, sse = [], [], []
    for im in images():
        hs = [lrf_amd.qmf_encode_batch(im[None], quality=q, color_space="RGB")[0] for q in QUALITIES]
        ds = [lrf_amd.qmf_encode_ragged([im], quality=q, color_space="RGB", deflate="device")[0] for q in QUALITIES]
        host.append(hs)
        device.append(ds)
        sse.append([int(((lrf_amd.qmf_decode(s).long() - im.long()) ** 2).sum()) for s in hs])
    return host, device, sse


def psnr_table(sse):
    """[image][quality] squared errors -> float64 [Q, B] on the host: the one expression of the library per image's own sample
    count, evaluated where the calls evaluate it (on the device: its log10 and sqrt are not the host's to the last bit)"""
    from lrf_amd.metrics import psnr_from_sse
    cols = [psnr_from_sse(torch.tensor(s, dtype=torch.int64).cuda(), im.numel())[1] for s, im in zip(sse, images())]
    return torch.stack(cols, dim=1).cpu()


def test_encode_ragged_gray_equals_the_per_image_batch_calls():
    """ranks and qualities per image, signs for some, host and device images, a tensor [B,1,H,W]; a rank above 32 in the list"""
    import lrf_amd
    ims = list(images())
    ranks = [1, 7, 9, 17, 32, 40]
    signs = [None if i % 2 else np.random.default_rng(i).choice(np.array([-1, 1], dtype=np.int8), size=r) for i, r in enumerate(ranks)]
    want = [lrf_amd.qmf_encode_batch(im[None], rank=r, color_space="RGB", init_sign=sg)[0] for im, r, sg in zip(ims, ranks, signs)]
    assert lrf_amd.qmf_encode_ragged(ims, rank=ranks, init_sign=signs, color_space="RGB") == want
    assert lrf_amd.qmf_encode_ragged([im.cuda() for im in ims], rank=ranks, init_sign=signs, color_space="RGB", pack_workers=1) == want
    quals = [3, 10, 22, 31, 50, 5]
    want_q = [lrf_amd.qmf_encode_batch(im[None], quality=q, color_space="RGB", bounds=(-128, 127), num_iters=3)[0] for im, q in zip(ims, quals)]
    assert lrf_amd.qmf_encode_ragged(ims[::-1], quality=quals[::-1], color_space="RGB", bounds=(-128, 127), num_iters=3) == want_q[::-1]
    batch = torch.stack([ims[2], ims[2].flip(2), ims[2].flip(1)])
    assert lrf_amd.qmf_encode_ragged(batch, quality=12, color_space="RGB") == lrf_amd.qmf_encode_batch(batch, quality=12, color_space="RGB")
    for s, im in zip(want, ims):
        assert tuple(lrf_amd.qmf_decode(s).shape) == tuple(im.shape)  # (the streams parse)


def test_device_deflate_streams_hold_the_same_factors_and_sizes():
    """deflate="device": Python's zlib inflates every column to the factors of the zlib-9 stream, qmf_decode reads the stream,
    and qmf_stream_sizes_gray_ragged counts its length"""
    import lrf_amd
    from lrf_amd import _lib
    ims = list(images())
    ranks = [1, 2, 9, 10, 32, 40]
    host = lrf_amd.qmf_encode_ragged(ims, rank=ranks, color_space="RGB")
    dev = lrf_amd.qmf_encode_ragged(ims, rank=ranks, color_space="RGB", deflate="device")
    for h, d, im, R in zip(host, dev, ims, ranks):
        mh, uh, vh = inflate_factors(h)
        md, ud, vd = inflate_factors(d)
        assert mh == md and ud.shape == (uh.shape[0], R) and np.array_equal(uh, ud) and np.array_equal(vh, vd)
        assert torch.equal(lrf_amd.qmf_decode(d), lrf_amd.qmf_decode(h))
    # the sizes, counted from the factors alone (the ranks the ragged entry serves)
    ctx = _lib.context(0)
    flat = torch.cat([im.reshape(-1) for im in ims[:5]]).cuda()
    offs = np.cumsum([0] + [im.numel() for im in ims[:4]]).tolist()
    U, V, u_off, v_off = ctx.encode_gray_ragged(flat, [(im.shape[1], im.shape[2], R, o) for im, R, o in zip(ims, ranks, offs)], 10, -16, 15)
    sizes = lrf_amd.qmf_stream_sizes_gray_ragged(U, V, [tuple(im.shape[1:]) for im in ims[:5]], ranks[:5], u_off, v_off)
    assert sizes.dtype == torch.int64 and sizes.is_cuda and sizes.cpu().tolist() == [len(s) for s in dev[:5]]
    assert lrf_amd.gray_streams_from_device_factors(ctx, U, V, [tuple(im.shape[1:]) for im in ims[:5]], ranks[:5], u_off, v_off, (-16, 15)) == dev[:5]


def pick_target(table, target):
    """the first quality (ascending) whose PSNR reaches the target, else the first of the highest PSNR"""
    out = []
    for b in range(table.shape[1]):
        col = table[:, b].tolist()
        ok = [k for k, p in enumerate(col) if p >= target[b]]
        out.append((ok[0], True) if ok else (col.index(max(col)), False))
    return out


def pick_budget(size, sse, budget):
    """among the candidates that fit, the lowest squared error, then the smaller size, then the lowest quality; where none fits
    the smallest stream (the lowest quality of equal sizes)"""
    out = []
    for b in range(len(size)):
        fit = [k for k in range(len(QUALITIES)) if size[b][k] <= budget[b]]
        if fit:
            out.append((min(fit, key=lambda k: (sse[b][k], size[b][k], k)), True))
        else:
            out.append((min(range(len(QUALITIES)), key=lambda k: (size[b][k], k)), False))
    return out


def targets_of(table):
    """per image: a table value itself, a target nothing reaches, and values between two rows"""
    t = []
    for b in range(table.shape[1]):
        col = table[:, b]
        if b == 0:
            t.append(float(col[3]))  # exactly on a table value: >= holds
        elif b == 1:
            t.append(float(col.max()) + 1.0)  # not reached
        else:
            t.append(float((col[b] + col[b + 1]) / 2))
    return t


def test_target_equals_the_brute_force_loop():
    import lrf_amd
    ims = list(images())
    host, _, sse = brute()
    table = psnr_table(sse)
    target = targets_of(table)
    want = pick_target(table, target)
    assert [r for _, r in want].count(True) >= 1 and [r for _, r in want].count(False) >= 1
    out = lrf_amd.qmf_encode_target(ims, target, qualities=QUALITIES, color_space="RGB")
    assert sorted(out) == ["psnr", "quality", "reached", "streams", "table"]
    assert torch.equal(out["table"], table)
    assert out["quality"] == [QUALITIES[k] for k, _ in want] and out["reached"].tolist() == [r for _, r in want]
    assert out["streams"] == [host[b][k] for b, (k, _) in enumerate(want)]
    assert torch.equal(out["psnr"], torch.stack([table[k, b] for b, (k, _) in enumerate(want)]))
    for b, s in enumerate(out["streams"]):  # (and what psnr gives for the decode, in its float32)
        from lrf_amd.metrics import psnr
        assert abs(float(psnr(lrf_amd.qmf_decode(s), ims[b])) - float(out["psnr"][b])) < 1e-3
    # two chunks give the bytes of one; device images; a permuted quality grid keeps its rows
    small = lrf_amd.qmf_encode_target(ims, target, qualities=QUALITIES, color_space="RGB", x_workspace_bytes=4 * 64 * 400)
    assert small["streams"] == out["streams"] and torch.equal(small["table"], table) and small["quality"] == out["quality"]
    on_dev = lrf_amd.qmf_encode_target([im.cuda() for im in ims], target, qualities=QUALITIES[::-1], color_space="RGB")
    assert on_dev["streams"] == out["streams"] and torch.equal(on_dev["table"], table.flip(0))


def test_budget_equals_the_brute_force_loop():
    import lrf_amd
    from lrf_amd.metrics import bits_per_pixel
    ims = list(images())
    _, device, sse = brute()
    size = [[len(s) for s in row] for row in device]
    table = psnr_table(sse)
    # budgets from the table: exactly a stream's size, one byte below the smallest (nothing fits), between two sizes
    budget = []
    for b in range(len(ims)):
        if b == 0:
            budget.append(size[b][4])
        elif b == 1:
            budget.append(min(size[b]) - 1)
        else:
            budget.append((size[b][b] + size[b][b + 1]) // 2)
    want = pick_budget(size, sse, budget)
    assert [r for _, r in want].count(True) >= 1 and [r for _, r in want].count(False) == 1
    out = lrf_amd.qmf_encode_budget(ims, nbytes=budget, qualities=QUALITIES, color_space="RGB")
    assert sorted(out) == ["bpp", "nbytes", "psnr", "quality", "reached", "size_table", "streams", "table"]
    assert torch.equal(out["table"], table)
    assert torch.equal(out["size_table"], torch.tensor(size, dtype=torch.int64).T)
    # equal ranks share a stream: the loop's choice is named by the lowest quality of its rank, as the call names it
    chosen = [k for k, _ in want]
    assert out["streams"] == [device[b][k] for b, k in enumerate(chosen)]
    assert [len(s) for s in out["streams"]] == out["nbytes"].tolist()
    assert out["quality"] == [QUALITIES[next(j for j in range(len(QUALITIES)) if device[b][j] == device[b][k])] for b, k in enumerate(chosen)]
    assert out["reached"].tolist() == [r for _, r in want]
    assert out["bpp"].tolist() == [bits_per_pixel(tuple(im.shape[1:]), s) for im, s in zip(ims, out["streams"])]
    assert all(n <= bud for n, bud, (_, r) in zip(out["nbytes"].tolist(), budget, want) if r)
    # bits per pixel with each image's own size, two chunks
    bpp = lrf_amd.qmf_encode_budget(ims, bpp=1.5, qualities=QUALITIES, color_space="RGB", x_workspace_bytes=4 * 64 * 400)
    want_bpp = pick_budget(size, sse, [int(1.5 * im.shape[1] * im.shape[2] / 8) for im in ims])
    assert bpp["streams"] == [device[b][k] for b, (k, _) in enumerate(want_bpp)] and bpp["reached"].tolist() == [r for _, r in want_bpp]


def test_a_tensor_goes_the_way_of_the_list_of_its_images():
    import lrf_amd
    rng = np.random.default_rng(12)
    batch = torch.from_numpy(np.stack([smooth(rng, 1, 37, 53) for _ in range(3)]))
    t = lrf_amd.qmf_encode_target(batch, [28.0, 31.0, 60.0], qualities=QUALITIES, color_space="RGB")
    l = lrf_amd.qmf_encode_target(list(batch), [28.0, 31.0, 60.0], qualities=QUALITIES, color_space="RGB")
    assert t["streams"] == l["streams"] and t["quality"] == l["quality"] and torch.equal(t["table"], l["table"]) and torch.equal(t["reached"], l["reached"])
    for b, (s, q) in enumerate(zip(t["streams"], t["quality"])):
        assert s == lrf_amd.qmf_encode_batch(batch[b:b + 1], quality=q, color_space="RGB")[0]
    tb = lrf_amd.qmf_encode_budget(batch.cuda(), bpp=2.0, qualities=QUALITIES, color_space="RGB")
    lb = lrf_amd.qmf_encode_budget(list(batch), bpp=2.0, qualities=QUALITIES, color_space="RGB")
    assert tb["streams"] == lb["streams"] and torch.equal(tb["size_table"], lb["size_table"]) and tb["quality"] == lb["quality"]
    dev_t = lrf_amd.qmf_encode_target(batch, 30.0, qualities=QUALITIES, color_space="RGB", deflate="device")
    for b, (s, q) in enumerate(zip(dev_t["streams"], dev_t["quality"])):
        assert s == lrf_amd.qmf_encode_ragged([batch[b]], quality=q, color_space="RGB", deflate="device")[0]
