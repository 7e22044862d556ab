"""GPU suite (-m gpu): qmf_encode_target and qmf_encode_budget on a LIST of images of differing sizes, against the same functions
called on every image alone as a batch of one (tests/test_encode_target_gpu.py and tests/test_encode_budget_gpu.py pin those) and
against qmf_encode_batch's streams.  Bytes, tables and choices are compared for equality."""
import numpy as np
import pytest
import torch

import _ragged_sweep_worker as W

pytestmark = pytest.mark.gpu
SIZES = W.SIZES + [W.SIZES[2], W.SIZES[0]]  # six images of four sizes
QUALITIES = (3, 6, 12, 25, 45)
# The images are small and noisy (15 to 25 dB over these qualities; streams of 700 to 3600 bytes, mostly container overhead): the
# goals below are set inside those ranges so that the images choose different qualities.  Image 4's PSNR is not monotonic in quality.
TARGETS = [17.0, 21.0, 15.0, 20.0, 99.0, 17.3]  # per image: reached at a low, the highest, the lowest quality; 99 dB: never
NEVER = 4
BPP = [3.0, 5.0, 0.01, 7.5, 4.2, 1.95]          # per image, of its own size; 0.01 bpp: nothing fits
NOTHING_FITS = 2


class Made:
    """the images and, per image, what the uniform functions return for it alone: made once, left unchanged"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            import lrf_amd
            imgs = [W.content(40 + j, H, Wd) for j, (H, Wd) in enumerate(SIZES)]
            target = [lrf_amd.qmf_encode_target(im[None], t, qualities=QUALITIES) for im, t in zip(imgs, TARGETS)]
            budget = [lrf_amd.qmf_encode_budget(im[None], bpp=b, qualities=QUALITIES) for im, b in zip(imgs, BPP)]
            cls._made = (imgs, target, budget)
        return cls._made


def _same_as_alone(out, alone, keys):
    for i, a in enumerate(alone):
        assert out["streams"][i] == a["streams"][0], i
        assert out["quality"][i] == a["quality"][0], i
        for k in keys:
            assert torch.equal(out[k][..., i], a[k][..., 0]), (k, i, out[k][..., i], a[k][..., 0])


def test_target_per_image_equals_the_uniform_function_image_by_image():
    import lrf_amd
    imgs, target, _ = Made.get()
    out = lrf_amd.qmf_encode_target(imgs, TARGETS, qualities=QUALITIES)
    assert set(out) == set(target[0]) and tuple(out["table"].shape) == (len(QUALITIES), len(imgs))
    _same_as_alone(out, target, ("table", "psnr", "reached"))
    for i, im in enumerate(imgs):
        assert out["streams"][i] == lrf_amd.qmf_encode_batch(im[None], quality=out["quality"][i])[0], i
    assert out["reached"].tolist() == [a["reached"][0].item() for a in target] and not out["reached"][NEVER] and out["reached"].sum() == 5
    # the fallback of a target nothing reaches: the candidate of the highest PSNR
    assert out["psnr"][NEVER] == out["table"][:, NEVER].max() and out["quality"][NEVER] == sorted(QUALITIES)[int(out["table"][:, NEVER].argmax())]
    assert len(set(out["quality"])) >= 3  # the images choose different qualities


def test_target_one_number_device_images_and_device_deflate():
    import lrf_amd
    imgs, _, _ = Made.get()
    one = lrf_amd.qmf_encode_target(imgs, 17.0, qualities=QUALITIES)
    per = lrf_amd.qmf_encode_target(imgs, [17.0] * len(imgs), qualities=QUALITIES)
    assert one["streams"] == per["streams"] and torch.equal(one["table"], per["table"])
    cuda = lrf_amd.qmf_encode_target([im.cuda() for im in imgs], 17.0, qualities=QUALITIES)
    assert cuda["streams"] == one["streams"] and cuda["quality"] == one["quality"] and torch.equal(cuda["table"], one["table"])
    dev = lrf_amd.qmf_encode_target(imgs, 17.0, qualities=QUALITIES, deflate="device")
    assert dev["quality"] == one["quality"]
    for i, im in enumerate(imgs):
        assert dev["streams"][i] == lrf_amd.qmf_encode_batch(im[None], quality=dev["quality"][i], deflate="device")[0], i
    shuffled = lrf_amd.qmf_encode_target(imgs, 17.0, qualities=QUALITIES[::-1])  # rows follow `qualities` as given
    assert torch.equal(shuffled["table"], one["table"].flip(0)) and shuffled["streams"] == one["streams"]


def test_budget_per_image_equals_the_uniform_function_image_by_image():
    import lrf_amd
    imgs, _, budget = Made.get()
    out = lrf_amd.qmf_encode_budget(imgs, bpp=BPP, qualities=QUALITIES)
    assert set(out) == set(budget[0]) and tuple(out["size_table"].shape) == (len(QUALITIES), len(imgs))
    _same_as_alone(out, budget, ("table", "size_table", "psnr", "reached", "nbytes", "bpp"))
    for i, im in enumerate(imgs):
        assert out["streams"][i] == lrf_amd.qmf_encode_batch(im[None], quality=out["quality"][i], deflate="device")[0], i
        assert len(out["streams"][i]) == int(out["nbytes"][i])
    assert not out["reached"][NOTHING_FITS] and out["reached"].sum() == 5 and len(set(out["quality"])) >= 3
    # the fallback of a budget nothing fits: the smallest stream
    assert int(out["nbytes"][NOTHING_FITS]) == int(out["size_table"][:, NOTHING_FITS].min())
    limit = [int(np.floor(b * H * Wd / 8)) for b, (H, Wd) in zip(BPP, SIZES)]  # bpp with each image's own size
    assert all(int(n) <= lim for n, lim, ok in zip(out["nbytes"], limit, out["reached"]) if ok)
    nb = lrf_amd.qmf_encode_budget(imgs, nbytes=limit, qualities=QUALITIES)
    assert nb["streams"] == out["streams"] and nb["quality"] == out["quality"]
    one = lrf_amd.qmf_encode_budget(imgs, nbytes=1000, qualities=QUALITIES)
    for i, im in enumerate(imgs):
        a = lrf_amd.qmf_encode_budget(im[None], nbytes=1000, qualities=QUALITIES)
        assert one["streams"][i] == a["streams"][0] and bool(one["reached"][i]) == bool(a["reached"][0])


def test_a_list_of_equal_sizes_returns_what_the_tensor_call_returns():
    import lrf_amd
    batch = torch.stack([W.content(60 + j, 40, 56) for j in range(4)])
    for fn, kw in ((lrf_amd.qmf_encode_target, dict(psnr=[17.0, 21.0, 99.0, 16.0])), (lrf_amd.qmf_encode_budget, dict(bpp=[3.0, 0.01, 6.0, 2.7]))):
        t = fn(batch, qualities=QUALITIES, **kw)
        l = fn(list(batch), qualities=QUALITIES, **kw)
        assert set(t) == set(l) and t["streams"] == l["streams"] and t["quality"] == l["quality"]
        for k in set(t) - {"streams", "quality"}:
            assert torch.equal(t[k], l[k]) and t[k].dtype == l[k].dtype, (k, t[k], l[k])
        assert 1 <= int(t["reached"].sum()) < 4 and len(set(t["quality"])) >= 3


def test_three_chunks_return_identical_streams():
    import lrf_amd
    from lrf_amd import _lib
    imgs, target, budget = Made.get()
    x_bytes = [4 * 64 * sum(d[4] for d in _lib.plane_dims(H, Wd)) for H, Wd in SIZES]
    limit = x_bytes[0] + x_bytes[1] + x_bytes[2]  # consecutive images as long as they fit: 0-2, 3-4, 5 — worked out below
    chunks, tot = 1, 0
    for b in x_bytes:
        if tot and tot + b > limit:
            chunks, tot = chunks + 1, 0
        tot += b
    assert chunks == 3
    whole = lrf_amd.qmf_encode_target(imgs, TARGETS, qualities=QUALITIES)
    parts = lrf_amd.qmf_encode_target(imgs, TARGETS, qualities=QUALITIES, x_workspace_bytes=limit)
    assert parts["streams"] == whole["streams"] and parts["quality"] == whole["quality"]
    assert all(torch.equal(parts[k], whole[k]) for k in ("table", "psnr", "reached"))
    tiny = lrf_amd.qmf_encode_target(imgs, TARGETS, qualities=QUALITIES, x_workspace_bytes=1)  # one image per chunk
    assert tiny["streams"] == whole["streams"] and torch.equal(tiny["table"], whole["table"])
    whole = lrf_amd.qmf_encode_budget(imgs, bpp=BPP, qualities=QUALITIES)
    parts = lrf_amd.qmf_encode_budget(imgs, bpp=BPP, qualities=QUALITIES, x_workspace_bytes=limit)
    assert parts["streams"] == whole["streams"] and parts["quality"] == whole["quality"]
    assert all(torch.equal(parts[k], whole[k]) for k in ("table", "size_table", "psnr", "reached", "nbytes", "bpp"))


def test_stream_sizes_ragged_equals_the_length_of_every_candidates_stream():
    import lrf_amd
    from lrf_amd import _lib
    from lrf_amd.codec import streams_from_device_factors
    ctx = _lib.context(0)
    imgs = [W.content(j, H, Wd) for j, (H, Wd) in enumerate(W.SIZES)]
    pairs = W.interleaved(W.CANDS)
    flat, offs = W.flat_of(imgs)
    U, V, u_off, v_off = ctx.encode_ragged_sweep(flat, [(H, Wd, o) for (H, Wd), o in zip(W.SIZES, offs)], [(i, list(t)) for i, t in pairs], 10, -16, 15)
    sizes, triples = [W.SIZES[i] for i, _ in pairs], [list(t) for _, t in pairs]
    got = lrf_amd.qmf_stream_sizes_ragged(U, V, sizes, triples, u_off, v_off, (-16, 15))
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (len(pairs),)
    streams = streams_from_device_factors(ctx, U, V, sizes, triples, u_off, v_off, (-16, 15))
    assert got.tolist() == [len(s) for s in streams]
    assert len({len(s) for s in streams}) > 1
