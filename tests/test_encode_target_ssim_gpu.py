"""GPU suite (-m gpu): qmf_encode_target(ssim=...) against a brute force built from public functions that existed before it —
per image and quality qmf_encode_batch(img[None], quality=q) -> qmf_decode -> ssim_batch / psnr_batch, then the selection rule
in plain Python.  Streams (byte for byte), chosen qualities, reached flags, the SSIM and both tables must be EQUAL.

Three images of 48x64, 33x47 and 64x80 (a 16-aligned, an odd and a strip-body size), smooth content plus noise so that the SSIM
spans the grid.  The targets come from the brute-force table: image 0 between its third and fourth candidate (reached inside
the grid), image 1 between its last two (reached only at the top), image 2 above its best (never reached)."""
import pytest
import torch

from conftest import make_image

pytestmark = pytest.mark.gpu
SIZES = [(48, 64), (33, 47), (64, 80)]
QUALITIES = (2, 8, 14, 20, 26, 32)


class Brute:
    """images, per (quality, image) the stream, the SSIM and the PSNR, and the targets: made once, left unchanged"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            import lrf_amd
            g = torch.Generator().manual_seed(21)
            images = []
            for i, (H, W) in enumerate(SIZES):
                smooth = make_image(dict(kind="smooth", seed=500 + i, H=H, W=W)).to(torch.int16)
                images.append((smooth + torch.randint(-12, 13, smooth.shape, generator=g, dtype=torch.int16)).clamp(0, 255).to(torch.uint8))
            streams = [[lrf_amd.qmf_encode_batch(im[None], quality=q)[0] for im in images] for q in QUALITIES]
            decoded = [[lrf_amd.qmf_decode(s) for s in row] for row in streams]
            ssim = torch.stack([torch.cat([lrf_amd.ssim_batch(im, d).cpu() for im, d in zip(images, row)]) for row in decoded])
            psnr = torch.stack([torch.cat([lrf_amd.psnr_batch(im, d).cpu() for im, d in zip(images, row)]) for row in decoded])
            col = lambda b: ssim[:, b].tolist()
            target = [(max(col(0)[:3]) + col(0)[3]) / 2, (max(col(1)[:-1]) + col(1)[-1]) / 2, (max(col(2)) + 1.0) / 2]
            print("brute-force ssim table", ssim.tolist(), "targets", target)
            cls._made = (images, streams, decoded, ssim, psnr, target)
        return cls._made


def rule(ssim, psnr, target):
    """select_target_ssim's rule written out: -> (index, reached) per image"""
    index, reached = [], []
    for b in range(ssim.shape[1]):
        col = ssim[:, b].tolist()
        hit = [q for q, v in enumerate(col) if v == v and v >= target[b]]
        reached.append(bool(hit))
        if hit:
            index.append(hit[0])
        elif any(v == v for v in col):
            best = max(v for v in col if v == v)
            index.append([q for q, v in enumerate(col) if v == best][0])
        else:
            best = max(psnr[:, b].tolist())
            index.append([q for q, v in enumerate(psnr[:, b].tolist()) if v == best][0])
    return index, reached


def check(out, index, reached):
    images, streams, decoded, ssim, psnr, target = Brute.get()
    assert out["quality"] == [QUALITIES[i] for i in index]
    assert out["reached"].tolist() == reached
    assert out["ssim_table"].dtype == torch.float64 and torch.equal(out["ssim_table"], ssim)
    assert torch.equal(out["table"], psnr)
    assert torch.equal(out["ssim"], torch.stack([ssim[i, b] for b, i in enumerate(index)]))
    assert torch.equal(out["psnr"], torch.stack([psnr[i, b] for b, i in enumerate(index)]))


def test_the_targets_meet_the_three_situations():
    images, streams, decoded, ssim, psnr, target = Brute.get()
    index, reached = rule(ssim, psnr, target)
    assert reached == [True, True, False]
    assert 0 < index[0] < len(QUALITIES) - 1 and index[1] == len(QUALITIES) - 1
    assert bool(torch.isfinite(ssim).all()) and len({tuple(row) for row in ssim.tolist()}) == len(QUALITIES)  # the SSIM spans the grid


def test_list_equals_the_brute_force():
    import lrf_amd
    images, streams, decoded, ssim, psnr, target = Brute.get()
    index, reached = rule(ssim, psnr, target)
    out = lrf_amd.qmf_encode_target(images, ssim=target, qualities=QUALITIES)
    assert set(out) == {"streams", "quality", "psnr", "reached", "table", "ssim", "ssim_table"}
    check(out, index, reached)
    assert out["streams"] == [streams[i][b] for b, i in enumerate(index)]  # byte for byte


def test_one_target_for_all_and_device_images():
    import lrf_amd
    images, streams, decoded, ssim, psnr, target = Brute.get()
    one = [target[0]] * 3
    index, reached = rule(ssim, psnr, one)
    out = lrf_amd.qmf_encode_target([im.cuda() for im in images], ssim=target[0], qualities=QUALITIES)
    check(out, index, reached)
    assert out["streams"] == [streams[i][b] for b, i in enumerate(index)]
    shuffled = (20, 2, 32, 8, 26, 14)  # the tables follow the order of `qualities`
    out = lrf_amd.qmf_encode_target(images, ssim=target, qualities=shuffled)
    rows = [QUALITIES.index(q) for q in shuffled]
    assert torch.equal(out["ssim_table"], ssim[rows]) and torch.equal(out["table"], psnr[rows])
    assert out["quality"] == [QUALITIES[i] for i in rule(ssim, psnr, target)[0]]


def test_tensor_form_goes_the_way_of_the_list():
    import lrf_amd
    images, *_ = Brute.get()
    batch = torch.stack([images[0], images[0].flip(2), images[0].flip(1)])
    tgt = [0.5, 0.9, 2.0]
    a = lrf_amd.qmf_encode_target(batch, ssim=tgt, qualities=QUALITIES)
    b = lrf_amd.qmf_encode_target(list(batch), ssim=tgt, qualities=QUALITIES)
    assert a["streams"] == b["streams"] and a["quality"] == b["quality"]
    for k in ("psnr", "reached", "table", "ssim", "ssim_table"):
        assert torch.equal(a[k], b[k]), k
    assert a["reached"].tolist()[2] is False and a["ssim"][2] == a["ssim_table"][:, 2].max()
    for i, s in enumerate(a["streams"]):
        assert s == lrf_amd.qmf_encode_batch(batch[i][None], quality=a["quality"][i])[0]
    p = lrf_amd.qmf_encode_target(batch, 30.0, qualities=QUALITIES)  # psnr keeps its position and its keys
    assert set(p) == {"streams", "quality", "psnr", "reached", "table"} and torch.equal(p["table"], a["table"])


def test_device_deflate_decodes_to_the_same_pixels():
    import lrf_amd
    images, streams, decoded, ssim, psnr, target = Brute.get()
    index, reached = rule(ssim, psnr, target)
    out = lrf_amd.qmf_encode_target(images, ssim=target, qualities=QUALITIES, deflate="device")
    check(out, index, reached)
    for b, i in enumerate(index):
        assert torch.equal(lrf_amd.qmf_decode(out["streams"][b]), decoded[i][b])


def test_a_constant_image_takes_the_highest_psnr():
    import lrf_amd
    images, *_ = Brute.get()
    const = torch.full((3, 40, 56), 131, dtype=torch.uint8)
    out = lrf_amd.qmf_encode_target([const, images[1]], ssim=0.5, qualities=QUALITIES)
    assert bool(torch.isnan(out["ssim_table"][:, 0]).all()) and not out["reached"][0] and torch.isnan(out["ssim"][0])
    best = out["table"][:, 0].max()
    assert out["psnr"][0] == best and out["quality"][0] == QUALITIES[out["table"][:, 0].tolist().index(best.item())]
    assert out["streams"][0] == lrf_amd.qmf_encode_batch(const[None], quality=out["quality"][0])[0]
