"""Image-compression metrics with the reference's definitions (lrf/utils/metrics.py)."""
import functools
from operator import mul

import numpy as np
import torch


def mse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return torch.mean((a - b) ** 2, dim=(-3, -2, -1))  # lrf/utils/metrics.py:24-35


def psnr(img1: torch.Tensor, img2: torch.Tensor, max_value: int = 255) -> torch.Tensor:
    # lrf/utils/metrics.py:57-71
    return 20 * torch.log10(max_value / torch.sqrt(mse(img1.float(), img2.float())))


def get_memory_usage(obj) -> int:
    # lrf/utils/metrics.py:94-117
    if isinstance(obj, (list, tuple, set)):
        return sum(get_memory_usage(o) for o in obj)
    if isinstance(obj, dict):
        return sum(get_memory_usage(o) for o in obj.values())
    if isinstance(obj, bytes):
        return len(obj)
    if isinstance(obj, np.ndarray):
        return obj.nbytes
    if isinstance(obj, torch.Tensor):
        return obj.numel() * obj.element_size()
    raise ValueError("Unsupported data type. Please provide an object containing NumPy arrays or PyTorch tensors.")


def compression_ratio(input, compressed) -> float:
    return get_memory_usage(input) / get_memory_usage(compressed)  # lrf/utils/metrics.py:120-133


def bits_per_pixel(size, compressed) -> float:
    # lrf/utils/metrics.py:149-162
    return get_memory_usage(compressed) * 8 / functools.reduce(mul, size, 1)


def ssim(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """Mean structural similarity of two (C, H, W) images, as lrf/utils/metrics.py:74-91 computes it.

    The reference delegates to scikit-image's `structural_similarity(img1, img2, channel_axis=0,
    data_range=img1.max() - img1.min())` (scikit-image is a dependency of the reference that is absent from this
    image, so this is a restatement of its published algorithm with the defaults that call selects — Wang et al.
    2004 with a 7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, `reflect` borders, the border of
    (win-1)/2 pixels cropped before averaging, per-channel means averaged).  Parity unpinned: there is no
    scikit-image here to check it against; tests/test_container_abi.py checks its defining properties only.
    """
    from scipy.ndimage import uniform_filter

    a = img1.detach().cpu().numpy()
    b = img2.detach().cpu().numpy()
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("Input images must have the same (C, H, W) shape.")
    win = 7
    if min(a.shape[1:]) < win:
        raise ValueError("win_size exceeds image extent.")
    data_range = float(a.max() - a.min())
    a = a.astype(np.float64, copy=False)
    b = b.astype(np.float64, copy=False)
    npix = win * win
    cov_norm = npix / (npix - 1.0)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    pad = (win - 1) // 2
    per_channel = []
    for x, y in zip(a, b):
        ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
        uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        per_channel.append(s[pad:-pad, pad:-pad].mean(dtype=np.float64))
    return torch.tensor(np.mean(per_channel))


def psnr_from_sse(sse: torch.Tensor, n, max_value: int = 255):
    """(mse, psnr) in float64 from exact integer squared errors over n samples each: mse = sse / n, psnr = 20 log10(max_value /
    sqrt(mse)), inf where sse is 0.  The ONE expression behind image_metrics_batch and qmf_encode_target, evaluated where `sse` lives.
    n: an integer, or an integer tensor [B] with one count per column of sse [..., B] (images of differing sizes).  The columns of
    each distinct count go through the integer form's own expression, so a column equals what the integer form gives for that
    count by construction, on any device (a list has few distinct sizes)."""
    if isinstance(n, torch.Tensor):
        counts = n.reshape(-1).cpu()
        if counts.numel() != sse.shape[-1]:
            raise ValueError(f"psnr_from_sse: {counts.numel()} counts for {sse.shape[-1]} columns")
        m = torch.empty(sse.shape, dtype=torch.float64, device=sse.device)
        for v in torch.unique(counts).tolist():
            cols = torch.nonzero(counts == v).reshape(-1).to(sse.device)
            m[..., cols] = sse[..., cols].double() / int(v)
    else:
        m = sse.double() / n
    return m, 20 * torch.log10(max_value / torch.sqrt(m))


def sweep_sse_batch(images: torch.Tensor, factors, triples, device=None) -> torch.Tensor:
    """The exact squared error of every (rank triple, image) pair of a sweep, straight from its int8 factors on the GPU
    (lrf_qmf_sweep_sse_rgb_u8, include/lrf_hip.h): no image is decoded to memory.

    images: uint8 [B,3,H,W] (a host tensor is uploaded); triples: Q rank triples; factors: one (U, V) pair of int8 CUDA tensors per
    triple, as `Context.encode_sweep_rgb` (or, for one triple, `qmf_factorize_batch`) returns them.  Returns an int64 device tensor
    [Q, B], equal to image_metrics_batch(images, decode of the factors)["sse"] per triple; psnr_from_sse turns it into PSNR."""
    from . import _lib
    _lib.check_sweep_sse_args(images, factors, triples)  # (before a context exists: these refusals need no GPU)
    if device is None:
        device = factors[0][0].device.index
    ctx = _lib.context(device)
    return ctx.sweep_sse(images.to(torch.device("cuda", ctx.device)).contiguous(), factors, [tuple(int(r) for r in t) for t in triples])


def image_metrics_batch(img1: torch.Tensor, img2: torch.Tensor, max_value: int = 255, want_ssim: bool = True, device=None) -> dict:
    """`mse`, `psnr` and `ssim` above for a whole batch of uint8 images on the GPU (lrf_image_metrics_u8, include/lrf_hip.h).

    img1, img2: uint8 [B,C,H,W] or one [C,H,W] pair; host tensors are uploaded.  Returns device tensors of shape [B]:
    "sse" int64 (the exact sum of squared differences), "mse" = sse / (C H W) and "psnr" = 20 log10(max_value / sqrt(mse))
    in float64 (inf where the images are equal, as `psnr` gives), "ssim" float64: the quantity `ssim(img1[i], img2[i])` defines
    (data_range from img1[i]; NaN where it gives NaN), absent with want_ssim=False.  The window sums are exact integers, so the
    results differ from the host functions by float64 rounding only (and by psnr's float32)."""
    from . import _lib
    if isinstance(img1, torch.Tensor) and isinstance(img2, torch.Tensor) and img1.dim() == 3 and img2.dim() == 3:
        img1, img2 = img1.unsqueeze(0), img2.unsqueeze(0)
    _lib.check_metrics_args(img1, img2, want_ssim)  # (before a context exists: these refusals need no GPU)
    if device is None and img1.is_cuda:
        device = img1.device.index
    if device is None and img2.is_cuda:
        device = img2.device.index
    ctx = _lib.context(device)
    dev = torch.device("cuda", ctx.device)
    a, b = img1.to(dev).contiguous(), img2.to(dev).contiguous()
    sse, s = ctx.image_metrics(a, b, want_ssim=want_ssim)
    m, p = psnr_from_sse(sse, a.shape[1] * a.shape[2] * a.shape[3], max_value)
    out = {"sse": sse, "mse": m, "psnr": p}
    if want_ssim:
        out["ssim"] = s
    return out


def psnr_batch(img1: torch.Tensor, img2: torch.Tensor, max_value: int = 255) -> torch.Tensor:
    """float64 device tensor [B]: `image_metrics_batch(...)["psnr"]` without the SSIM work"""
    return image_metrics_batch(img1, img2, max_value=max_value, want_ssim=False)["psnr"]


def ssim_batch(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """float64 device tensor [B]: `image_metrics_batch(...)["ssim"]`"""
    return image_metrics_batch(img1, img2)["ssim"]


def image_metrics_ragged(list_a, list_b, want_ssim: bool = True, max_value: int = 255, device=None) -> dict:
    """image_metrics_batch for pairs that differ in size, in one GPU call (lrf_image_metrics_ragged_u8, include/lrf_hip.h).

    list_a, list_b: two lists of uint8 [C,H_i,W_i] tensors, pair i of one shape, every pair of the same C, all on the host or
    all on one device (host tensors are uploaded).  Returns device tensors of shape [n] under image_metrics_batch's keys: "sse"
    int64, "mse" and "psnr" float64 over each pair's own C H_i W_i samples (psnr_from_sse with per-item counts), "ssim" float64
    (absent with want_ssim=False).  Entry i has the bits image_metrics_batch(list_a[i][None], list_b[i][None]) gives, NaN
    included, whatever the order of the lists.  Entries of list_a that are one tensor object are uploaded and scanned for their
    data range once."""
    from . import _lib
    C, sizes = _lib.check_metrics_ragged_args(list_a, list_b, want_ssim)  # (before a context exists: these refusals need no GPU)
    if device is None and list_a[0].is_cuda:
        device = list_a[0].device.index
    ctx = _lib.context(device)
    dev = torch.device("cuda", ctx.device)
    a_at, offs_a, offs_b, na, nb = {}, [], [], 0, 0
    for (H, W), x in zip(sizes, list_a):
        if id(x) not in a_at:
            a_at[id(x)] = na
            na = (na + C * H * W + 15) // 16 * 16
        offs_a.append(a_at[id(x)])
        offs_b.append(nb)
        nb = (nb + C * H * W + 15) // 16 * 16
    a, b = torch.empty((na,), dtype=torch.uint8, device=dev), torch.empty((nb,), dtype=torch.uint8, device=dev)
    done = set()
    for x, y, oa, ob in zip(list_a, list_b, offs_a, offs_b):
        if oa not in done:
            a[oa:oa + x.numel()].view(x.shape).copy_(x)
            done.add(oa)
        b[ob:ob + y.numel()].view(y.shape).copy_(y)
    pairs = np.array([(H, W, oa, ob) for (H, W), oa, ob in zip(sizes, offs_a, offs_b)], dtype=np.int64)
    sse, s = ctx.metrics_ragged(a, b, pairs, C, want_ssim=want_ssim)
    m, p = psnr_from_sse(sse, torch.tensor([C * H * W for H, W in sizes], dtype=torch.int64), max_value)
    out = {"sse": sse, "mse": m, "psnr": p}
    if want_ssim:
        out["ssim"] = s
    return out
