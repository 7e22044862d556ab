"""eval_compression — the reference's per-image evaluation protocol (lrf/utils/misc.py:59-121) for this path:
one encode call and one decode call, wall-clock milliseconds each, then compression ratio, bpp, PSNR and SSIM
(metrics.ssim restates scikit-image's algorithm; scikit-image itself is absent from this image)."""
import time
from typing import Callable

import numpy as np
import torch

from .metrics import bits_per_pixel, compression_ratio, get_memory_usage, psnr, ssim


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def eval_compression(image, encoder: Callable, decoder: Callable, reconstruct: bool = False, **kwargs) -> dict:
    if isinstance(image, np.ndarray):
        image = torch.tensor(image.transpose((2, 0, 1)))  # HWC -> CHW, as the reference does
    elif not isinstance(image, torch.Tensor):
        raise ValueError("Image must be a file path, numpy array, or torch tensor.")
    _sync()
    t0 = time.perf_counter()
    encoded = encoder(image, **kwargs)
    _sync()
    encoding_time = 1000 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    reconstructed = decoder(encoded)
    _sync()
    decoding_time = 1000 * (time.perf_counter() - t0)
    output = {
        "compression ratio": compression_ratio(image, encoded),
        "bit rate (bpp)": bits_per_pixel(image.shape[-2:], encoded),
        "PSNR (dB)": psnr(image, reconstructed).item(),
        "SSIM": ssim(image, reconstructed).item(),
        "SSIM pinned to scikit-image": False,  # (metrics.ssim: a restatement; scikit-image is absent)
        "encoding time (ms)": encoding_time,
        "decoding time (ms)": decoding_time,
    }
    if reconstruct:
        output["reconstructed"] = reconstructed
    return output


def rd_sweep(images, qualities, encoder: Callable, decoder: Callable, **kwargs) -> list:
    """The loop of experiments/comparison/eval.py:83-110 for one method: every image at every quality."""
    records = []
    for idx, image in enumerate(images):
        for q in qualities:
            rec = eval_compression(image, encoder, decoder, quality=float(q), **kwargs)
            rec.update({"image": idx, "quality": float(q)})
            records.append(rec)
    return records


def rd_sweep_batched(images, qualities, fused: bool = True, metrics: str = "host", **kwargs) -> list:
    """The same sweep for `qmf_encode` / `qmf_decode` with all images of one size in ONE call per quality
    (`qmf_encode_batch` / `qmf_decode_batch`): images are independent, so every stream — hence bpp, PSNR, SSIM — is the one the
    per-image loop of `rd_sweep` produces (tests/test_harness_gpu.py); the times are the batch's, divided by the images.
    `fused` (round 5; default branch only — kwargs limited to bounds / num_iters): ALL qualities in one GPU call
    (`qmf_encode_sweep`: patch matrices, Gram matrices and the SVD initialisation once per image, the iterations of every
    (quality, image) pair in large launches); same streams again, the encoding time is the call's divided by qualities x images.
    `metrics`: "host" (default) scores every pair with `metrics.psnr` / `metrics.ssim` on the host, one image at a time, as
    `rd_sweep` does — the records are the per-image loop's exactly; "device" keeps the decoded batch on the GPU and scores it
    with ONE `image_metrics_batch` call per quality (the originals are uploaded once, [B] values come back per quality): PSNR in
    float64 from the exact squared error (the host's is float32) and SSIM to float64 rounding, plus "metrics time (ms)" (the
    call's, divided by the images).
    images: a uint8 tensor [B,3,H,W] or a sequence of [3,H,W] tensors of one size.  kwargs: qmf_encode's (bounds, num_iters,
    patch, patch_size ...) except quality / rank."""
    from .codec import qmf_decode_batch, qmf_encode_batch, qmf_encode_sweep
    from .metrics import image_metrics_batch
    if metrics not in ("host", "device"):
        raise ValueError(f'metrics must be "host" or "device", got {metrics!r}')
    stack = images if isinstance(images, torch.Tensor) and images.dim() == 4 else torch.stack(list(images))
    B = stack.shape[0]
    qualities = list(qualities)
    records = []
    all_streams, t_fused = None, 0.0
    stack_dev = None
    if fused and set(kwargs) <= {"bounds", "num_iters"} and stack.dtype == torch.uint8 and kwargs.get("num_iters", 10) >= 1:
        _sync()
        t0 = time.perf_counter()
        all_streams = qmf_encode_sweep(stack, qualities=[float(q) for q in qualities], **kwargs)
        _sync()
        t_fused = 1000 * (time.perf_counter() - t0) / (B * max(len(qualities), 1))
    for qi, q in enumerate(qualities):
        _sync()
        t0 = time.perf_counter()
        streams = all_streams[qi] if all_streams is not None else qmf_encode_batch(stack, quality=float(q), **kwargs)
        _sync()
        t_enc = t_fused if all_streams is not None else 1000 * (time.perf_counter() - t0) / B
        t0 = time.perf_counter()
        rec_dev = qmf_decode_batch(streams)
        if metrics == "device":
            _sync()
            t_dec = 1000 * (time.perf_counter() - t0) / B
            if stack_dev is None:
                stack_dev = stack.to(rec_dev.device)
                shape, nbytes = stack.shape[-2:], [get_memory_usage(stack[idx]) for idx in range(B)]
            t0 = time.perf_counter()
            m = image_metrics_batch(stack_dev, rec_dev)
            p_all, s_all = m["psnr"].cpu().tolist(), m["ssim"].cpu().tolist()  # (the copies wait for the kernels)
            t_met = 1000 * (time.perf_counter() - t0) / B
            for idx in range(B):
                records.append({
                    "compression ratio": nbytes[idx] / get_memory_usage(streams[idx]),
                    "bit rate (bpp)": bits_per_pixel(shape, streams[idx]),
                    "PSNR (dB)": p_all[idx],
                    "SSIM": s_all[idx],
                    "SSIM pinned to scikit-image": False,
                    "encoding time (ms)": t_enc,
                    "decoding time (ms)": t_dec,
                    "metrics time (ms)": t_met,
                    "image": idx,
                    "quality": float(q),
                })
            continue
        rec_all = rec_dev.cpu()
        _sync()
        t_dec = 1000 * (time.perf_counter() - t0) / B
        for idx in range(B):
            image, encoded, reconstructed = stack[idx].cpu(), streams[idx], rec_all[idx]
            records.append({
                "compression ratio": compression_ratio(image, encoded),
                "bit rate (bpp)": bits_per_pixel(image.shape[-2:], encoded),
                "PSNR (dB)": psnr(image, reconstructed).item(),
                "SSIM": ssim(image, reconstructed).item(),
                "SSIM pinned to scikit-image": False,
                "encoding time (ms)": t_enc,
                "decoding time (ms)": t_dec,
                "image": idx,
                "quality": float(q),
            })
    return records
