"""qmf_encode / qmf_decode with the reference's signatures (lrf/compression/qmf.py:116-353), running the
arithmetic on the MI355X.  Python keeps the byte container (JSON metadata + per-column zlib), exactly
as the reference does on the host."""
import functools
import math
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .container import (bytes_to_dict, combine_bytes, decode_tensor, dict_to_bytes, encode_tensor, separate_bytes)


def qmf_ranks(image_hw, rank=None, quality=None):
    """The (Y, Cb, Cr) ranks qmf_encode uses: lrf/compression/qmf.py:215-225, 244-250."""
    H, W = image_hw
    if not isinstance(rank, Iterable):
        rank = (None, None, None) if rank is None else (rank, max(rank // 2, 1), max(rank // 2, 1))
    if not isinstance(quality, Iterable):
        quality = (None, None, None) if quality is None else (quality, quality / 2, quality / 2)
    out = []
    for i, (_, _, _, _, M) in enumerate(_lib.plane_dims(H, W)):
        if rank[i] is None:
            assert quality[i] >= 0 and quality[i] <= 100, "'quality' must be between 0 and 100."
            out.append(max(round(min(M, 64) * quality[i] / 100), 1))
        else:
            out.append(rank[i])
    return out


def _check_hip_branch(color_space, scale_factor, patch, patch_size, bounds, dtype, kwargs):
    """Splits qmf_encode's **kwargs (lrf/compression/qmf.py:127, forwarded to QMF(...) at :189, 208, 256, 280) into the loop
    parameters of the tuned path and the options only the general solver takes (`qmf_opts`: l2, l1_ratio, eps, num_levels)."""
    if color_space == "YCbCr" and not (len(scale_factor) == 2 and min(scale_factor) > 0):
        raise ValueError("scale_factor must be two positive numbers")
    if dtype is not torch.int8:
        raise NotImplementedError("HIP path stores int8 factors only")
    num_iters = kwargs.pop("num_iters", 10)
    init_sign = kwargs.pop("init_sign", None)
    kwargs.pop("init", None)  # explicit (u0, v0) fp32 initial factors (tests)
    kwargs.pop("verbose", None)
    for dup in ("factor", "project"):  # the reference passes these itself: a caller's copy is a duplicate keyword there too
        if dup in kwargs:
            raise TypeError(f"QMF() got multiple values for keyword argument '{dup}'")
    qmf_opts = {}
    l2 = kwargs.pop("l2", 0)
    l2p = tuple(l2) if isinstance(l2, (tuple, list)) else (l2, l2)
    if any(v != 0 for v in l2p):
        qmf_opts["l2"] = l2
        qmf_opts["l1_ratio"] = kwargs.pop("l1_ratio", 0)
    else:
        kwargs.pop("l1_ratio", None)  # without an l2 weight the l1 share multiplies zero (qmf.py:154-157)
    eps = kwargs.pop("eps", 1e-16)
    if eps != 1e-16:
        qmf_opts["eps"] = eps
    num_levels = kwargs.pop("num_levels", None)
    if num_levels:
        qmf_opts["num_levels"] = num_levels
    if kwargs:
        raise TypeError(f"CoordinateDescent.__init__() got an unexpected keyword argument '{sorted(kwargs)[0]}'")
    if num_iters < 0:
        raise ValueError("num_iters must be >= 0")
    lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
    return num_iters, lo, hi, init_sign, qmf_opts


def qmf_factorize_batch(images: torch.Tensor, ranks: Sequence[int], num_iters: int = 10, bounds=(-16, 15),
                        init_sign=None, out=None):
    """GPU-only part of the encoder for a batch [B,3,H,W] of uint8 images already in HBM.

    Returns (U, V): int8 CUDA tensors [B, sum_c M_c R_c] and [B, 64 sum_c R_c] holding, per image, the factors of
    the Y, Cb, Cr planes back to back (row-major [M_c, R_c] / [64, R_c])."""
    assert images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[1] == 3
    ctx = _lib.context(images.device.index)
    sign = None
    if init_sign is not None:
        sign = torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1, sum(ranks))
        sign = sign.expand(images.shape[0], sum(ranks)).contiguous().cuda(images.device)
    return ctx.encode_rgb(images.contiguous(), list(ranks), num_iters, math.ceil(bounds[0]), math.floor(bounds[1]),
                          sign, out=out)


def qmf_encode_sweep(images: torch.Tensor, qualities=None, ranks=None, bounds=(-16, 15), num_iters: int = 10, init_sign=None,
                     pack_workers: Optional[int] = None) -> list:
    """qmf_encode of a batch [B,3,H,W] at every quality of `qualities` (or every rank / rank triple of `ranks`) in ONE GPU
    call (lrf_qmf_encode_sweep_rgb_u8: the R-D sweep of experiments/comparison/eval.py:83-110; default branch — YCbCr, 8x8
    patches).  Returns one list of B byte streams per quality, each stream byte-identical to `qmf_encode(image, quality=q)`.
    Qualities that give the same rank triple are computed once; rank triples above 32 fall back to one call each."""
    assert (qualities is None) != (ranks is None), "give either qualities or ranks"
    H, W = images.shape[-2:]
    params = list(qualities) if qualities is not None else list(ranks)
    triples = [tuple(qmf_ranks((H, W), None, p)) if qualities is not None else tuple(qmf_ranks((H, W), p, None)) for p in params]
    if images.dtype != torch.uint8:
        raise NotImplementedError("HIP path takes uint8 images")
    ctx = _lib.context(images.device.index if images.is_cuda else None)
    dev = (images if images.is_cuda else images.cuda(ctx.device)).contiguous()
    B = dev.shape[0]
    lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
    unique = sorted(set(triples))
    fused = [t for t in unique if max(t) <= 32]
    factors = {}
    if fused and num_iters >= 1:
        rmax = [max(t[c] for t in fused) for c in range(3)]
        sign = None
        if init_sign is not None:  # [Rmax_Y + Rmax_Cb + Rmax_Cr] or [B, ...]: the signs of the largest ranks' components
            sign = torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1, sum(rmax)).expand(B, sum(rmax)).contiguous().cuda(dev.device)
        for t, (U, V) in zip(fused, ctx.encode_sweep_rgb(dev, fused, num_iters, lo, hi, sign)):
            factors[t] = (U, V)
    out = {}
    for t in unique:
        if t in factors:
            Uh, Vh = (x.numpy() for x in ctx.to_host(*factors[t]))
            out[t] = pack_streams_native(Uh, Vh, (H, W), list(t), bounds, (8, 8), "uint8", threads=pack_workers or default_pack_threads())
        else:  # ranks above 32 (or num_iters = 0): the per-triple encoder
            if init_sign is not None:
                raise NotImplementedError("init_sign with rank triples outside the fused sweep")
            out[t] = qmf_encode_batch(dev, rank=list(t), bounds=bounds, num_iters=num_iters, pack_workers=pack_workers)
    return [out[t] for t in triples]


def target_candidates(image_hw, qualities):
    """The rank triples a quality grid gives on an H x W image, each once, in ascending quality, with the LOWEST quality that
    gives it: ([triple], [quality]).  (Neighbouring qualities often round to the same ranks: 32 qualities, ~24 triples.)"""
    triples, lowest = [], []
    for q in sorted(qualities):
        t = tuple(qmf_ranks(image_hw, None, q))
        if t not in triples:
            triples.append(t)
            lowest.append(q)
    return triples, lowest


def select_target(sse: torch.Tensor, n, target: torch.Tensor):
    """The choice qmf_encode_target makes, from exact squared errors: sse int64 [Q,B] (candidate q in ascending quality, image b),
    n samples per image (an integer, or one integer per image as a tensor [B]: a list of mixed sizes), target float64 [B] in dB -> (table float64 [Q,B] of PSNR, index int64 [B], reached bool [B]).
    index[b] is the FIRST candidate whose PSNR >= target[b] — every candidate is looked at, nothing assumes that PSNR grows with
    quality — and, where none reaches it, the first candidate of the highest PSNR (reached False).  sse = 0 is PSNR inf, which
    reaches every target.  Evaluated on the device `sse` lives on, by the expression image_metrics_batch uses."""
    from .metrics import psnr_from_sse
    table = psnr_from_sse(sse, n)[1]
    ok = table >= target.to(table.device).reshape(1, -1)
    reached = ok.any(dim=0)
    first_ok = torch.argmax(ok.to(torch.uint8), dim=0)  # (argmax: the first of equal maxima)
    best = torch.argmax(table, dim=0)
    return table, torch.where(reached, first_ok, best), reached


def select_target_ssim(ssim_table: torch.Tensor, psnr_table: torch.Tensor, target: torch.Tensor):
    """The choice qmf_encode_target(ssim=...) makes: ssim_table and psnr_table float64 [Q,B] (candidate q in ascending quality,
    image b), target float64 [B] -> (index int64 [B], reached bool [B]).  index[b] is the FIRST candidate with ssim >= target[b]
    — every candidate is looked at, nothing assumes that SSIM grows with quality, and a NaN never reaches —; where none reaches
    it, the first candidate of the highest non-NaN SSIM (reached False); where every SSIM of the image is NaN (a constant source:
    data_range 0), the first candidate of the highest PSNR.  Pure torch, evaluated on the device `ssim_table` lives on."""
    ok = ssim_table >= target.to(ssim_table.device).reshape(1, -1)
    reached = ok.any(dim=0)
    first_ok = torch.argmax(ok.to(torch.uint8), dim=0)  # (argmax: the first of equal maxima)
    nan = torch.isnan(ssim_table)
    best = torch.argmax(torch.where(nan, torch.full_like(ssim_table, -math.inf), ssim_table), dim=0)
    best = torch.where(nan.all(dim=0), torch.argmax(psnr_table.to(ssim_table.device), dim=0), best)
    return torch.where(reached, first_ok, best), reached


def _check_sweep_args(images, qualities, num_iters, name):
    """what qmf_encode_target and qmf_encode_budget refuse about images, qualities and num_iters -> qualities as a list"""
    if not isinstance(images, torch.Tensor):
        raise TypeError(f"{name} takes a tensor of images, got {type(images).__name__}")
    if images.dtype != torch.uint8:
        raise NotImplementedError(f"{name}: the HIP path takes uint8 images")
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError(f"{name} takes a batch [B,3,H,W], got {tuple(images.shape)}")
    if num_iters < 1:
        raise NotImplementedError(f"{name}: num_iters = 0 (the truncated initialisation) is outside the fused sweep")
    qualities = list(qualities)
    if not qualities or any(not (0 <= q <= 100) for q in qualities):
        raise ValueError(f"{name}: 'qualities' must be a non-empty sequence of numbers between 0 and 100")
    return qualities


def _check_target_args(images, psnr, qualities, num_iters):
    """qmf_encode_target's refusals, raised before a GPU is asked for -> (qualities as a list, target as float64 [B])"""
    qualities = _check_sweep_args(images, qualities, num_iters, "qmf_encode_target")
    target = torch.as_tensor(psnr, dtype=torch.float64).reshape(-1)
    B = images.shape[0]
    if target.numel() not in (1, B) or bool(torch.isnan(target).any()):
        raise ValueError(f"qmf_encode_target: 'psnr' must be one number or one per image ({B}), got {target.numel()} values")
    return qualities, target.expand(B).contiguous()


def _sweep_candidates(images, qualities, bounds, num_iters):
    """Every distinct rank triple of `qualities` factorised and scored on the GPU: triples within rank 32 in one fused sweep,
    larger ones one call each -> (ctx, the images on the device, triples, the lowest quality of each, {triple: (U, V)}, sse int64
    [Q,B] on the device)."""
    H, W = images.shape[-2:]
    B = images.shape[0]
    triples, lowest = target_candidates((H, W), qualities)
    ctx = _lib.context(images.device.index if images.is_cuda else None)
    dev = (images if images.is_cuda else images.cuda(ctx.device)).contiguous()
    lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
    fused = [t for t in triples if max(t) <= 32]
    factors = dict(zip(fused, ctx.encode_sweep_rgb(dev, fused, num_iters, lo, hi, None))) if fused else {}
    sse = torch.empty((len(triples), B), dtype=torch.int64, device=dev.device)
    if fused:
        sse[[triples.index(t) for t in fused]] = ctx.sweep_sse(dev, [factors[t] for t in fused], fused)
    for i, t in enumerate(triples):
        if t not in factors:  # a rank above 32: the per-triple encoder, scored by a sweep of one
            factors[t] = qmf_factorize_batch(dev, list(t), num_iters, bounds)
            sse[i] = ctx.sweep_sse(dev, [factors[t]], [t])[0]
    return ctx, dev, triples, lowest, factors, sse


def qmf_encode_target(images, psnr=None, qualities=range(1, 33), bounds=(-16, 15), num_iters: int = 10,
                      pack_workers: Optional[int] = None, deflate: str = "host", x_workspace_bytes: int = 1 << 30, color_space: str = "YCbCr",
                      ssim=None) -> dict:
    """Per image of a batch [B,3,H,W], the smallest-quality stream that reaches `psnr` dB (one number, or one per image).

    Default branch only (YCbCr, 8x8 patches, uint8, num_iters >= 1).  Every distinct rank triple of `qualities` is factorised on
    the GPU (triples within rank 32 in one lrf_qmf_encode_sweep_rgb_u8 call, larger ones one call each) and scored there
    straight from its factors (lrf_qmf_sweep_sse_rgb_u8: no image is decoded to memory, nothing but a [Q,B] table leaves the
    kernel).  Per image the lowest quality whose PSNR >= psnr wins; if none does, the candidate of the highest PSNR
    (reached False).  Only the winners' factors come to the host and only they are packed (zlib-9): B streams, not Q x B.

    Returns {"streams": B byte streams, stream i byte-identical to qmf_encode_batch(images[i:i+1], quality=quality[i])[0];
    "quality": the chosen quality per image (the lowest of those that share its rank triple); "psnr": float64 [B], the chosen
    stream's PSNR, what psnr_batch gives for its decode; "reached": bool [B]; "table": float64 [Q,B], the PSNR of every
    (quality of `qualities`, image) pair}.  The tensors are host tensors.

    deflate="device": the winners' columns are deflated on the GPU (as in qmf_encode_batch) and only their streams' bytes come
    to the host; the streams then hold the same factors as the default call's but are not byte-identical to them.

    `images` may also be a list or tuple of uint8 [3,H_i,W_i] tensors of differing sizes, all on the host or all on one device
    (_rate_control_list): `psnr` is then one number or one per image, the candidates of image i are
    target_candidates((H_i, W_i), qualities), and the dict has the same keys — "table" [len(qualities), B] with image i's column
    computed over its own 3 H_i W_i samples.  A quality whose triple has a rank above 32 on some image is refused
    (NotImplementedError naming the image and the quality; the default grid never gives one).  x_workspace_bytes bounds the fp32
    patch matrices of one GPU call: a longer list is processed in chunks of consecutive images, which changes no byte.  A batch
    of equal sizes is best given as a tensor.

    color_space="RGB": gray images, a list of [1,H_i,W_i] tensors or a tensor [B,1,H,W] (which goes the same way as the list of
    its images: _rate_control_list_gray).  The candidates of image i are the distinct ranks chan_rank(M_i, 64, quality) of
    `qualities`, the samples H_i W_i, a chunk counts 4 * 64 * M_i bytes per image; same keys, same meanings, stream i
    byte-identical to qmf_encode_ragged([images[i]], quality=quality[i], color_space="RGB", deflate=deflate)[0] (with the default
    deflate: to qmf_encode_batch(images[i][None], quality=quality[i], color_space="RGB")[0]).  A quality
    whose rank passes 32 on some image raises NotImplementedError naming the image and the quality; three-channel images raise
    NotImplementedError.

    ssim=: the target is an SSIM (one number, or one per image) instead of a PSNR — exactly one of `psnr` and `ssim` is given.
    A list goes through _rate_control_list with every candidate scored from its factors by lrf_qmf_ssim_ragged_rgb_u8 (decoded
    chunk by chunk into a scratch buffer of bounded size, never Q x B images); a tensor [B,3,H,W] goes the same way as the list
    of its images.  Per image the choice is select_target_ssim's: the lowest quality whose SSIM >= ssim, else the candidate of
    the highest SSIM (reached False), for a constant image (every SSIM NaN) the candidate of the highest PSNR.  Same keys —
    "table" is still the PSNR table, from the same call's exact squared errors — plus "ssim" float64 [B], the chosen stream's
    SSIM (what ssim_batch gives for its decode), and "ssim_table" float64 [len(qualities), B].  An image with a side below the
    7x7 window raises ValueError naming it; color_space="RGB" raises NotImplementedError."""
    assert color_space in ("RGB", "YCbCr"), "`color_space` must be one of 'RGB' or 'YCbCr'."
    if (psnr is None) == (ssim is None):
        raise ValueError("qmf_encode_target: give exactly one of 'psnr' and 'ssim'")
    on_device = _deflate_on_device(deflate)
    if ssim is not None:
        if color_space == "RGB":
            raise NotImplementedError("qmf_encode_target: ssim= takes three-channel images (color_space='YCbCr'); gray images take psnr=")
        if not isinstance(images, (list, tuple)):
            _check_sweep_args(images, qualities, num_iters, "qmf_encode_target")
            images = list(images.unbind(0))
        return _rate_control_list(images, "qmf_encode_target", dict(ssim=ssim), qualities, bounds, num_iters, pack_workers, on_device, x_workspace_bytes)
    if color_space == "RGB":
        return _rate_control_list_gray(images, "qmf_encode_target", dict(psnr=psnr), qualities, bounds, num_iters, pack_workers, on_device,
                                       x_workspace_bytes)
    if isinstance(images, (list, tuple)):
        return _rate_control_list(images, "qmf_encode_target", dict(psnr=psnr), qualities, bounds, num_iters, pack_workers, on_device, x_workspace_bytes)
    qualities, target = _check_target_args(images, psnr, qualities, num_iters)
    H, W = images.shape[-2:]
    B = images.shape[0]
    ctx, dev, triples, lowest, factors, sse = _sweep_candidates(images, qualities, bounds, num_iters)
    table, index, reached = select_target(sse, 3 * H * W, target)
    chosen_psnr = table.gather(0, index.reshape(1, -1))[0]
    table, index, reached, chosen_psnr = table.cpu(), index.cpu(), reached.cpu(), chosen_psnr.cpu()
    streams = [None] * B
    for i, t in enumerate(triples):  # images choose different triples: one gather, one copy and one packing call per group
        rows = torch.nonzero(index == i).reshape(-1)
        if rows.numel() == 0:
            continue
        sel = rows.to(dev.device)
        if on_device:
            for b, s_ in zip(rows.tolist(), _device_streams_of_rows(ctx, factors[t], sel, (H, W), t, bounds, pack_workers)):
                streams[b] = s_
            continue
        Uh, Vh = (x.numpy() for x in ctx.to_host(factors[t][0].index_select(0, sel), factors[t][1].index_select(0, sel)))
        packed = pack_streams_native(Uh, Vh, (H, W), list(t), bounds, (8, 8), "uint8", threads=pack_workers or default_pack_threads())
        for b, s in zip(rows.tolist(), packed):
            streams[b] = s
    row_of = [triples.index(tuple(qmf_ranks((H, W), None, q))) for q in qualities]
    return {"streams": streams, "quality": [lowest[i] for i in index.tolist()], "psnr": chosen_psnr, "reached": reached,
            "table": table[row_of]}


def _device_streams_of_rows(ctx, pair, sel, image_hw, triple, bounds, pack_workers) -> list:
    """the deflate="device" streams of the images `sel` (a device index tensor) of one triple's factors (U [B,nu], V [B,nv])"""
    Us, Vs = pair[0].index_select(0, sel), pair[1].index_select(0, sel)
    k = Us.shape[0]
    return streams_from_device_factors(ctx, Us, Vs, [tuple(image_hw)] * k, [triple] * k, np.arange(k, dtype=np.int64) * Us.shape[1],
                                       np.arange(k, dtype=np.int64) * Vs.shape[1], bounds, _pack_threads(pack_workers))


@functools.lru_cache(maxsize=256)
def _factor_header_len(r):
    return len(dict_to_bytes({"num_fibers": r, "mode": "col", "dtype": "int8"}))


def container_bytes(meta_len, ranks, column_lengths):
    """len() of the container lrf_pack_qmf_streams_deflated folds from an image's deflated columns, by host arithmetic: the
    metadata JSON of meta_len bytes, then six factors (u_Y, v_Y, u_Cb, v_Cb, u_Cr, v_Cr), each one JSON header {"num_fibers",
    "mode", "dtype"} in front of its ranks[c] columns; combine_bytes puts four length bytes in front of every part but the last
    (container.py).  column_lengths: integers [..., 2 sum(ranks)] (an array or a tensor, on any device), the lengths of an image's
    column streams in any order -> their sum over the last axis plus the constant of (meta_len, ranks), computed once for all
    images."""
    ranks = [int(r) for r in ranks]
    lens = column_lengths if isinstance(column_lengths, torch.Tensor) else np.asarray(column_lengths, dtype=np.int64)
    if len(ranks) != 3 or min(ranks) < 1 or lens.shape[-1] != 2 * sum(ranks):
        raise ValueError(f"container_bytes: three ranks >= 1 and 2 sum(ranks) column lengths expected, got {ranks} and {tuple(lens.shape)}")
    const = 4 + int(meta_len) + 4 * 5  # the metadata's prefix; five of the six factors carry one
    for r in ranks:  # per factor: the header and its prefix, a prefix for every column but the last
        const += 2 * (4 + _factor_header_len(r) + 4 * (r - 1))
    total = lens.sum(dim=-1, dtype=torch.int64) if isinstance(lens, torch.Tensor) else lens.sum(axis=-1, dtype=np.int64)
    return total + const


def qmf_stream_sizes(factors, triples, image_hw, bounds=(-16, 15)) -> torch.Tensor:
    """The exact size of every stream of a sweep, counted on the GPU without producing one (lrf_deflate_sizes_i8).  factors: one
    (U, V) pair of int8 CUDA tensors per rank triple of `triples`, as Context.encode_sweep_rgb returns them (for one triple:
    [qmf_factorize_batch's pair], or the pair and the triple themselves) -> int64 CUDA tensor [Q, B], out[q][b] = len() of the
    stream streams_from_device_factors (deflate="device") produces for image b at triple q.  One count over all U matrices and
    one over all V matrices; the factors are taken where they lie when they are consecutive views of two flat buffers and
    concatenated otherwise.  The column lengths are summed per (q, b) on the device and the container constant of triple q added."""
    if len(factors) == 2 and isinstance(factors[0], torch.Tensor):
        factors, triples = [factors], [triples]
    triples = [tuple(int(r) for r in t) for t in triples]
    H, W = image_hw
    if not factors or len(factors) != len(triples):
        raise ValueError("qmf_stream_sizes needs one (U, V) pair per rank triple")
    Ms = np.array([d[4] for d in _lib.plane_dims(H, W)], dtype=np.int64)
    B = factors[0][0].shape[0]
    u_mats, v_mats, uo, vo = [], [], 0, 0
    for (U, V), t in zip(factors, triples):
        R = np.array(t, dtype=np.int64)
        nu, nv = int((Ms * R).sum()), 64 * int(R.sum())
        if not (isinstance(U, torch.Tensor) and isinstance(V, torch.Tensor) and U.dtype == torch.int8 and V.dtype == torch.int8):
            raise TypeError("factors must be int8 tensors")
        if len(t) != 3 or min(t) < 1 or tuple(U.shape) != (B, nu) or tuple(V.shape) != (B, nv):
            raise ValueError(f"factor buffers do not match the geometry at ranks {t}: expected int8 U {(B, nu)} and V {(B, nv)}, got "
                             f"{tuple(U.shape)} and {tuple(V.shape)}")
        for mats, at, per_image, first, rows in ((u_mats, uo, nu, np.cumsum(Ms * R) - Ms * R, Ms),
                                                 (v_mats, vo, nv, 64 * (np.cumsum(R) - R), np.full(3, 64, dtype=np.int64))):
            m = np.empty((B, 3, 3), dtype=np.int64)  # (src_off, rows, cols): image after image, plane after plane
            m[:, :, 0] = at + per_image * np.arange(B, dtype=np.int64).reshape(B, 1) + first
            m[:, :, 1] = rows
            m[:, :, 2] = R
            mats.append(m.reshape(-1, 3))
        uo += B * nu
        vo += B * nv
    ctx = _lib.context(factors[0][0].device.index)
    u_len = ctx.deflate_sizes(_lib.flat_views([f[0] for f in factors]), np.concatenate(u_mats))
    v_len = ctx.deflate_sizes(_lib.flat_views([f[1] for f in factors]), np.concatenate(v_mats))
    out = torch.empty((len(triples), B), dtype=torch.int64, device=u_len.device)
    at = 0
    for q, t in enumerate(triples):  # the lengths lie triple after triple, image after image: [B, sum(ranks)] of each kind
        n = B * sum(t)
        cols = torch.cat([u_len[at:at + n].view(B, -1), v_len[at:at + n].view(B, -1)], dim=1)
        out[q] = container_bytes(len(_stream_metadata((H, W), list(t), bounds)), t, cols)
        at += n
    return out


def select_budget(size: torch.Tensor, sse: torch.Tensor, budget: torch.Tensor):
    """The choice qmf_encode_budget makes, from exact sizes and exact squared errors: size, sse int64 [Q,B] (candidate q in
    ascending quality, image b), budget int64 [B] in bytes -> (index int64 [B], reached bool [B]).  Per image, among the
    candidates with size <= budget the one of the LOWEST sse wins; equal sse: the smaller size; equal in both: the lowest
    quality.  Every candidate is looked at — nothing assumes that size or error is monotonic in quality.  Where no candidate fits,
    the smallest stream wins (equal sizes: the lowest quality) and reached is False.  Evaluated on the device the tables live on."""
    Q = size.shape[0]
    big = torch.iinfo(torch.int64).max
    rank = torch.arange(Q, dtype=torch.int64, device=size.device).reshape(Q, 1)
    fits = size <= budget.to(size.device).reshape(1, -1)
    reached = fits.any(dim=0)
    best = fits & (sse == torch.where(fits, sse, big).min(dim=0).values)
    best = best & (size == torch.where(best, size, big).min(dim=0).values)
    smallest = size == size.min(dim=0).values
    index = torch.where(torch.where(reached, best, smallest), rank, Q).min(dim=0).values
    return index, reached


def _check_budget_args(images, bpp, nbytes, qualities, num_iters):
    """qmf_encode_budget's refusals, raised before a GPU is asked for -> (qualities as a list, budget as int64 [B] in bytes)"""
    qualities = _check_sweep_args(images, qualities, num_iters, "qmf_encode_budget")
    if (bpp is None) == (nbytes is None):
        raise ValueError("qmf_encode_budget: give exactly one of 'bpp' and 'nbytes'")
    B, _, H, W = images.shape
    name, value = ("bpp", bpp) if bpp is not None else ("nbytes", nbytes)
    v = torch.as_tensor(value).detach().cpu()
    if v.dtype == torch.bool or v.is_complex():
        raise TypeError(f"qmf_encode_budget: '{name}' must hold numbers, got {v.dtype}")
    v = v.to(torch.float64).reshape(-1)
    if v.numel() not in (1, B) or bool(torch.isnan(v).any()) or bool((v < 0).any()):
        raise ValueError(f"qmf_encode_budget: '{name}' must be one number >= 0 or one per image ({B}), got {v.tolist() if v.numel() <= 8 else v.numel()}")
    if bpp is not None:
        v = v * H * W / 8  # bits per pixel become bytes once, in float64; everything after that is integers
    budget = torch.floor(v).clamp(max=2.0 ** 62).to(torch.int64)
    return qualities, budget.expand(B).contiguous()


def qmf_encode_budget(images, bpp=None, nbytes=None, qualities=range(1, 33), bounds=(-16, 15), num_iters: int = 10,
                      pack_workers: Optional[int] = None, x_workspace_bytes: int = 1 << 30, color_space: str = "YCbCr") -> dict:
    """Per image of a batch [B,3,H,W], the best stream that fits a byte budget: `nbytes` bytes, or `bpp` bits per pixel (=
    floor(bpp H W / 8) bytes); one number, or one per image.

    Default branch only (YCbCr, 8x8 patches, uint8, num_iters >= 1).  Every distinct rank triple of `qualities` is factorised
    and scored on the GPU as in qmf_encode_target, and the size of every candidate's stream is COUNTED there, exact to the byte,
    without producing it (qmf_stream_sizes: the device coder's streams have a length that follows from their columns' byte
    counts alone; zlib-9 streams do not, so the budget is met by deflate="device" streams).  select_budget picks per image; only
    the winners' factors are gathered and packed, B streams instead of Q x B, and every packed stream's length is compared with
    the counted one (RuntimeError on a difference).

    Returns {"streams": B byte streams, stream i byte-identical to qmf_encode_batch(images[i:i+1], quality=quality[i],
    deflate="device")[0]; "quality": the chosen quality per image (the lowest of those that share its rank triple); "nbytes":
    int64 [B], their lengths; "bpp": float64 [B], bits_per_pixel((H, W), stream); "psnr": float64 [B]; "reached": bool [B], False
    where no candidate fits (the smallest stream is returned then); "size_table": int64 [len(qualities), B]; "table": float64
    [len(qualities), B], the PSNR of every (quality, image) pair}.  The tensors are host tensors.

    `images` may also be a list or tuple of uint8 [3,H_i,W_i] tensors of differing sizes, all on the host or all on one device
    (_rate_control_list): `bpp` / `nbytes` are then one number or one per image, `bpp` converted with each image's own H_i W_i;
    same keys, same meanings.  Refusals and x_workspace_bytes: as in qmf_encode_target.

    color_space="RGB": gray images, a list of [1,H_i,W_i] tensors or a tensor [B,1,H,W], as in qmf_encode_target; the sizes are
    those of the two-factor containers the device coder's columns fold into (qmf_stream_sizes_gray_ragged), and stream i is
    byte-identical to qmf_encode_ragged([images[i]], quality=quality[i], color_space="RGB", deflate="device")[0]."""
    from .metrics import bits_per_pixel, psnr_from_sse
    assert color_space in ("RGB", "YCbCr"), "`color_space` must be one of 'RGB' or 'YCbCr'."
    if color_space == "RGB":
        return _rate_control_list_gray(images, "qmf_encode_budget", dict(bpp=bpp, nbytes=nbytes), qualities, bounds, num_iters, pack_workers, True,
                                       x_workspace_bytes)
    if isinstance(images, (list, tuple)):
        return _rate_control_list(images, "qmf_encode_budget", dict(bpp=bpp, nbytes=nbytes), qualities, bounds, num_iters, pack_workers, True,
                                  x_workspace_bytes)
    qualities, budget = _check_budget_args(images, bpp, nbytes, qualities, num_iters)
    H, W = images.shape[-2:]
    B = images.shape[0]
    ctx, dev, triples, lowest, factors, sse = _sweep_candidates(images, qualities, bounds, num_iters)
    size = torch.empty_like(sse)
    fused = [t for t in triples if max(t) <= 32]  # (their factors are views of two flat buffers: counted where they lie)
    if fused:
        size[[triples.index(t) for t in fused]] = qmf_stream_sizes([factors[t] for t in fused], fused, (H, W), bounds)
    for i, t in enumerate(triples):
        if max(t) > 32:
            size[i] = qmf_stream_sizes([factors[t]], [t], (H, W), bounds)[0]
    index, reached = select_budget(size, sse, budget)
    table = psnr_from_sse(sse, 3 * H * W)[1]
    chosen_psnr = table.gather(0, index.reshape(1, -1))[0]
    counted = size.gather(0, index.reshape(1, -1))[0]
    table, size, index, reached, chosen_psnr, counted = (x.cpu() for x in (table, size, index, reached, chosen_psnr, counted))
    streams = [None] * B
    for i, t in enumerate(triples):  # images choose different triples: one gather, one deflate and one fold per group
        rows = torch.nonzero(index == i).reshape(-1)
        if rows.numel() == 0:
            continue
        for b, s in zip(rows.tolist(), _device_streams_of_rows(ctx, factors[t], rows.to(dev.device), (H, W), t, bounds, pack_workers)):
            streams[b] = s
    for b, s in enumerate(streams):
        if len(s) != int(counted[b]):
            raise RuntimeError(f"qmf_encode_budget: image {b} at quality {lowest[int(index[b])]}: the stream has {len(s)} bytes, "
                               f"{int(counted[b])} were counted")
    row_of = [triples.index(tuple(qmf_ranks((H, W), None, q))) for q in qualities]
    return {"streams": streams, "quality": [lowest[i] for i in index.tolist()], "nbytes": counted,
            "bpp": torch.tensor([bits_per_pixel((H, W), s) for s in streams], dtype=torch.float64), "psnr": chosen_psnr,
            "reached": reached, "size_table": size[row_of], "table": table[row_of]}


def _check_rate_list_args(images, qualities, num_iters, name):
    """what the list forms of qmf_encode_target and qmf_encode_budget refuse about images, qualities and num_iters, before a GPU
    is asked for -> (qualities as a list, [(H, W)], per image (triples, lowest, rows): what target_candidates gives for its size and,
    per quality in ascending order, which of the triples it has — worked out once per distinct size)"""
    if len(images) < 1:
        raise ValueError(f"{name} takes a non-empty list of images")
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor):
            raise TypeError(f"{name}: image {i} is {type(im).__name__}, not a tensor")
        if im.dim() == 4:  # a batch wrapped in a list is the wrong kind of argument, as before lists were taken: the batch itself is the tensor form
            raise TypeError(f"{name}: entry {i} of the list is a batch {tuple(im.shape)}; a list holds [3,H,W] images, a batch is passed as a tensor")
        if im.dtype != torch.uint8:
            raise NotImplementedError(f"{name}: image {i} is {im.dtype}; the HIP path takes uint8 images")
        if im.dim() != 3 or im.shape[0] != 3 or im.shape[1] < 1 or im.shape[2] < 1:
            raise ValueError(f"{name}: image {i} must be [3,H,W], got {tuple(im.shape)}")
    if len({im.device for im in images}) != 1:
        raise ValueError(f"{name}: the images of a list must all be on the host or all on one device, got {sorted({str(im.device) for im in images})}")
    if num_iters < 1:
        raise NotImplementedError(f"{name}: num_iters = 0 (the truncated initialisation) is outside the fused sweep")
    qualities = list(qualities)
    if not qualities or any(not (0 <= q <= 100) for q in qualities):
        raise ValueError(f"{name}: 'qualities' must be a non-empty sequence of numbers between 0 and 100")
    sizes = [(int(im.shape[1]), int(im.shape[2])) for im in images]
    per_size = {}
    for i, hw in enumerate(sizes):
        if hw in per_size:
            continue
        if 3 * hw[0] * hw[1] >= 2 ** 31:
            raise NotImplementedError(f"{name}: image {i} of {hw[0]}x{hw[1]} has 2^31 / 3 pixels or more")
        for q in sorted(qualities):
            t = qmf_ranks(hw, None, q)
            if max(t) > 32:
                raise NotImplementedError(f"{name}: image {i} ({hw[0]}x{hw[1]}) at quality {q} has ranks {tuple(t)}: a list takes ranks up to 32 "
                                          f"(encode such images one by one through the tensor form)")
        triples, lowest = target_candidates(hw, qualities)
        per_size[hw] = (triples, lowest, [triples.index(tuple(qmf_ranks(hw, None, q))) for q in sorted(qualities)])
    return qualities, sizes, [per_size[hw] for hw in sizes]


def _per_image_numbers(value, n, name, what):
    """`value` (one number or one per image) as a float64 tensor [n] on the host; ValueError for another count or a NaN"""
    v = torch.as_tensor(value).detach().cpu()
    if v.dtype == torch.bool or v.is_complex():
        raise TypeError(f"{name}: '{what}' must hold numbers, got {v.dtype}")
    v = v.to(torch.float64).reshape(-1)
    if v.numel() not in (1, n) or bool(torch.isnan(v).any()):
        raise ValueError(f"{name}: '{what}' must be one number or one per image ({n}), got {v.numel()} values")
    return v.expand(n).contiguous()


def budget_bytes_per_image(sizes, bpp=None, nbytes=None) -> torch.Tensor:
    """The byte budget of every image of a list, int64 [B]: `nbytes` as it is, or `bpp` bits per pixel converted with each image's
    own size, floor(bpp H_i W_i / 8) — in float64 once, integers from there on (what qmf_encode_budget does for a tensor)."""
    name = "qmf_encode_budget"
    if (bpp is None) == (nbytes is None):
        raise ValueError(f"{name}: give exactly one of 'bpp' and 'nbytes'")
    v = _per_image_numbers(bpp if bpp is not None else nbytes, len(sizes), name, "bpp" if bpp is not None else "nbytes")
    if bool((v < 0).any()):
        raise ValueError(f"{name}: '{'bpp' if bpp is not None else 'nbytes'}' must be >= 0")
    if bpp is not None:
        v = v * torch.tensor([h * w for h, w in sizes], dtype=torch.float64) / 8
    return torch.floor(v).clamp(max=2.0 ** 62).to(torch.int64)


def qmf_stream_sizes_ragged(U, V, sizes, triples, u_off, v_off, bounds=(-16, 15)) -> torch.Tensor:
    """The exact length of the deflate="device" stream of every candidate of a ragged sweep, counted on the GPU without producing
    one.  U, V: flat int8 CUDA tensors holding m candidates of sizes[j] = (H, W) and ranks triples[j] at u_off[j] / v_off[j]
    (Context.encode_ragged_sweep's layout, or encode_ragged's) -> int64 CUDA tensor [m], out[j] = len() of the stream
    streams_from_device_factors produces for candidate j.  One lrf_deflate_sizes_i8 count over all U matrices and one over all V
    matrices; the column lengths are summed per candidate on the device and container_bytes adds the constant of the candidate's
    own metadata length and ranks."""
    m = len(sizes)
    if m < 1 or not (len(triples) == len(u_off) == len(v_off) == m):
        raise ValueError("qmf_stream_sizes_ragged needs one size, rank triple, u_off and v_off per candidate")
    if not (isinstance(U, torch.Tensor) and isinstance(V, torch.Tensor) and U.dtype == torch.int8 and V.dtype == torch.int8):
        raise TypeError("factors must be int8 tensors")
    key = np.concatenate([np.asarray(sizes, dtype=np.int64).reshape(m, 2), np.asarray(triples, dtype=np.int64).reshape(m, 3)], axis=1)
    Rs = key[:, 2:]
    if Rs.min() < 1:
        raise ValueError("qmf_stream_sizes_ragged: ranks must be >= 1")
    Ms = _lib.plane_patches(key[:, 0], key[:, 1])
    # the container constant once per distinct (size, triple): container_bytes of all-zero column lengths
    distinct, inverse = np.unique(key, axis=0, return_inverse=True)
    const = np.array([int(container_bytes(len(_stream_metadata((int(k[0]), int(k[1])), [int(r) for r in k[2:]], bounds)), [int(r) for r in k[2:]],
                                          np.zeros(2 * int(k[2:].sum()), dtype=np.int64))) for k in distinct], dtype=np.int64)[inverse.reshape(-1)]
    u_mats = np.empty((m, 3, 3), dtype=np.int64)  # (src_off, rows, cols): candidate after candidate, plane after plane
    u_mats[:, :, 0] = np.asarray(u_off, dtype=np.int64).reshape(m, 1) + np.cumsum(Ms * Rs, axis=1) - Ms * Rs
    u_mats[:, :, 1] = Ms
    u_mats[:, :, 2] = Rs
    v_mats = u_mats.copy()
    v_mats[:, :, 0] = np.asarray(v_off, dtype=np.int64).reshape(m, 1) + 64 * (np.cumsum(Rs, axis=1) - Rs)
    v_mats[:, :, 1] = 64
    ctx = _lib.context(U.device.index)
    out = torch.from_numpy(const).to(U.device)
    per = Rs.sum(axis=1)
    step = (1 << 20) // 3  # (lrf_deflate_sizes_i8 takes 2^20 matrices a call)
    for k in range(0, m, step):
        owner = torch.from_numpy(np.repeat(np.arange(k, min(k + step, m), dtype=np.int64), per[k:k + step])).to(U.device)
        for flat, mats in ((U, u_mats), (V, v_mats)):
            lens = ctx.deflate_sizes(flat.reshape(-1), mats[k:k + step].reshape(-1, 3))
            out.index_add_(0, owner, lens.to(torch.int64))
    return out


def _rate_control_list(images, name, goal, qualities, bounds, num_iters, pack_workers, on_device, x_workspace_bytes) -> dict:
    """qmf_encode_target / qmf_encode_budget for a list of images of differing sizes.  Per chunk of consecutive images (as many as
    keep the fp32 patch matrices within x_workspace_bytes; one image at least): ONE ragged sweep encode of every (image, candidate
    triple), ONE ragged squared error straight from the factors, for the budget ONE ragged size count, the choice on the device
    (select_target / select_budget on [len(qualities), B] tables gathered from the per-candidate vectors), and only the winners
    packed.  Nothing depends on the other images of a call, so a chunk boundary changes no byte."""
    from .metrics import bits_per_pixel, psnr_from_sse
    budget_mode = name == "qmf_encode_budget"
    ssim_mode = not budget_mode and goal.get("ssim") is not None  # the target is an SSIM: the candidates are scored by ssim_ragged
    qualities, sizes, cand_of = _check_rate_list_args(images, qualities, num_iters, name)
    B = len(images)
    if budget_mode:
        goal_t = budget_bytes_per_image(sizes, goal["bpp"], goal["nbytes"])
    elif ssim_mode:
        goal_t = _per_image_numbers(goal["ssim"], B, name, "ssim")
        for i, (h, w) in enumerate(sizes):
            if min(h, w) < 7:
                raise ValueError(f"{name}: image {i} ({h}x{w}) is smaller than the 7x7 window of the SSIM")
    else:
        goal_t = _per_image_numbers(goal["psnr"], B, name, "psnr")
    if int(x_workspace_bytes) < 1:
        raise ValueError(f"{name}: x_workspace_bytes must be >= 1")
    sorted_q = sorted(qualities)
    x_bytes = [4 * 64 * sum(d[4] for d in _lib.plane_dims(*hw)) for hw in sizes]
    chunks, at = [], 0
    while at < B:
        end, tot, ncand = at, 0, 0
        while end < B and (end == at or (tot + x_bytes[end] <= x_workspace_bytes and end - at < 65535 and ncand + len(cand_of[end][0]) <= 2 ** 20)):
            tot += x_bytes[end]
            ncand += len(cand_of[end][0])
            end += 1
        chunks.append(range(at, end))
        at = end
    ctx = _lib.context(images[0].device.index if images[0].is_cuda else None)
    dev = torch.device("cuda", ctx.device)
    lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
    streams, quality = [None] * B, [None] * B
    tables, size_tables, chosen, reached_all, counted_all, ssim_tables, chosen_ssim = [], [], [], [], [], [], []
    for chunk in chunks:
        n = len(chunk)
        offs, off = [], 0
        for i in chunk:
            offs.append(off)
            off = (off + 3 * sizes[i][0] * sizes[i][1] + 15) // 16 * 16
        if images[0].is_cuda:
            flat = torch.empty((off,), dtype=torch.uint8, device=dev)
            for i, o in zip(chunk, offs):
                flat[o:o + images[i].numel()].view(images[i].shape).copy_(images[i])
        else:
            stage = torch.empty((off,), dtype=torch.uint8).pin_memory()
            for i, o in zip(chunk, offs):
                stage[o:o + images[i].numel()].view(images[i].shape).copy_(images[i])
            flat = stage.to(dev, non_blocking=True)
        # the candidates, image after image in ascending quality, and row[q][k]: the candidate of (sorted quality q, image k)
        counts = np.array([len(cand_of[i][0]) for i in chunk], dtype=np.int64)
        first = np.cumsum(counts) - counts
        owner = np.repeat(np.arange(n, dtype=np.int64), counts)               # the image (within the chunk) of every candidate
        ranks = np.array([t for i in chunk for t in cand_of[i][0]], dtype=np.int64).reshape(-1, 3)
        row = first.reshape(1, n) + np.array([cand_of[i][2] for i in chunk], dtype=np.int64).T
        cands = np.concatenate([owner.reshape(-1, 1), ranks], axis=1)
        hw = np.array([sizes[i] for i in chunk], dtype=np.int64).reshape(n, 2)
        U, V, u_off, v_off = ctx.encode_ragged_sweep(flat, [(sizes[i][0], sizes[i][1], o) for i, o in zip(chunk, offs)], cands, num_iters, lo, hi, None)
        u_off, v_off = np.asarray(u_off, dtype=np.int64), np.asarray(v_off, dtype=np.int64)
        c_hw = hw[owner]
        items = np.concatenate([c_hw, ranks, u_off.reshape(-1, 1), v_off.reshape(-1, 1), np.asarray(offs, dtype=np.int64)[owner].reshape(-1, 1)], axis=1)
        row_d = torch.from_numpy(row).to(dev)
        if ssim_mode:
            sse_vec, ssim_vec = ctx.ssim_ragged(flat, items, U, V)
            ssim_t = ssim_vec[row_d]
        else:
            sse_vec = ctx.sse_ragged(flat, items, U, V)
        sse = sse_vec[row_d]
        samples = torch.tensor([3 * sizes[i][0] * sizes[i][1] for i in chunk], dtype=torch.int64)  # (on the host: psnr_from_sse groups the columns by count)
        goal_c = goal_t[chunk.start:chunk.stop]
        if budget_mode:
            size = qmf_stream_sizes_ragged(U, V, c_hw, ranks, u_off, v_off, bounds)[row_d]
            index, reached = select_budget(size, sse, goal_c)
            table = psnr_from_sse(sse, samples)[1]
            counted_all.append(size.gather(0, index.reshape(1, -1))[0].cpu())
            size_tables.append(size.cpu())
        elif ssim_mode:
            table = psnr_from_sse(sse, samples)[1]
            index, reached = select_target_ssim(ssim_t, table, goal_c)
            ssim_tables.append(ssim_t.cpu())
            chosen_ssim.append(ssim_t.gather(0, index.reshape(1, -1))[0].cpu())
        else:
            table, index, reached = select_target(sse, samples, goal_c)
        chosen.append(table.gather(0, index.reshape(1, -1))[0].cpu())
        tables.append(table.cpu())
        reached_all.append(reached.cpu())
        index = index.cpu().tolist()
        win = [int(row[index[k], k]) for k in range(n)]
        w_sizes, w_triples = [sizes[i] for i in chunk], [ranks[j].tolist() for j in win]
        u_off, v_off = u_off.tolist(), v_off.tolist()
        if on_device:
            packed = streams_from_device_factors(ctx, U, V, w_sizes, w_triples, [u_off[j] for j in win], [v_off[j] for j in win], bounds,
                                                 _pack_threads(pack_workers))
        else:  # only the winners' factors come to the host: gathered back to back on the device first
            nus = [sum(d[4] * r for d, r in zip(_lib.plane_dims(*hw), t)) for hw, t in zip(w_sizes, w_triples)]
            nvs = [64 * sum(t) for t in w_triples]
            Uw = torch.cat([U[u_off[j]:u_off[j] + nu] for j, nu in zip(win, nus)])
            Vw = torch.cat([V[v_off[j]:v_off[j] + nv] for j, nv in zip(win, nvs)])
            Uh, Vh = (x.numpy() for x in ctx.to_host(Uw, Vw))  # waits for the stream, then raises if a launch of this call gave up
            wu, wv = np.cumsum([0] + nus[:-1]).tolist(), np.cumsum([0] + nvs[:-1]).tolist()
            packed = None
            if pack_workers != "python" and not (isinstance(pack_workers, int) and pack_workers < 0):
                try:
                    packed, rc = pack_streams_ragged_native(Uh, Vh, w_sizes, w_triples, wu, wv, bounds, threads=pack_workers or default_pack_threads())
                    if rc:
                        raise RuntimeError(f"lrf_pack_qmf_streams_ragged failed ({rc})")
                except OSError:  # liblrf_pack.so missing or linked against another zlib: the Python container code, same bytes
                    packed = None
            if packed is None:
                packed = [pack_image(split_factors(Uh[a:a + nu], Vh[b:b + nv], hw, t), hw, t, bounds, (8, 8), "uint8")
                          for a, b, nu, nv, hw, t in zip(wu, wv, nus, nvs, w_sizes, w_triples)]
        for k, i in enumerate(chunk):
            streams[i] = packed[k]
            quality[i] = sorted_q[index[k]]
    if budget_mode:
        counted = torch.cat(counted_all)
        for b, s in enumerate(streams):
            if len(s) != int(counted[b]):
                raise RuntimeError(f"qmf_encode_budget: image {b} at quality {quality[b]}: the stream has {len(s)} bytes, {int(counted[b])} were counted")
    row_of = [sorted_q.index(q) for q in qualities]
    out = {"streams": streams, "quality": quality, "psnr": torch.cat(chosen), "reached": torch.cat(reached_all),
           "table": torch.cat(tables, dim=1)[row_of]}
    if ssim_mode:
        out["ssim"] = torch.cat(chosen_ssim)
        out["ssim_table"] = torch.cat(ssim_tables, dim=1)[row_of]
    if budget_mode:
        out["nbytes"] = counted
        out["bpp"] = torch.tensor([bits_per_pixel(hw, s) for hw, s in zip(sizes, streams)], dtype=torch.float64)
        out["size_table"] = torch.cat(size_tables, dim=1)[row_of]
    return out


def qmf_factorize_host(images: torch.Tensor, ranks: Sequence[int], num_iters: int = 10, bounds=(-16, 15), init_sign=None,
                       out=None, slots: int = 2, sub_batch: int = 0, device=None):
    """Host -> host form of qmf_factorize_batch: `images` is a uint8 CPU tensor [B,3,H,W]
    (page-locked — torch's pin_memory — for link-speed copies), the int8 factors come back as CPU tensors.  The batch
    streams through the pipelined encoder (include/lrf_hip.h, lrf_pipe): uploads, kernels and downloads of different
    sub-batches overlap.  Same values as qmf_factorize_batch, bit for bit."""
    release_plane_lanes()  # idle contexts / streams of small any-shape calls would cost the pipe's schedule
    pipe = _lib.pipe(device, slots, sub_batch)
    return pipe.encode_rgb_host(images, list(ranks), num_iters, math.ceil(bounds[0]), math.floor(bounds[1]), init_sign, out)


def split_factors(U_row: np.ndarray, V_row: np.ndarray, image_hw, ranks):
    """One image's packed factor rows -> [u_y, v_y, u_cb, v_cb, u_cr, v_cr] numpy int8 matrices."""
    H, W = image_hw
    out, uo, vo = [], 0, 0
    for (_, _, _, _, M), R in zip(_lib.plane_dims(H, W), ranks):
        out.append(U_row[uo:uo + M * R].reshape(M, R))
        out.append(V_row[vo:vo + 64 * R].reshape(64, R))
        uo += M * R
        vo += 64 * R
    return out


def pack_image(factors, image_hw, ranks, bounds, patch_size=(8, 8), dtype_name="uint8") -> bytes:
    """metadata + six factor blobs -> the reference's byte stream (lrf/compression/qmf.py:157-162,233-254,288-290)."""
    H, W = image_hw
    dims = _lib.plane_dims(H, W)
    metadata = {
        "dtype": dtype_name,
        "color space": "YCbCr",
        "patch": True,
        "bounds": bounds,
        "patch size": patch_size,
        "original size": [[d[0], d[1]] for d in dims],
        "padded size": [[d[2], d[3]] for d in dims],
        "rank": list(ranks),
    }
    return combine_bytes([dict_to_bytes(metadata), combine_bytes([encode_tensor(f) for f in factors])])


_PACK_POOL = None
_PACK_LIB = None


def default_pack_threads() -> int:
    """Host threads for the zlib-9 container packing when the caller names none: the CPUs this process may actually use —
    the smaller of its affinity mask and its cgroup CPU quota (a GPU box here: 256 CPUs in the mask, a quota of 16; more
    threads than the quota borrow against it and are then throttled, DESIGN.md "bytes out")."""
    import os
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: [t.strip(), None])):
        try:
            with open(path) as f:
                quota, period = parse(f.read())
            if period is None:
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    period = f.read().strip()
            if quota not in ("max", "-1") and int(period) > 0:
                n = min(n, max(1, int(quota) // int(period)))
            break
        except (OSError, ValueError):
            continue
    return max(1, min(n, 64))


def _pack_lib():
    """liblrf_pack.so (include/lrf_pack.h): the same container built by native host threads."""
    global _PACK_LIB
    if _PACK_LIB is None:
        import ctypes
        import os
        # LRF_PACK_LIB: another build of lrf_pack.cpp (the sanitizer builds of tools/run_sanitizers.sh)
        path = os.environ.get("LRF_PACK_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "liblrf_pack.so")
        lib = ctypes.CDLL(path)
        lib.lrf_pack_qmf_streams.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.c_char_p,
                                             ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.POINTER(ctypes.c_int64)]
        lib.lrf_pack_qmf_streams_planes.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int),
                                                    ctypes.c_int64, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int,
                                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]
        lib.lrf_pack_free.argtypes = [ctypes.c_void_p]
        lib.lrf_pack_free.restype = None
        lib.lrf_pack_unpack_qmf_factors_ragged.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                                           ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int),
                                                           ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
                                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
        lib.lrf_pack_qmf_streams_ragged.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                    ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64),
                                                    ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64),
                                                    ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]
        lib.lrf_pack_unpack_qmf_factors.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                                    ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                    ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
        # the Huffman-only deflate coder of factor columns (include/lrf_pack_deflate.h)
        lib.lrf_pack_deflate_bound.restype = ctypes.c_int64
        lib.lrf_pack_deflate_bound.argtypes = [ctypes.c_int64]
        lib.lrf_pack_deflate_column_i8.restype = ctypes.c_int64
        lib.lrf_pack_deflate_column_i8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
        lib.lrf_pack_qmf_streams_deflated.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_char_p),
                                                      ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                      ctypes.POINTER(ctypes.c_int64)]
        # the inflate of factor columns (include/lrf_pack_inflate.h)
        lib.lrf_pack_inflate_column_i8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
        lib.lrf_pack_inflate_max_distance.restype = ctypes.c_int64
        lib.lrf_pack_inflate_max_distance.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
        lib.lrf_pack_index_qmf_columns_ragged.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_int64]
        # Byte identity with the reference (CPython's zlib module at level 9) needs the same deflate implementation:
        # a Python built against another zlib (conda, zlib-ng) would make the native streams valid but different.
        import zlib
        lib.lrf_pack_zlib_version.restype = ctypes.c_char_p
        native = (lib.lrf_pack_zlib_version() or b"").decode(errors="replace")
        if native != zlib.ZLIB_RUNTIME_VERSION:
            raise OSError(f"liblrf_pack.so links zlib {native}, this Python runs zlib {zlib.ZLIB_RUNTIME_VERSION}: "
                          "using the Python container code so that streams stay byte-identical to the reference's")
        _PACK_LIB = lib
    return _PACK_LIB


def pack_streams_native(Uh: np.ndarray, Vh: np.ndarray, image_hw, ranks, bounds, patch_size=(8, 8), dtype_name="uint8",
                        threads: int = 0) -> list:
    """All images of a batch -> byte streams through liblrf_pack.so (byte-identical to pack_image)."""
    import ctypes
    H, W = image_hw
    dims = _lib.plane_dims(H, W)
    metadata = dict_to_bytes({
        "dtype": dtype_name, "color space": "YCbCr", "patch": True, "bounds": bounds, "patch size": patch_size,
        "original size": [[d[0], d[1]] for d in dims], "padded size": [[d[2], d[3]] for d in dims], "rank": list(ranks)})
    Uh = np.ascontiguousarray(Uh, dtype=np.int8)
    Vh = np.ascontiguousarray(Vh, dtype=np.int8)
    B = Uh.shape[0]
    M = (ctypes.c_int64 * 3)(*[d[4] for d in dims])
    R = (ctypes.c_int * 3)(*[int(r) for r in ranks])
    out = (ctypes.c_void_p * B)()
    lens = (ctypes.c_int64 * B)()
    rc = _pack_lib().lrf_pack_qmf_streams(Uh.ctypes.data_as(ctypes.c_void_p), Uh.shape[1], Vh.ctypes.data_as(ctypes.c_void_p),
                                          Vh.shape[1], B, M, R, metadata, len(metadata), int(threads), out, lens)
    if rc:
        raise RuntimeError(f"lrf_pack_qmf_streams failed ({rc})")
    streams = []
    for b in range(B):
        streams.append(ctypes.string_at(out[b], lens[b]))
        _pack_lib().lrf_pack_free(out[b])
    return streams


def anyshape_metadata(image_hw, ranks, bounds, patch_size, dtype_name="uint8", chroma=None) -> dict:
    """Metadata of the patch-size / patch=False streams, keys in the reference's order (qmf.py:157-162, 233-254, 265-277)."""
    dims = _lib.plane_dims_any(image_hw[0], image_hw[1], patch_size, chroma)
    metadata = {"dtype": dtype_name, "color space": "YCbCr", "patch": patch_size is not None, "bounds": bounds}
    if patch_size is not None:
        metadata["patch size"] = patch_size
        metadata["original size"] = [[d[0], d[1]] for d in dims]
        metadata["padded size"] = [[d[2], d[3]] for d in dims]
    else:
        metadata["original size"] = [[d[0], d[1]] for d in dims]
    metadata["rank"] = list(ranks)
    return metadata


def pack_anyshape_native(per_plane, image_hw, ranks, bounds, patch_size, dtype_name="uint8", chroma=None, threads: int = 0) -> list:
    """All images of a batch of the patch-size / patch=False branches -> byte streams through liblrf_pack.so
    (lrf_pack_qmf_streams_planes; byte-identical to pack_anyshape per image, tests/test_container_abi.py).
    per_plane: three (u [B,M,R], v [B,N,R]) int8 numpy pairs."""
    import ctypes
    metadata = dict_to_bytes(anyshape_metadata(image_hw, ranks, bounds, patch_size, dtype_name, chroma))
    arrs = []
    for u, v in per_plane:
        arrs += [np.ascontiguousarray(u, dtype=np.int8), np.ascontiguousarray(v, dtype=np.int8)]
    B = arrs[0].shape[0]
    F = (ctypes.c_void_p * 6)(*[a.ctypes.data for a in arrs])
    rows = (ctypes.c_int64 * 6)(*[a.shape[1] for a in arrs])
    cols = (ctypes.c_int * 6)(*[a.shape[2] for a in arrs])
    out = (ctypes.c_void_p * B)()
    lens = (ctypes.c_int64 * B)()
    rc = _pack_lib().lrf_pack_qmf_streams_planes(F, rows, cols, B, 0 if patch_size is not None else 1, metadata, len(metadata), int(threads),
                                                 out, lens)
    if rc:
        raise RuntimeError(f"lrf_pack_qmf_streams_planes failed ({rc})")
    streams = []
    for b in range(B):
        streams.append(ctypes.string_at(out[b], lens[b]))
        _pack_lib().lrf_pack_free(out[b])
    return streams


def _pack_pool(workers):
    """zlib releases the GIL, so the per-column zlib-9 packing of finished images scales over host threads
    (SURVEY.md §8f N2); the streams stay byte-identical to the serial ones."""
    global _PACK_POOL
    from concurrent.futures import ThreadPoolExecutor
    if _PACK_POOL is None or _PACK_POOL._max_workers != workers:
        _PACK_POOL = ThreadPoolExecutor(max_workers=workers)
    return _PACK_POOL


def _deflate_on_device(deflate, patch=True, patch_size=(8, 8)) -> bool:
    """the `deflate` keyword of the encoders: "host" (False) or "device" (True); ValueError for anything else,
    NotImplementedError for the branches the device coder does not serve yet"""
    if deflate not in ("host", "device"):
        raise ValueError(f"deflate must be 'host' or 'device', got {deflate!r}")
    if deflate == "device" and (not patch or tuple(patch_size) != (8, 8)):
        raise NotImplementedError("deflate='device' covers the 8x8-patch branch only (patch=False packs a factor as one long fiber)")
    return deflate == "device"


def _pack_threads(pack_workers) -> int:
    return pack_workers if isinstance(pack_workers, int) and pack_workers > 0 else default_pack_threads()


def streams_from_device_factors(ctx, U, V, sizes, triples, u_off, v_off, bounds, threads: int = 0) -> list:
    """The one way factors become streams with deflate="device": U, V flat int8 CUDA tensors holding n images of sizes[i] =
    (H, W) and ranks triples[i] at u_off[i] / v_off[i] (encode_rgb's layout of one image each).  Every column is deflated where
    it lies (lrf_deflate_columns_i8, one call for the U matrices and one for the V matrices into the same slots and lengths),
    the slots and the lengths come to the host in one copy each (ctx.to_host: a failed launch raises here) and
    lrf_pack_qmf_streams_deflated folds them into the containers.  The streams are not byte-identical to the zlib-9 ones; they
    hold the same factors and every inflate reads them."""
    import ctypes
    lib = _pack_lib()
    n = len(sizes)
    m_of, meta_of = {}, {}
    for hw, t in zip(sizes, triples):
        if tuple(hw) not in m_of:
            m_of[tuple(hw)] = [int(d[4]) for d in _lib.plane_dims(*hw)]
        if (tuple(hw), tuple(t)) not in meta_of:
            meta_of[(tuple(hw), tuple(t))] = _stream_metadata(hw, list(t), bounds)
    Ms = np.array([m_of[tuple(hw)] for hw in sizes], dtype=np.int64).reshape(n, 3)
    Rs = np.array([[int(r) for r in t] for t in triples], dtype=np.int64).reshape(n, 3)
    mats = np.empty((n, 3, 2, 3), dtype=np.int64)  # (src_off, rows, cols) in stream order: image, plane, U before V
    mats[:, :, 0, 0] = np.asarray(u_off, dtype=np.int64).reshape(n, 1) + np.cumsum(Ms * Rs, axis=1) - Ms * Rs
    mats[:, :, 0, 1] = Ms
    mats[:, :, 1, 0] = np.asarray(v_off, dtype=np.int64).reshape(n, 1) + 64 * (np.cumsum(Rs, axis=1) - Rs)
    mats[:, :, 1, 1] = 64
    mats[:, :, :, 2] = Rs[:, :, None]
    table, nbytes, ncols = _lib.deflate_table(mats.reshape(-1, 3))
    slots = torch.empty((nbytes,), dtype=torch.uint8, device=U.device)
    lens = torch.empty((ncols,), dtype=torch.int32, device=U.device)
    by_factor = table.reshape(n, 3, 2, 5)
    ctx.deflate_columns_into(U.reshape(-1), by_factor[:, :, 0].reshape(-1, 5), slots, lens)
    ctx.deflate_columns_into(V.reshape(-1), by_factor[:, :, 1].reshape(-1, 5), slots, lens)
    slots_h, lens_h = (t.numpy() for t in ctx.to_host(slots, lens))
    col_off = _lib.deflate_column_offsets(table)
    metas = [meta_of[(tuple(hw), tuple(t))] for hw, t in zip(sizes, triples)]
    meta_len = np.array([len(m) for m in metas], dtype=np.int64)
    R32 = np.ascontiguousarray(Rs, dtype=np.int32)
    out = (ctypes.c_void_p * n)()
    out_len = (ctypes.c_int64 * n)()
    rc = lib.lrf_pack_qmf_streams_deflated(slots_h.ctypes.data, slots_h.size, n, Ms.ctypes.data, R32.ctypes.data, col_off.ctypes.data,
                                           lens_h.ctypes.data, ncols, (ctypes.c_char_p * n)(*metas), meta_len.ctypes.data, int(threads), out, out_len)
    if rc:
        raise RuntimeError(f"lrf_pack_qmf_streams_deflated failed ({rc})")
    streams = []
    for b in range(n):
        streams.append(ctypes.string_at(out[b], out_len[b]))
        lib.lrf_pack_free(out[b])
    return streams


def qmf_encode_batch(images: torch.Tensor, rank=None, quality=None, bounds=(-16, 15), num_iters: int = 10,
                     init_sign=None, pack_workers: Optional[int] = None, patch: bool = True, patch_size=(8, 8), deflate: str = "host",
                     color_space: str = "YCbCr") -> list:
    """Batched qmf_encode (YCbCr branch) -> list of byte streams, one per image.  The factorisation of the whole batch
    runs on the GPU; for the default 8x8 patches the byte containers are packed by liblrf_pack.so on native host threads
    (`pack_workers` None / 0: as many as this process may use, default_pack_threads), or, with pack_workers="python", by the Python container code on a
    thread pool.  Other patch sizes and patch=False go through the any-shape kernels (container packed in Python).

    deflate="device": the columns are deflated on the GPU (Huffman-only zlib streams, lrf_deflate_columns_i8) while the factors
    are still there, and the host only folds them into the container: same factors, other bytes, read by every decoder.  8x8
    patches only (NotImplementedError otherwise).  A host tensor then takes the context path (upload, factorise, deflate), not
    the pipelined encoder: wiring the pipe's slots to the coder is a follow-up.

    color_space="RGB": gray images [B,1,H,W] with 8x8 patches, the streams of qmf_encode(images[i], color_space="RGB")
    (_qmf_encode_batch_gray); other channel counts, patch settings and deflate="device" raise NotImplementedError (the device
    coder serves gray images through qmf_encode_ragged(color_space="RGB", deflate="device"))."""
    assert (rank, quality) != (None, None), "Either 'rank' or 'quality' must be specified."
    assert color_space in ("RGB", "YCbCr"), "`color_space` must be one of 'RGB' or 'YCbCr'."
    if color_space == "RGB":  # gray images [B,1,H,W]: one lrf_qmf_encode_gray_u8 call
        return _qmf_encode_batch_gray(images, rank, quality, bounds, num_iters, init_sign, pack_workers, patch, patch_size, deflate)
    H, W = images.shape[-2:]
    on_device = _deflate_on_device(deflate, patch, patch_size)
    if on_device:
        if images.dtype != torch.uint8:
            raise NotImplementedError("HIP path takes uint8 images")
        ctx = _lib.context(images.device.index if images.is_cuda else None)
        dev = images if images.is_cuda else images.cuda(ctx.device)
        ranks = qmf_ranks((H, W), rank, quality)
        U, V = qmf_factorize_batch(dev, ranks, num_iters, bounds, init_sign)
        B = U.shape[0]
        return streams_from_device_factors(ctx, U, V, [(H, W)] * B, [ranks] * B, np.arange(B, dtype=np.int64) * U.shape[1],
                                           np.arange(B, dtype=np.int64) * V.shape[1], bounds, _pack_threads(pack_workers))
    if (not images.is_cuda) and patch and tuple(patch_size) == (8, 8) and images.dtype == torch.uint8 and num_iters >= 1 \
            and pack_workers != "python" and not (isinstance(pack_workers, int) and pack_workers < 0):
        # host tensor in, byte streams out: the pipelined encoder, the container of each finished sub-batch packed by
        # liblrf_pack.so while the GPU works on the next ones
        try:
            _pack_lib()
        except OSError:
            pass
        else:
            ranks = qmf_ranks((H, W), rank, quality)
            release_plane_lanes()  # idle contexts / streams of small any-shape calls would cost the pipe's schedule
            pipe = _lib.pipe(None)
            streams = []
            for first, n, U, V in pipe.encode_rgb_host_iter(images, ranks, num_iters, math.ceil(bounds[0]), math.floor(bounds[1]),
                                                            init_sign):
                streams += pack_streams_native(U[first:first + n].numpy(), V[first:first + n].numpy(), (H, W), ranks, bounds,
                                               (8, 8), "uint8", threads=pack_workers or default_pack_threads())
            return streams
    ctx = _lib.context(images.device.index if images.is_cuda else None)
    dev = images if images.is_cuda else images.cuda(ctx.device)
    if not patch or tuple(patch_size) != (8, 8):
        if images.dtype != torch.uint8:
            raise NotImplementedError("HIP path takes uint8 images")
        lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
        return _qmf_encode_anyshape(ctx, dev, rank, quality, bounds, (lo, hi), tuple(patch_size) if patch else None, num_iters,
                                    init_sign, None)
    ranks = qmf_ranks((H, W), rank, quality)
    U, V = qmf_factorize_batch(dev, ranks, num_iters, bounds, init_sign)
    Uh, Vh = (t.numpy() for t in ctx.to_host(U, V))  # waits for the stream, then raises if a launch of this call gave up
    dtype_name = str(images.dtype).split(".")[-1]
    if pack_workers != "python" and not (isinstance(pack_workers, int) and pack_workers < 0):
        try:
            return pack_streams_native(Uh, Vh, (H, W), ranks, bounds, (8, 8), dtype_name, threads=pack_workers or default_pack_threads())
        except OSError:  # liblrf_pack.so missing or linked against another zlib: the Python container code, same bytes
            pack_workers = "python"
    pack_workers = None if pack_workers == "python" else -pack_workers

    def pack(b):
        return pack_image(split_factors(Uh[b], Vh[b], (H, W), ranks), (H, W), ranks, bounds, (8, 8), dtype_name)

    import os
    workers = pack_workers if pack_workers is not None else min(32, os.cpu_count() or 1)
    if workers <= 1 or images.shape[0] == 1:
        return [pack(b) for b in range(images.shape[0])]
    return list(_pack_pool(workers).map(pack, range(images.shape[0])))


def _stream_metadata(image_hw, ranks, bounds, patch_size=(8, 8), dtype_name="uint8") -> bytes:
    """the metadata block pack_image writes for one image of the default branch"""
    dims = _lib.plane_dims(*image_hw)
    return dict_to_bytes({
        "dtype": dtype_name, "color space": "YCbCr", "patch": True, "bounds": bounds, "patch size": patch_size,
        "original size": [[d[0], d[1]] for d in dims], "padded size": [[d[2], d[3]] for d in dims], "rank": list(ranks)})


def pack_streams_ragged_native(Uh: np.ndarray, Vh: np.ndarray, sizes, triples, u_off, v_off, bounds, threads: int = 0):
    """lrf_pack_qmf_streams_ragged: flat int8 U / V holding n images of sizes[i] = (H, W) and ranks triples[i] at u_off[i] /
    v_off[i] -> (n byte streams, each byte-identical to pack_image of that image, 0), or (None, rc) when the library refuses the
    layout.  Raises OSError where liblrf_pack.so cannot be used."""
    import ctypes
    lib = _pack_lib()
    n = len(sizes)
    Uh = np.ascontiguousarray(Uh, dtype=np.int8).reshape(-1)
    Vh = np.ascontiguousarray(Vh, dtype=np.int8).reshape(-1)
    metas = [_stream_metadata(hw, t, bounds) for hw, t in zip(sizes, triples)]
    out = (ctypes.c_void_p * max(n, 1))()
    lens = (ctypes.c_int64 * max(n, 1))()
    rc = lib.lrf_pack_qmf_streams_ragged(
        Uh.ctypes.data_as(ctypes.c_void_p), Uh.size, Vh.ctypes.data_as(ctypes.c_void_p), Vh.size, n,
        (ctypes.c_int64 * max(3 * n, 1))(*[int(d[4]) for hw in sizes for d in _lib.plane_dims(*hw)]),
        (ctypes.c_int * max(3 * n, 1))(*[int(r) for t in triples for r in t]), (ctypes.c_int64 * max(n, 1))(*[int(x) for x in u_off]),
        (ctypes.c_int64 * max(n, 1))(*[int(x) for x in v_off]), (ctypes.c_char_p * max(n, 1))(*metas),
        (ctypes.c_int64 * max(n, 1))(*[len(m) for m in metas]), int(threads), out, lens)
    if rc:
        return None, rc
    streams = []
    for b in range(n):
        streams.append(ctypes.string_at(out[b], lens[b]))
        lib.lrf_pack_free(out[b])
    return streams, 0


def _per_image(value, n, name, one):
    """`value` as a list of n entries: `one(value)` says whether it is a single entry meant for every image"""
    if value is None or one(value):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"qmf_encode_ragged: '{name}' must be one value or one per image ({n}), got {len(value)} entries")
    return value


def _check_encode_ragged_args(images, rank, quality, ranks, num_iters, init_sign):
    """qmf_encode_ragged's refusals, raised before a GPU is asked for -> ([(H, W)], [rank triple per image], [sign per image: None or int8 array])"""
    if isinstance(images, torch.Tensor) and images.dim() != 4:
        raise ValueError(f"qmf_encode_ragged takes a sequence of [3,H,W] images, got a tensor of shape {tuple(images.shape)}")
    if isinstance(images, (bytes, str)) or len(images) < 1:
        raise ValueError("qmf_encode_ragged takes a non-empty sequence of images")
    n = len(images)
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor):
            raise TypeError(f"qmf_encode_ragged: image {i} is {type(im).__name__}, not a tensor")
        if im.dtype != torch.uint8:
            raise NotImplementedError(f"qmf_encode_ragged: image {i} is {im.dtype}; the HIP path takes uint8 images")
        if im.dim() != 3 or im.shape[0] != 3 or im.shape[1] < 1 or im.shape[2] < 1:
            raise ValueError(f"qmf_encode_ragged: image {i} must be [3,H,W], got {tuple(im.shape)}")
    if num_iters < 1:
        raise NotImplementedError("qmf_encode_ragged: num_iters = 0 (the truncated initialisation) is outside the fused encoder (qmf_encode takes it)")
    if sum(x is not None for x in (rank, quality, ranks)) != 1:
        raise ValueError("qmf_encode_ragged: give exactly one of 'rank', 'quality' and 'ranks'")
    scalar = lambda v: not isinstance(v, Iterable)
    triple = lambda v: len(v) == 3 and all(scalar(x) for x in v)
    rank_l = _per_image(rank, n, "rank", scalar)
    quality_l = _per_image(quality, n, "quality", scalar)
    ranks_l = _per_image(None if ranks is None else list(ranks), n, "ranks", triple)
    sizes = [(int(im.shape[1]), int(im.shape[2])) for im in images]
    triples = []
    for i, hw in enumerate(sizes):
        r = rank_l[i] if ranks_l[i] is None else list(ranks_l[i])
        if r is None and quality_l[i] is None:
            raise ValueError(f"qmf_encode_ragged: image {i} has neither a rank nor a quality")
        if isinstance(r, list) and len(r) != 3:
            raise ValueError(f"qmf_encode_ragged: image {i}: a rank triple has three entries, got {len(r)}")
        t = [int(x) for x in qmf_ranks(hw, r, quality_l[i])]
        if min(t) < 1:
            raise ValueError(f"qmf_encode_ragged: image {i}: ranks {t} must be >= 1")
        triples.append(t)
    one_sign = lambda v: isinstance(v, (np.ndarray, torch.Tensor)) or (len(v) > 0 and all(x is not None and scalar(x) for x in v))
    signs = []
    for i, sg in enumerate(_per_image(init_sign, n, "init_sign", one_sign)):
        if sg is not None:
            sg = np.ascontiguousarray(torch.as_tensor(sg, dtype=torch.int8).reshape(-1).numpy())
            if sg.size != sum(triples[i]):
                raise ValueError(f"qmf_encode_ragged: image {i}: init_sign holds {sg.size} signs, its ranks {triples[i]} need {sum(triples[i])}")
        signs.append(sg)
    return sizes, triples, signs


def qmf_encode_ragged(images, rank=None, quality=None, ranks=None, bounds=(-16, 15), num_iters: int = 10, init_sign=None,
                      pack_workers: Optional[int] = None, deflate: str = "host", color_space: str = "YCbCr") -> list:
    """qmf_encode of a list of uint8 images [3,H_i,W_i] (host or device) that differ in size and in ranks, in one GPU call
    (lrf_qmf_encode_ragged_rgb_u8) -> one byte stream per image, stream i byte-identical to
    qmf_encode_batch(images[i][None], ...)[0] with that image's parameters.  Default branch only (YCbCr, 8x8 patches, uint8,
    num_iters >= 1).

    rank (an integer: (r, r // 2, r // 2) as in qmf_encode), quality, ranks (a (Y, Cb, Cr) triple) and init_sign (sum(ranks)
    signs) are each one value for all images or one entry per image; every entry goes through qmf_ranks((H_i, W_i), ...).

    Host images are gathered in one page-locked buffer, each at a multiple of 16 bytes (so that images whose sides are multiples
    of 16 keep the planes kernel made for them), and go up in one copy; then one C call, one copy of all factors back and one
    call of the native packer over all columns of all images.  Images whose triple has a rank above 32 are encoded one by one
    through qmf_encode_batch and put back in place.  For a list of equal sizes and ranks qmf_encode_batch is the call to use.

    deflate="device": as in qmf_encode_batch — the columns are deflated on the GPU and only folded into the containers on the
    host; the streams hold the same factors but are not the zlib-9 bytes.

    color_space="RGB": gray images, a list of [1,H_i,W_i] tensors or a tensor [B,1,H,W], in one lrf_qmf_encode_gray_ragged_u8 call
    (_qmf_encode_ragged_gray): `rank` or `quality` is one scalar or one per image (through chan_rank(M_i, 64, ...)), `ranks` is
    refused (a gray stream has a scalar rank), init_sign holds R signs; stream i is byte-identical to
    qmf_encode_batch(images[i][None], ..., color_space="RGB")[0], images of rank above 32 go through that call one by one, and
    three-channel images raise NotImplementedError, as qmf_encode_batch(color_space="RGB") does.  deflate="device" is served
    here (gray_streams_from_device_factors: the device coder's column streams inside the two-factor container's layout; a stream
    depends on its own image and parameters alone)."""
    assert color_space in ("RGB", "YCbCr"), "`color_space` must be one of 'RGB' or 'YCbCr'."
    if color_space == "RGB":
        return _qmf_encode_ragged_gray(images, rank, quality, ranks, bounds, num_iters, init_sign, pack_workers, deflate)
    on_device = _deflate_on_device(deflate)
    sizes, triples, signs = _check_encode_ragged_args(images, rank, quality, ranks, num_iters, init_sign)
    n = len(sizes)
    streams = [None] * n
    fused = [i for i in range(n) if max(triples[i]) <= 32]
    for i in range(n):
        if i not in fused:
            streams[i] = qmf_encode_batch(images[i][None], rank=list(triples[i]), bounds=bounds, num_iters=num_iters, init_sign=signs[i],
                                          pack_workers=pack_workers, deflate=deflate)[0]
    if not fused:
        return streams
    on_dev = [images[i] for i in fused if images[i].is_cuda]
    ctx = _lib.context(on_dev[0].device.index if on_dev else None)
    dev = torch.device("cuda", ctx.device)
    offs, off = [], 0
    for i in fused:
        offs.append(off)
        off = (off + 3 * sizes[i][0] * sizes[i][1] + 15) // 16 * 16
    if on_dev:  # pixels already in HBM: gathered there
        flat = torch.empty((off,), dtype=torch.uint8, device=dev)
        for i, o in zip(fused, offs):
            flat[o:o + images[i].numel()].view(images[i].shape).copy_(images[i])
    else:
        stage = torch.empty((off,), dtype=torch.uint8).pin_memory()
        for i, o in zip(fused, offs):
            stage[o:o + images[i].numel()].view(images[i].shape).copy_(images[i])
        flat = stage.to(dev, non_blocking=True)
    sign, sign_offs = None, [-1] * len(fused)
    if any(signs[i] is not None for i in fused):
        so = 0
        for k, i in enumerate(fused):
            if signs[i] is not None:
                sign_offs[k] = so
                so += signs[i].size
        sign = torch.from_numpy(np.concatenate([signs[i] for i in fused if signs[i] is not None])).to(dev)
    lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
    U, V, u_off, v_off = ctx.encode_ragged(flat, [(sizes[i][0], sizes[i][1], triples[i], o, s) for i, o, s in zip(fused, offs, sign_offs)],
                                           num_iters, lo, hi, sign)
    if on_device:
        packed = streams_from_device_factors(ctx, U, V, [sizes[i] for i in fused], [triples[i] for i in fused], u_off, v_off, bounds,
                                             _pack_threads(pack_workers))
        for i, s_ in zip(fused, packed):
            streams[i] = s_
        return streams
    Uh, Vh = (t.numpy() for t in ctx.to_host(U, V))  # waits for the stream, then raises if a launch of this call gave up
    packed = None
    if pack_workers != "python" and not (isinstance(pack_workers, int) and pack_workers < 0):
        try:
            packed, rc = pack_streams_ragged_native(Uh, Vh, [sizes[i] for i in fused], [triples[i] for i in fused], u_off, v_off, bounds,
                                                    threads=pack_workers or default_pack_threads())
            if rc:
                raise RuntimeError(f"lrf_pack_qmf_streams_ragged failed ({rc})")
        except OSError:  # liblrf_pack.so missing or linked against another zlib: the Python container code, same bytes
            packed = None
    if packed is None:
        packed = []
        for k, i in enumerate(fused):
            nu, nv = sum(d[4] * r for d, r in zip(_lib.plane_dims(*sizes[i]), triples[i])), 64 * sum(triples[i])
            packed.append(pack_image(split_factors(Uh[u_off[k]:u_off[k] + nu], Vh[v_off[k]:v_off[k] + nv], sizes[i], triples[i]), sizes[i],
                                     triples[i], bounds, (8, 8), "uint8"))
    for i, s_ in zip(fused, packed):
        streams[i] = s_
    return streams


def qmf_encode(image: torch.Tensor, rank=None, quality=None, color_space: str = "YCbCr",
               scale_factor=(0.5, 0.5), patch: bool = True, patch_size=(8, 8), bounds=(-16, 15),
               dtype: torch.dtype = torch.int8, **kwargs) -> bytes:
    """QMF compression of one image [3,H,W]: same signature and byte stream as the reference's
    lrf.qmf_encode (lrf/compression/qmf.py:116-292).  With color_space="RGB" the image may have any channel count [C,H,W],
    1 <= C <= 16 (_qmf_encode_channels)."""
    assert (rank, quality) != (None, None), "Either 'rank' or 'quality' must be specified."
    assert color_space in ("RGB", "YCbCr"), "`color_space` must be one of 'RGB' or 'YCbCr'."
    num_iters, lo, hi, init_sign, qmf_opts = _check_hip_branch(color_space, scale_factor, patch, patch_size, bounds, dtype,
                                                               dict(kwargs))
    if image.dtype != torch.uint8:
        raise NotImplementedError("HIP path takes uint8 images")
    H, W = image.shape[-2:]
    C = image.shape[0] if image.dim() == 3 else 3
    if C != 3:  # gray and n-channel images: the RGB colour-space branch, where the reference infers c (qmf.py:43-56)
        if color_space != "RGB":
            raise NotImplementedError(f"color_space='YCbCr' needs three channels, got {C}: use color_space='RGB' (the reference's "
                                      "result there is an accident of einsum broadcasting)")
        if qmf_opts:
            raise NotImplementedError(f"{', '.join(sorted(qmf_opts))}: the general solver's options are not served for {C} channels")
    ctx = _lib.context(image.device.index if image.is_cuda else None)
    dev = (image if image.is_cuda else image.cuda(ctx.device)).unsqueeze(0)
    if C != 3:
        return _qmf_encode_channels(ctx, dev, rank, quality, bounds, (lo, hi), tuple(patch_size) if patch else None, num_iters, init_sign,
                                    kwargs.get("init"))
    if qmf_opts:  # l2 / l1_ratio / eps / num_levels: the general solver behind the same driver (qmf.py:256 forwards them to QMF)
        return _qmf_encode_general(ctx, dev, color_space, rank, quality, bounds, tuple(patch_size) if patch else None, num_iters,
                                   init_sign, kwargs.get("init"), _lib.chroma_size(H, W, scale_factor) if color_space == "YCbCr" else None,
                                   qmf_opts)
    if color_space == "RGB":
        return _qmf_encode_rgbspace(ctx, dev, rank, quality, bounds, (lo, hi), tuple(patch_size) if patch else None, num_iters, init_sign,
                                    kwargs.get("init"))
    chroma = _lib.chroma_size(H, W, scale_factor)
    if not patch or tuple(patch_size) != (8, 8) or chroma is not None:  # the any-shape path (also 8x8 with another scale factor)
        return _qmf_encode_anyshape(ctx, dev, rank, quality, bounds, (lo, hi), tuple(patch_size) if patch else None, num_iters,
                                    init_sign, kwargs.get("init"), chroma)[0]
    ranks = qmf_ranks((H, W), rank, quality)
    if num_iters == 0:
        factors = _svd_init_factors(ctx, dev, ranks, init_sign)
    else:
        U, V = qmf_factorize_batch(dev, ranks, num_iters, (lo, hi), init_sign)
        Uh, Vh = (t.numpy() for t in ctx.to_host(U, V))
        try:  # the container through liblrf_pack.so: the columns of the six factors are zlib-packed on host threads
            return pack_streams_native(Uh, Vh, (H, W), ranks, bounds, patch_size, str(image.dtype).split(".")[-1],
                                       threads=default_pack_threads())[0]
        except OSError:  # library not built: the same bytes from the Python container code
            factors = split_factors(Uh[0], Vh[0], (H, W), ranks)
    return pack_image(factors, (H, W), ranks, bounds, patch_size, str(image.dtype).split(".")[-1])


def anyshape_ranks(image_hw, patch_size, rank=None, quality=None, chroma=None):
    """Ranks of (Y, Cb, Cr) for patches `patch_size` (lrf/compression/qmf.py:244-250) or, with patch_size None,
    for patch=False (:268-274): max(round(min(M, N) * quality / 100), 1) on the matrix each plane becomes."""
    H, W = image_hw
    if not isinstance(rank, Iterable):
        rank = (None, None, None) if rank is None else (rank, max(rank // 2, 1), max(rank // 2, 1))
    if not isinstance(quality, Iterable):
        quality = (None, None, None) if quality is None else (quality, quality / 2, quality / 2)
    out = []
    for i, d in enumerate(_lib.plane_dims_any(H, W, patch_size, chroma)):
        if rank[i] is None:
            assert quality[i] >= 0 and quality[i] <= 100, "'quality' must be between 0 and 100."
            out.append(max(round(min(d[4], d[5]) * quality[i] / 100), 1))
        else:
            out.append(rank[i])
    return out


def _qmf_encode_anyshape(ctx, dev, rank, quality, bounds, int_bounds, patch_size, num_iters, init_sign, init, chroma=None):
    """qmf_encode(color_space="YCbCr") with a patch size other than 8x8 (lrf/compression/qmf.py:232-262) or with
    patch=False (patch_size None, :264-286) for a batch dev [B,3,H,W]: per plane one matrix [M, N] per image, all images
    of a plane factorised in one call of the any-shape kernels.  Returns one byte stream per image.
    `init`: optional three (u0, v0) fp32 pairs ([M,R] / [N,R], or with a leading batch axis) replacing the SVD
    initialisation (tests); `init_sign`: [R0+R1+R2] or [B, R0+R1+R2]."""
    B = dev.shape[0]
    H, W = dev.shape[-2:]
    dims = _lib.plane_dims_any(H, W, patch_size, chroma)
    ranks = anyshape_ranks((H, W), patch_size, rank, quality, chroma)
    # Small calls: the three planes on three contexts / streams.  These kernels give a matrix to one workgroup, so one image
    # keeps a CU or two busy per plane and its latency is the SUM of the planes' chains unless they run side by side (one
    # 512x768 image without patches: 57 -> 45 ms); a large batch fills the chip by itself (three streams: no gain).
    side_by_side = B <= 8 and torch.cuda.is_available()
    offs = [sum(ranks[:c]) for c in range(3)]

    def one_plane(pctx, c):
        X = pctx.planes_any(dev, patch_size, c, chroma)
        R = ranks[c]
        sign = None
        if init_sign is not None:
            sg = torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1, sum(ranks))[:, offs[c]:offs[c] + R]
            sign = sg.expand(B, R).contiguous().cuda(dev.device)
        if init is not None:
            u0 = torch.as_tensor(init[c][0], dtype=torch.float32).reshape(-1, dims[c][4], R).expand(B, -1, -1).contiguous().cuda(dev.device)
            v0 = torch.as_tensor(init[c][1], dtype=torch.float32).reshape(-1, dims[c][5], R).expand(B, -1, -1).contiguous().cuda(dev.device)
            u, v = (u0.cpu().to(torch.int8), v0.cpu().to(torch.int8)) if num_iters == 0 else \
                pctx.bcd(X, u0, v0, num_iters, int_bounds[0], int_bounds[1])
        elif num_iters == 0:  # the float factors go straight through torch's truncating cast (qmf.py:258-260)
            u0, v0 = pctx.svd_init(X, R, sign)
            u, v = u0.cpu().to(torch.int8), v0.cpu().to(torch.int8)
        else:
            u, v = pctx.decompose(X, R, num_iters, int_bounds[0], int_bounds[1], sign)
        return u, v, X  # X: kept alive until its stream has been waited for

    if side_by_side:
        ctxs, lanes = _plane_lanes(dev.device)
        cur = torch.cuda.current_stream(dev.device)
        pending = []
        for c in range(3):
            lanes[c].wait_stream(cur)
            with torch.cuda.stream(lanes[c]):
                pending.append(one_plane(ctxs[c], c))
        for c in range(3):
            cur.wait_stream(lanes[c])
        per_plane = [(u.cpu().numpy(), v.cpu().numpy()) for u, v, _ in pending]  # [B, M, R], [B, N, R]
    else:
        per_plane = []
        for c in range(3):
            u, v, _ = one_plane(ctx, c)
            per_plane.append((u.cpu().numpy(), v.cpu().numpy()))
    dtype_name = str(dev.dtype).split(".")[-1]
    try:  # the containers of the whole batch on native host threads (a column, or a whole factor, per work item)
        return pack_anyshape_native(per_plane, (H, W), ranks, bounds, patch_size, dtype_name, chroma)
    except OSError:  # liblrf_pack.so absent or linked against another zlib: the Python container code, same bytes
        pass
    streams = []
    for b in range(B):
        factors = []
        for u, v in per_plane:
            # patch=False keeps the plane's channel axis: the factors are 3-D there (qmf.py:281-282), 2-D with patches
            factors += [u[b:b + 1], v[b:b + 1]] if patch_size is None else [u[b], v[b]]
        streams.append(pack_anyshape(factors, (H, W), ranks, bounds, patch_size, dtype_name, chroma))
    return streams


def _qmf_encode_general(ctx, dev, color_space, rank, quality, bounds, patch_size, num_iters, init_sign, init, chroma, qmf_opts):
    """qmf_encode with QMF options beyond the tuned configuration — `l2`, `l1_ratio`, `eps`, `num_levels`, which the
    reference forwards to QMF(rank, bounds, factor=(0, 1), **kwargs) per matrix (lrf/compression/qmf.py:189, 208, 256, 280) —
    for one image dev [1,3,H,W]: the same matrices as the other branches (any patch size, patch=False, both colour spaces),
    each through lrf_amd.QMF's general path (lrf_qmf_decompose_ex_f32), the float factors through torch's cast to int8
    (qmf.py:258-260) and the same container.  `init`: per matrix an (u0, v0) pair replacing the SVD initialisation (tests)."""
    from .factorization import QMF
    H, W = dev.shape[-2:]
    if color_space == "RGB":
        if isinstance(rank, (list, tuple)) or isinstance(quality, (list, tuple)):
            raise ValueError("color_space='RGB' takes a scalar rank / quality")
        Hp, Wp, M, N = _lib.rgbspace_dims_any(H, W, patch_size)
        if rank is None:
            assert quality >= 0 and quality <= 100, "'quality' must be between 0 and 100."
            R = max(round(min(M, N) * quality / 100), 1)
        else:
            R = rank
        X = ctx.rgbspace_matrix_any(dev, patch_size)
        mats = [X[0]] if patch_size is None else [X]  # [3, H, W]: three matrices in one call; [1, M, N]: one
        ranks = [R]
    else:
        ranks = anyshape_ranks((H, W), patch_size, rank, quality, chroma)
        mats = [ctx.planes_any(dev, patch_size, c, chroma) for c in range(3)]
    offs = [sum(ranks[:c]) for c in range(len(ranks))]
    factors = []
    for c, (Xc, R) in enumerate(zip(mats, ranks)):
        nb = Xc.shape[0]
        sign = None
        if init_sign is not None:
            sign = torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1, sum(ranks))[:, offs[c]:offs[c] + R].expand(nb, R).contiguous()
        opts = dict(qmf_opts)
        num_levels = opts.pop("num_levels", None)
        if init is not None:  # the reference's initial factors (fixtures): straight into the general loop
            u0 = torch.as_tensor(init[c][0], dtype=torch.float32).reshape(nb, Xc.shape[1], R)
            v0 = torch.as_tensor(init[c][1], dtype=torch.float32).reshape(nb, Xc.shape[2], R)
            w0 = None if len(init[c]) < 3 else torch.as_tensor(init[c][2], dtype=torch.float32).reshape(1, 2).expand(nb, 2)
            if num_iters == 0:
                u, v = u0, v0
            else:
                u, v, _ = ctx.decompose_ex(Xc, R, num_iters, bounds, opts.get("l2", 0), opts.get("l1_ratio", 0), (0, 1), None,
                                           init=(u0, v0), eps=opts.get("eps", 1e-16), w_init=w0)
        else:
            u, v, _ = QMF(rank=R, num_iters=num_iters, bounds=bounds, num_levels=num_levels, factor=(0, 1), init_sign=sign,
                          **opts).decompose(Xc)
        u8, v8 = u.cpu().to(torch.int8).numpy(), v.cpu().to(torch.int8).numpy()  # the affine pair w is dropped, as at qmf.py:257
        if color_space == "RGB":
            factors += [u8[0], v8[0]] if patch_size is not None else [u8, v8]
        else:
            factors += [u8[0:1], v8[0:1]] if patch_size is None else [u8[0], v8[0]]
    dtype_name = str(dev.dtype).split(".")[-1]
    if color_space == "RGB":
        metadata = {"dtype": dtype_name, "color space": "RGB", "patch": patch_size is not None, "bounds": bounds}
        if patch_size is not None:
            metadata.update({"patch size": patch_size, "original size": [H, W], "padded size": [Hp, Wp], "rank": ranks[0]})
        else:
            metadata["rank"] = ranks[0]
        return combine_bytes([dict_to_bytes(metadata), combine_bytes([encode_tensor(np.ascontiguousarray(f)) for f in factors])])
    return pack_anyshape(factors, (H, W), ranks, bounds, patch_size, dtype_name, chroma)


_PLANE_LANES = {}
_PLANE_LANES_LOCK = __import__("threading").Lock()


def _plane_lanes(device):
    """three contexts and three streams per (host thread, device) for the plane-parallel small calls of _qmf_encode_anyshape.
    They are released again (release_plane_lanes) before this thread's pipelined batch encoder runs: every extra context /
    stream alive in the process costs the pipe's schedule (one unused context and two streams moved
    256 x 512x768 host -> host from 6.1 to 7-9 ms), and a lane's workspace is a few hundred MB after a large patch=False call."""
    import threading
    key = (threading.get_ident(), torch.device(device).index or 0)
    with _PLANE_LANES_LOCK:
        lanes = _PLANE_LANES.get(key)
    if lanes is None:
        lanes = ([_lib.Context(key[1]) for _ in range(3)], [torch.cuda.Stream(device=key[1]) for _ in range(3)])
        with _PLANE_LANES_LOCK:
            _PLANE_LANES[key] = lanes
    return lanes


def release_plane_lanes(all_threads: bool = False) -> int:
    """Destroys the plane lanes of the calling thread: their contexts (workspaces, streams) and torch streams.  Called by
    qmf_encode_batch's host path; safe to call any time (the lanes are re-created on demand).  all_threads=True also takes
    the lanes of OTHER threads — only for a quiescent process (tests, shutdown): a lane another thread is encoding on would
    be closed under it.  Returns the number of lane sets released."""
    import threading
    me = threading.get_ident()
    n = 0
    with _PLANE_LANES_LOCK:
        mine = [(k, _PLANE_LANES.pop(k)) for k in list(_PLANE_LANES) if all_threads or k[0] == me]
    for key, (ctxs, lanes) in mine:
        for st in lanes:
            st.synchronize()
        for c in ctxs:
            c.close()
        n += 1
    return n


def pack_anyshape(factors, image_hw, ranks, bounds, patch_size, dtype_name="uint8", chroma=None) -> bytes:
    """Byte stream of the patch-size / patch=False branches (metadata keys in the reference's order, qmf.py:157-162,
    233-254, 265-277, 288-290).  factors: [u_y, v_y, u_cb, v_cb, u_cr, v_cr] int8, 2-D with patches, [1, rows, R]
    without (the reference keeps the plane's channel axis there and encode_tensor stores such tensors whole)."""
    metadata = anyshape_metadata(image_hw, ranks, bounds, patch_size, dtype_name, chroma)
    return combine_bytes([dict_to_bytes(metadata), combine_bytes([encode_tensor(np.ascontiguousarray(f)) for f in factors])])


def _qmf_decode_anyshape(encoded_image: bytes, device=None) -> torch.Tensor:
    """YCbCr branch of qmf_decode for any patch size / patch=False (qmf.py:325-351) -> uint8 CUDA tensor [3,H,W]."""
    encoded_metadata, encoded_factors = separate_bytes(encoded_image, 2)
    metadata = bytes_to_dict(encoded_metadata)
    if metadata["dtype"] != "uint8":
        raise NotImplementedError("HIP decode writes uint8 images")
    patch_size = tuple(metadata["patch size"]) if metadata["patch"] else None
    f = [decode_tensor(x) for x in separate_bytes(encoded_factors, 6)]
    H, W = metadata["original size"][0]
    chroma = tuple(int(v) for v in metadata["original size"][1])  # any scale_factor: the stream carries the plane sizes
    if chroma == (H // 2, W // 2):
        chroma = None
    dims = _lib.plane_dims_any(H, W, patch_size, chroma)
    for c in range(3):
        if list(metadata["original size"][c]) != [dims[c][0], dims[c][1]] or \
                (patch_size is not None and list(metadata["padded size"][c]) != [dims[c][2], dims[c][3]]):
            raise ValueError("stream geometry is not the reflect-padded layout its plane sizes imply (Cb and Cr must agree)")
        if tuple(f[2 * c].shape[-2:]) != (dims[c][4], f[2 * c].shape[-1]) or tuple(f[2 * c + 1].shape[-2:]) != (dims[c][5], f[2 * c].shape[-1]):
            raise ValueError("stream factors do not match the plane geometry its metadata describes")
    ctx = _lib.context(device)
    Us, Vs = [], []
    for c in range(3):
        u = np.array(f[2 * c], dtype=np.int8)  # copies: decode_tensor may hand back read-only views
        v = np.array(f[2 * c + 1], dtype=np.int8)
        Us.append(torch.from_numpy(u.reshape(1, dims[c][4], -1)).cuda(ctx.device))
        Vs.append(torch.from_numpy(v.reshape(1, dims[c][5], -1)).cuda(ctx.device))
    return ctx.decode_any(Us, Vs, H, W, patch_size, chroma)[0]


def rgbspace_dims(H, W):
    """(Hp, Wp, M) of the RGB colour-space branch: reflect padding to multiples of 8, one row per 8x8 patch."""
    Hp, Wp = H + (8 - H % 8) % 8, W + (8 - W % 8) % 8
    return Hp, Wp, (Hp // 8) * (Wp // 8)


def _qmf_encode_rgbspace(ctx, dev, rank, quality, bounds, int_bounds, patch_size, num_iters, init_sign, init):
    """qmf_encode(color_space="RGB") (lrf/compression/qmf.py:164-212, 288-290): with patches one [M, 3 p q] matrix per image,
    without (patch_size None) the three channel planes as matrices [3, H, W].  8x8 patches with num_iters >= 1 run on the
    fused entry point; the other forms go matrix -> lrf_qmf_decompose_f32 / _bcd_f32 / _svd_init_f32 (any shape)."""
    if isinstance(rank, (list, tuple)) or isinstance(quality, (list, tuple)):
        raise ValueError("color_space='RGB' takes a scalar rank / quality")
    H, W = dev.shape[-2:]
    Hp, Wp, M, N = _lib.rgbspace_dims_any(H, W, patch_size)
    if rank is None:
        assert quality >= 0 and quality <= 100, "'quality' must be between 0 and 100."
        R = max(round(min(M, N) * quality / 100), 1)
    else:
        R = rank
    nmat = 1 if patch_size is not None else 3
    sign = None if init_sign is None else torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1, R).expand(nmat, R).contiguous()
    metadata = {"dtype": str(dev.dtype).split(".")[-1], "color space": "RGB", "patch": patch_size is not None, "bounds": bounds}
    if patch_size is not None:
        metadata.update({"patch size": patch_size, "original size": [H, W], "padded size": [Hp, Wp], "rank": R})
    else:
        metadata["rank"] = R
    if patch_size is not None and tuple(patch_size) == (8, 8) and num_iters >= 1:
        U, V = ctx.qmf_rgbspace_encode(dev, R, num_iters, int_bounds, sign, init)
        factors = [U[0].cpu().numpy(), V[0].cpu().numpy()]
    else:
        X = ctx.rgbspace_matrix_any(dev, patch_size)
        X = X[0] if patch_size is None else X  # [3, H, W]: three matrices; [1, M, N]: one
        if init is not None:
            u0 = torch.as_tensor(init[0], dtype=torch.float32).reshape(nmat, M, R).contiguous().cuda(dev.device)
            v0 = torch.as_tensor(init[1], dtype=torch.float32).reshape(nmat, N, R).contiguous().cuda(dev.device)
        elif num_iters == 0 or init is None:
            u0 = v0 = None
        sg = None if sign is None else sign.cuda(dev.device)
        if num_iters == 0:  # the float factors go straight through torch's truncating cast (qmf.py:188, 210)
            if init is None:
                u0, v0 = ctx.svd_init(X, R, sg)
            u, v = u0.cpu().to(torch.int8), v0.cpu().to(torch.int8)
        elif init is not None:
            u, v = ctx.bcd(X, u0, v0, num_iters, int_bounds[0], int_bounds[1])
        else:
            u, v = ctx.decompose(X, R, num_iters, int_bounds[0], int_bounds[1], sg)
        u, v = u.cpu().numpy(), v.cpu().numpy()
        factors = [u[0], v[0]] if patch_size is not None else [u, v]  # patch=False keeps the channel axis (qmf.py:208-210)
    return combine_bytes([dict_to_bytes(metadata), combine_bytes([encode_tensor(np.ascontiguousarray(f)) for f in factors])])


def _two_factor_metadata(dtype_name, bounds, patch_size, hw, padded, R) -> bytes:
    """the metadata block of a two-factor container (qmf.py:180-187, 204-212)"""
    metadata = {"dtype": dtype_name, "color space": "RGB", "patch": patch_size is not None, "bounds": bounds}
    if patch_size is not None:
        metadata.update({"patch size": patch_size, "original size": list(hw), "padded size": list(padded), "rank": R})
    else:
        metadata["rank"] = R
    return dict_to_bytes(metadata)


def _two_factor_stream(dtype_name, bounds, patch_size, hw, padded, R, factors) -> bytes:
    """the container of the RGB colour-space branch (qmf.py:180-187, 204-212): its metadata, a scalar rank and two factors"""
    return combine_bytes([_two_factor_metadata(dtype_name, bounds, patch_size, hw, padded, R),
                          combine_bytes([encode_tensor(np.ascontiguousarray(f)) for f in factors])])


def _qmf_encode_channels(ctx, dev, rank, quality, bounds, int_bounds, patch_size, num_iters, init_sign, init):
    """qmf_encode(color_space="RGB") of one image dev [1,C,H,W] with C != 3 (the reference infers c: lrf/compression/qmf.py:43-56,
    164-212).  C = 1 with 8x8 patches and num_iters >= 1 is one [M,64] matrix, the shape of the tuned kernels: one
    lrf_qmf_encode_gray_u8 call.  Every other form goes matrix (lrf_qmf_chan_matrix_u8) -> lrf_qmf_decompose_f32 / _bcd_f32 /
    _svd_init_f32 (any shape), as _qmf_encode_rgbspace does for three channels."""
    if isinstance(rank, (list, tuple)) or isinstance(quality, (list, tuple)):
        raise ValueError("color_space='RGB' takes a scalar rank / quality")
    C, H, W = dev.shape[-3:]
    Hp, Wp, M, N = _lib.chan_dims(H, W, C, patch_size)
    R = _lib.chan_rank(M, N, rank, quality)
    nmat = 1 if patch_size is not None else C
    sign = None if init_sign is None else torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1, R).expand(nmat, R).contiguous()
    u0 = v0 = None
    if init is not None:
        u0 = torch.as_tensor(init[0], dtype=torch.float32).reshape(nmat, M, R).contiguous().cuda(dev.device)
        v0 = torch.as_tensor(init[1], dtype=torch.float32).reshape(nmat, N, R).contiguous().cuda(dev.device)
    if C == 1 and patch_size == (8, 8) and num_iters >= 1:
        U, V = ctx.encode_gray(dev[:, 0], R, num_iters, int_bounds, sign, None if init is None else (u0, v0))
        Uh, Vh = ctx.to_host(U, V)
        factors = [Uh[0].numpy(), Vh[0].numpy()]
    else:
        X = ctx.chan_matrix(dev, patch_size)
        X = X[0] if patch_size is None else X  # [C, H, W]: C matrices; [1, M, N]: one
        sg = None if sign is None else sign.cuda(dev.device)
        if num_iters == 0:  # the float factors go straight through torch's truncating cast (qmf.py:188, 210)
            if init is None:
                u0, v0 = ctx.svd_init(X, R, sg)
            u, v = u0.cpu().to(torch.int8), v0.cpu().to(torch.int8)
        elif init is not None:
            u, v = ctx.to_host(*ctx.bcd(X, u0, v0, num_iters, int_bounds[0], int_bounds[1]))
        else:
            u, v = ctx.to_host(*ctx.decompose(X, R, num_iters, int_bounds[0], int_bounds[1], sg))
        u, v = u.numpy(), v.numpy()
        factors = [u[0], v[0]] if patch_size is not None else [u, v]  # patch=False keeps the channel axis (qmf.py:208-210)
    return _two_factor_stream(str(dev.dtype).split(".")[-1], bounds, patch_size, (H, W), (Hp, Wp), R, factors)


def _qmf_encode_batch_gray(images, rank, quality, bounds, num_iters, init_sign, pack_workers, patch, patch_size, deflate) -> list:
    """qmf_encode_batch(color_space="RGB") of gray images [B,1,H,W]: ONE lrf_qmf_encode_gray_u8 call, then the Python container
    code on the pack pool (zlib releases the GIL) -> the streams qmf_encode(images[i], color_space="RGB") gives."""
    if deflate not in ("host", "device"):
        raise ValueError(f"deflate must be 'host' or 'device', got {deflate!r}")
    if deflate == "device":
        raise NotImplementedError("deflate='device' is not served by qmf_encode_batch(color_space='RGB'): qmf_encode_ragged(color_space='RGB', "
                                  "deflate='device') folds the device coder's columns into two-factor containers")
    if images.dim() != 4 or images.shape[1] != 1:
        raise NotImplementedError(f"qmf_encode_batch(color_space='RGB') serves gray images [B,1,H,W], got {tuple(images.shape)}: "
                                  "other channel counts go one by one through qmf_encode")
    if not patch or tuple(patch_size) != (8, 8):
        raise NotImplementedError("qmf_encode_batch(color_space='RGB') serves 8x8 patches only: other patch settings go one by one "
                                  "through qmf_encode")
    if images.dtype != torch.uint8:
        raise NotImplementedError("HIP path takes uint8 images")
    if num_iters < 1:
        raise NotImplementedError("qmf_encode_batch(color_space='RGB') needs num_iters >= 1")
    if isinstance(rank, (list, tuple)) or isinstance(quality, (list, tuple)):
        raise ValueError("color_space='RGB' takes a scalar rank / quality")
    B, _, H, W = images.shape
    Hp, Wp, M, N = _lib.chan_dims(H, W, 1, (8, 8))
    R = _lib.chan_rank(M, N, rank, quality)
    ctx = _lib.context(images.device.index if images.is_cuda else None)
    dev = images if images.is_cuda else images.cuda(ctx.device)
    sign = None if init_sign is None else torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1, R).expand(B, R).contiguous()
    U, V = ctx.encode_gray(dev[:, 0], R, num_iters, (math.ceil(bounds[0]), math.floor(bounds[1])), sign)
    Uh, Vh = (t.numpy() for t in ctx.to_host(U, V))
    dtype_name = str(images.dtype).split(".")[-1]

    def pack(b):
        return _two_factor_stream(dtype_name, bounds, (8, 8), (H, W), (Hp, Wp), R, [Uh[b], Vh[b]])

    import os
    workers = abs(pack_workers) if isinstance(pack_workers, int) and pack_workers else min(32, os.cpu_count() or 1)
    if workers <= 1 or B == 1:
        return [pack(b) for b in range(B)]
    return list(_pack_pool(workers).map(pack, range(B)))


# ---- gray image lists: ragged encode, target PSNR and byte budget (lrf_qmf_encode_gray_ragged_u8, _sweep_, lrf_qmf_sse_gray_ragged_u8)
def container_bytes_two_factor(meta_len, R, column_lengths):
    """len() of a two-factor container (_two_factor_stream's layout) whose columns are given streams, by host arithmetic: the
    metadata JSON of meta_len bytes, then two factors (u, v), each one JSON header {"num_fibers", "mode", "dtype"} in front of
    its R columns; combine_bytes puts four length bytes in front of every part but the last (container.py).  column_lengths:
    integers [..., 2 R] (an array or a tensor, on any device), the lengths of an image's column streams in any order -> their
    sum over the last axis plus the constant of (meta_len, R)."""
    R = int(R)
    lens = column_lengths if isinstance(column_lengths, torch.Tensor) else np.asarray(column_lengths, dtype=np.int64)
    if R < 1 or lens.shape[-1] != 2 * R:
        raise ValueError(f"container_bytes_two_factor: a rank >= 1 and 2 R column lengths expected, got {R} and {tuple(lens.shape)}")
    # the metadata's prefix, the prefix of u; per factor: the header and its prefix, a prefix for every column but the last
    const = 4 + int(meta_len) + 4 + 2 * (4 + _factor_header_len(R) + 4 * (R - 1))
    total = lens.sum(dim=-1, dtype=torch.int64) if isinstance(lens, torch.Tensor) else lens.sum(axis=-1, dtype=np.int64)
    return total + const


def _gray_factor_mats(sizes, ranks, u_off, v_off):
    """(src_off, rows, cols) of the factors of m gray streams, int64 [m, 2, 3]: U [M, R] then V [64, R]"""
    m = len(sizes)
    if m < 1 or not (len(ranks) == len(u_off) == len(v_off) == m):
        raise ValueError("one size, rank, u_off and v_off per stream expected")
    m_of = {}
    for hw in sizes:
        if tuple(hw) not in m_of:
            m_of[tuple(hw)] = _lib.chan_dims(int(hw[0]), int(hw[1]), 1, (8, 8))[2]
    mats = np.empty((m, 2, 3), dtype=np.int64)
    mats[:, 0, 0] = np.asarray(u_off, dtype=np.int64)
    mats[:, 0, 1] = [m_of[tuple(hw)] for hw in sizes]
    mats[:, 1, 0] = np.asarray(v_off, dtype=np.int64)
    mats[:, 1, 1] = 64
    mats[:, :, 2] = np.asarray(ranks, dtype=np.int64).reshape(m, 1)
    if mats[:, :, 2].min() < 1:
        raise ValueError("ranks must be >= 1")
    return mats


def _gray_metadata(hw, R, bounds) -> bytes:
    Hp, Wp, _, _ = _lib.chan_dims(int(hw[0]), int(hw[1]), 1, (8, 8))
    return _two_factor_metadata("uint8", bounds, (8, 8), (int(hw[0]), int(hw[1])), (Hp, Wp), int(R))


def gray_streams_from_device_factors(ctx, U, V, sizes, ranks, u_off, v_off, bounds) -> list:
    """The way gray factors become streams with deflate="device": U, V flat int8 CUDA tensors holding n gray images of sizes[i] =
    (H, W) and rank ranks[i], U [M, R] at u_off[i] and V [64, R] at v_off[i].  Every column is deflated where it lies
    (ctx.deflate_columns_into, one call for the U matrices and one for the V matrices into the same slots and lengths), the
    slots and the lengths come to the host in one copy each, and the container code folds them: the column streams take the
    place of zlib.compress's output inside encode_tensor's layout.  The streams are not byte-identical to the zlib-9 ones; they
    hold the same factors and every inflate reads them."""
    n = len(sizes)
    mats = _gray_factor_mats(sizes, ranks, u_off, v_off)
    table, nbytes, ncols = _lib.deflate_table(mats.reshape(-1, 3))
    slots = torch.empty((nbytes,), dtype=torch.uint8, device=U.device)
    lens = torch.empty((ncols,), dtype=torch.int32, device=U.device)
    by_factor = table.reshape(n, 2, 5)
    ctx.deflate_columns_into(U.reshape(-1), by_factor[:, 0], slots, lens)
    ctx.deflate_columns_into(V.reshape(-1), by_factor[:, 1], slots, lens)
    slots_h, lens_h = (t.numpy() for t in ctx.to_host(slots, lens))
    col_off = _lib.deflate_column_offsets(table)
    blob = slots_h.tobytes()
    streams, at = [], 0
    for i in range(n):
        R = int(ranks[i])
        header = dict_to_bytes({"num_fibers": R, "mode": "col", "dtype": "int8"})
        factors = []
        for _ in range(2):
            cols = [blob[int(col_off[at + j]):int(col_off[at + j]) + int(lens_h[at + j])] for j in range(R)]
            factors.append(combine_bytes([header, combine_bytes(cols)]))
            at += R
        streams.append(combine_bytes([_gray_metadata(sizes[i], R, bounds), combine_bytes(factors)]))
    return streams


def qmf_stream_sizes_gray_ragged(U, V, sizes, ranks, u_off, v_off, bounds=(-16, 15)) -> torch.Tensor:
    """The exact length of the deflate="device" stream of every gray candidate, counted on the GPU without producing one.  U, V:
    flat int8 CUDA tensors holding m candidates of sizes[j] = (H, W) and rank ranks[j] at u_off[j] / v_off[j]
    (Context.encode_gray_ragged_sweep's layout, or encode_gray_ragged's) -> int64 CUDA tensor [m], out[j] = len() of the stream
    gray_streams_from_device_factors produces for candidate j.  One ctx.deflate_sizes count over all U matrices and one over all V
    matrices; the column lengths are summed per candidate on the device and container_bytes_two_factor adds the constant of the
    candidate's own metadata length and rank."""
    if not (isinstance(U, torch.Tensor) and isinstance(V, torch.Tensor) and U.dtype == torch.int8 and V.dtype == torch.int8):
        raise TypeError("factors must be int8 tensors")
    m = len(sizes)
    mats = _gray_factor_mats(sizes, ranks, u_off, v_off)
    Rs = mats[:, 0, 2]
    const_of = {}
    for hw, R in zip(sizes, Rs.tolist()):
        key = (int(hw[0]), int(hw[1]), R)
        if key not in const_of:
            const_of[key] = int(container_bytes_two_factor(len(_gray_metadata(hw, R, bounds)), R, np.zeros(2 * R, dtype=np.int64)))
    const = np.array([const_of[(int(hw[0]), int(hw[1]), R)] for hw, R in zip(sizes, Rs.tolist())], dtype=np.int64)
    ctx = _lib.context(U.device.index)
    out = torch.from_numpy(const).to(U.device)
    step = 1 << 20  # (lrf_deflate_sizes_i8 takes 2^20 matrices a call)
    for k in range(0, m, step):
        owner = torch.from_numpy(np.repeat(np.arange(k, min(k + step, m), dtype=np.int64), Rs[k:k + step])).to(U.device)
        for flat, which in ((U, 0), (V, 1)):
            out.index_add_(0, owner, ctx.deflate_sizes(flat.reshape(-1), mats[k:k + step, which]).to(torch.int64))
    return out


def _gray_image_list(images, name):
    """the images of a color_space="RGB" list call as a list of uint8 [1,H,W] tensors: a list or tuple of them, or a tensor
    [B,1,H,W]; refusals raised before a GPU is asked for"""
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError(f"{name}(color_space='RGB') takes a list of [1,H,W] images or a tensor [B,1,H,W], got a tensor of shape {tuple(images.shape)}")
        images = list(images)
    if isinstance(images, (bytes, str)) or not isinstance(images, (list, tuple)) or len(images) < 1:
        raise ValueError(f"{name} takes a non-empty sequence of images")
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor):
            raise TypeError(f"{name}: image {i} is {type(im).__name__}, not a tensor")
        if im.dtype != torch.uint8:
            raise NotImplementedError(f"{name}: image {i} is {im.dtype}; the HIP path takes uint8 images")
        if im.dim() == 3 and im.shape[0] == 3:
            raise NotImplementedError(f"{name}(color_space='RGB') serves gray images [1,H,W], image {i} is {tuple(im.shape)}: other channel "
                                      "counts go one by one through qmf_encode")
        if im.dim() != 3 or im.shape[0] != 1 or im.shape[1] < 1 or im.shape[2] < 1:
            raise ValueError(f"{name}: image {i} must be [1,H,W], got {tuple(im.shape)}")
    if len({im.device for im in images}) != 1:
        raise ValueError(f"{name}: the images of a list must all be on the host or all on one device, got {sorted({str(im.device) for im in images})}")
    return list(images)


def _check_encode_gray_ragged_args(images, rank, quality, ranks, num_iters, init_sign):
    """qmf_encode_ragged(color_space="RGB")'s refusals, raised before a GPU is asked for -> (images as a list, [(H, W)], [rank per
    image], [sign per image: None or int8 array])"""
    name = "qmf_encode_ragged"
    if ranks is not None:
        raise ValueError("qmf_encode_ragged(color_space='RGB'): 'ranks' is refused, a gray stream has a scalar rank (give 'rank' or 'quality')")
    images = _gray_image_list(images, name)
    n = len(images)
    if num_iters < 1:
        raise NotImplementedError("qmf_encode_ragged: num_iters = 0 (the truncated initialisation) is outside the fused encoder (qmf_encode takes it)")
    if (rank is None) == (quality is None):
        raise ValueError("qmf_encode_ragged(color_space='RGB'): give exactly one of 'rank' and 'quality'")
    scalar = lambda v: not isinstance(v, Iterable)
    rank_l = _per_image(rank, n, "rank", scalar)
    quality_l = _per_image(quality, n, "quality", scalar)
    sizes = [(int(im.shape[1]), int(im.shape[2])) for im in images]
    Rs = []
    for i, hw in enumerate(sizes):
        if not scalar(rank_l[i]) or not scalar(quality_l[i]):
            raise ValueError(f"qmf_encode_ragged(color_space='RGB'): image {i}: a scalar rank / quality expected")
        if hw[0] * hw[1] >= 2 ** 31:
            raise NotImplementedError(f"qmf_encode_ragged: image {i} of {hw[0]}x{hw[1]} has 2^31 pixels or more")
        M = _lib.chan_dims(hw[0], hw[1], 1, (8, 8))[2]
        R = int(_lib.chan_rank(M, 64, rank_l[i], quality_l[i]))
        if R < 1:
            raise ValueError(f"qmf_encode_ragged: image {i}: rank {R} must be >= 1")
        Rs.append(R)
    one_sign = lambda v: isinstance(v, (np.ndarray, torch.Tensor)) or (len(v) > 0 and all(x is not None and scalar(x) for x in v))
    signs = []
    for i, sg in enumerate(_per_image(init_sign, n, "init_sign", one_sign)):
        if sg is not None:
            sg = np.ascontiguousarray(torch.as_tensor(sg, dtype=torch.int8).reshape(-1).numpy())
            if sg.size != Rs[i]:
                raise ValueError(f"qmf_encode_ragged: image {i}: init_sign holds {sg.size} signs, its rank needs {Rs[i]}")
        signs.append(sg)
    return images, sizes, Rs, signs


def _gray_flat(images, idxs, sizes, dev):
    """the images idxs of the list in one flat device buffer, each at a multiple of 16 bytes (so that widths that are multiples
    of 16 keep the planes body made for them); host images go through one page-locked buffer and one copy -> (flat, offsets)"""
    offs, off = [], 0
    for i in idxs:
        offs.append(off)
        off = (off + sizes[i][0] * sizes[i][1] + 15) // 16 * 16
    if images[idxs[0]].is_cuda:
        flat = torch.empty((off,), dtype=torch.uint8, device=dev)
        for i, o in zip(idxs, offs):
            flat[o:o + images[i].numel()].view(images[i].shape).copy_(images[i])
    else:
        stage = torch.empty((off,), dtype=torch.uint8).pin_memory()
        for i, o in zip(idxs, offs):
            stage[o:o + images[i].numel()].view(images[i].shape).copy_(images[i])
        flat = stage.to(dev, non_blocking=True)
    return flat, offs


def _gray_host_streams(Uh, Vh, sizes, ranks, u_off, v_off, bounds, pack_workers) -> list:
    """the zlib-9 containers of gray factors on the host: _two_factor_stream per image on the pack pool, as _qmf_encode_batch_gray"""
    def pack(k):
        H, W = sizes[k]
        Hp, Wp, M, _ = _lib.chan_dims(H, W, 1, (8, 8))
        R = ranks[k]
        return _two_factor_stream("uint8", bounds, (8, 8), (H, W), (Hp, Wp), R,
                                  [Uh[u_off[k]:u_off[k] + M * R].reshape(M, R), Vh[v_off[k]:v_off[k] + 64 * R].reshape(64, R)])

    import os
    workers = abs(pack_workers) if isinstance(pack_workers, int) and pack_workers else min(32, os.cpu_count() or 1)
    if workers <= 1 or len(sizes) == 1:
        return [pack(k) for k in range(len(sizes))]
    return list(_pack_pool(workers).map(pack, range(len(sizes))))


def _qmf_encode_ragged_gray(images, rank, quality, ranks, bounds, num_iters, init_sign, pack_workers, deflate) -> list:
    """qmf_encode_ragged(color_space="RGB"): a list of gray images [1,H_i,W_i] (or a tensor [B,1,H,W]) of differing sizes and
    ranks in ONE lrf_qmf_encode_gray_ragged_u8 call -> stream i byte-identical to qmf_encode_batch(images[i][None], ...,
    color_space="RGB")[0].  Images of rank above 32 go one by one through that call and are put back in place."""
    if deflate not in ("host", "device"):
        raise ValueError(f"deflate must be 'host' or 'device', got {deflate!r}")
    images, sizes, Rs, signs = _check_encode_gray_ragged_args(images, rank, quality, ranks, num_iters, init_sign)
    n = len(images)
    streams = [None] * n
    fused = [i for i in range(n) if Rs[i] <= 32]
    ctx = _lib.context(images[0].device.index if images[0].is_cuda else None)
    dev = torch.device("cuda", ctx.device)
    lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
    for i in range(n):
        if Rs[i] <= 32:
            continue
        if deflate == "device":  # (the batch call packs on the host only: its factors, the device coder's columns)
            sg = None if signs[i] is None else torch.from_numpy(signs[i]).reshape(1, -1)
            U1, V1 = ctx.encode_gray(images[i].to(dev), Rs[i], num_iters, (lo, hi), sg)
            streams[i] = gray_streams_from_device_factors(ctx, U1.reshape(-1), V1.reshape(-1), [sizes[i]], [Rs[i]], [0], [0], bounds)[0]
        else:
            streams[i] = qmf_encode_batch(images[i][None], rank=Rs[i], bounds=bounds, num_iters=num_iters, init_sign=signs[i], pack_workers=pack_workers,
                                          color_space="RGB")[0]
    if not fused:
        return streams
    flat, offs = _gray_flat(images, fused, sizes, dev)
    sign, sign_offs = None, [-1] * len(fused)
    if any(signs[i] is not None for i in fused):
        so = 0
        for k, i in enumerate(fused):
            if signs[i] is not None:
                sign_offs[k] = so
                so += signs[i].size
        sign = torch.from_numpy(np.concatenate([signs[i] for i in fused if signs[i] is not None])).to(dev)
    U, V, u_off, v_off = ctx.encode_gray_ragged(flat, [(sizes[i][0], sizes[i][1], Rs[i], o, s) for i, o, s in zip(fused, offs, sign_offs)],
                                                num_iters, lo, hi, sign)
    f_sizes, f_ranks = [sizes[i] for i in fused], [Rs[i] for i in fused]
    if deflate == "device":
        packed = gray_streams_from_device_factors(ctx, U, V, f_sizes, f_ranks, u_off, v_off, bounds)
    else:
        Uh, Vh = (t.numpy() for t in ctx.to_host(U, V))  # waits for the stream, then raises if a launch of this call gave up
        packed = _gray_host_streams(Uh, Vh, f_sizes, f_ranks, u_off, v_off, bounds, pack_workers)
    for i, s_ in zip(fused, packed):
        streams[i] = s_
    return streams


def gray_target_candidates(image_hw, qualities):
    """The ranks a quality grid gives on a gray H x W image, each once, in ascending quality, with the LOWEST quality that gives
    it: ([rank], [quality])"""
    M = _lib.chan_dims(int(image_hw[0]), int(image_hw[1]), 1, (8, 8))[2]
    ranks, lowest = [], []
    for q in sorted(qualities):
        r = int(_lib.chan_rank(M, 64, None, q))
        if r not in ranks:
            ranks.append(r)
            lowest.append(q)
    return ranks, lowest


def _check_gray_rate_list_args(images, qualities, num_iters, name):
    """what qmf_encode_target / qmf_encode_budget (color_space="RGB") refuse about images, qualities and num_iters, before a GPU is
    asked for -> (images as a list, qualities as a list, [(H, W)], per image (ranks, lowest, rows): what gray_target_candidates
    gives for its size and, per quality in ascending order, which of the ranks it has)"""
    images = _gray_image_list(images, name)
    if num_iters < 1:
        raise NotImplementedError(f"{name}: num_iters = 0 (the truncated initialisation) is outside the fused sweep")
    qualities = list(qualities)
    if not qualities or any(not (0 <= q <= 100) for q in qualities):
        raise ValueError(f"{name}: 'qualities' must be a non-empty sequence of numbers between 0 and 100")
    sizes = [(int(im.shape[1]), int(im.shape[2])) for im in images]
    per_size = {}
    for i, hw in enumerate(sizes):
        if hw in per_size:
            continue
        if hw[0] * hw[1] >= 2 ** 31:
            raise NotImplementedError(f"{name}: image {i} of {hw[0]}x{hw[1]} has 2^31 pixels or more")
        M = _lib.chan_dims(hw[0], hw[1], 1, (8, 8))[2]
        for q in sorted(qualities):
            r = int(_lib.chan_rank(M, 64, None, q))
            if r > 32:
                raise NotImplementedError(f"{name}: image {i} ({hw[0]}x{hw[1]}) at quality {q} has rank {r}: a gray list takes ranks up to 32 "
                                          f"(encode such images through qmf_encode_batch(color_space='RGB'))")
        ranks, lowest = gray_target_candidates(hw, qualities)
        per_size[hw] = (ranks, lowest, [ranks.index(int(_lib.chan_rank(M, 64, None, q))) for q in sorted(qualities)])
    return images, qualities, sizes, [per_size[hw] for hw in sizes]


def _exact_goal(value):
    """a goal given as Python or numpy floats as a float64 tensor (torch.as_tensor alone makes a list of floats float32, and a
    target that sits exactly on a table value must stay there); everything else as it came"""
    if value is None or isinstance(value, torch.Tensor):
        return value
    a = np.asarray(value)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) if a.dtype.kind == "f" else value


def _rate_control_list_gray(images, name, goal, qualities, bounds, num_iters, pack_workers, on_device, x_workspace_bytes) -> dict:
    """qmf_encode_target / qmf_encode_budget with color_space="RGB": gray images of differing sizes (a list of [1,H,W], or a tensor
    [B,1,H,W], which goes the same way as the list of its images).  _rate_control_list's structure on the gray entries: per chunk
    of consecutive images (4 * 64 * M bytes of fp32 patch matrix each within x_workspace_bytes; one image at least) ONE ragged
    sweep encode of every (image, candidate rank), ONE ragged squared error straight from the factors, for the budget ONE ragged
    size count, the choice on the device (select_target / select_budget, unchanged), and only the winners packed."""
    from .metrics import bits_per_pixel, psnr_from_sse
    budget_mode = name == "qmf_encode_budget"
    images, qualities, sizes, cand_of = _check_gray_rate_list_args(images, qualities, num_iters, name)
    B = len(images)
    if budget_mode:
        goal_t = budget_bytes_per_image(sizes, _exact_goal(goal["bpp"]), _exact_goal(goal["nbytes"]))
    else:
        goal_t = _per_image_numbers(_exact_goal(goal["psnr"]), B, name, "psnr")
    if int(x_workspace_bytes) < 1:
        raise ValueError(f"{name}: x_workspace_bytes must be >= 1")
    sorted_q = sorted(qualities)
    x_bytes = [4 * 64 * _lib.chan_dims(hw[0], hw[1], 1, (8, 8))[2] for hw in sizes]
    chunks, at = [], 0
    while at < B:
        end, tot, ncand = at, 0, 0
        while end < B and (end == at or (tot + x_bytes[end] <= x_workspace_bytes and end - at < 65535 and ncand + len(cand_of[end][0]) <= 2 ** 20)):
            tot += x_bytes[end]
            ncand += len(cand_of[end][0])
            end += 1
        chunks.append(range(at, end))
        at = end
    ctx = _lib.context(images[0].device.index if images[0].is_cuda else None)
    dev = torch.device("cuda", ctx.device)
    lo, hi = math.ceil(bounds[0]), math.floor(bounds[1])
    streams, quality = [None] * B, [None] * B
    tables, size_tables, chosen, reached_all, counted_all = [], [], [], [], []
    for chunk in chunks:
        n = len(chunk)
        flat, offs = _gray_flat(images, list(chunk), sizes, dev)
        # the candidates, image after image in ascending quality, and row[q][k]: the candidate of (sorted quality q, image k)
        counts = np.array([len(cand_of[i][0]) for i in chunk], dtype=np.int64)
        first = np.cumsum(counts) - counts
        owner = np.repeat(np.arange(n, dtype=np.int64), counts).tolist()  # the image (within the chunk) of every candidate
        ranks = [r for i in chunk for r in cand_of[i][0]]
        row = first.reshape(1, n) + np.array([cand_of[i][2] for i in chunk], dtype=np.int64).T
        U, V, u_off, v_off = ctx.encode_gray_ragged_sweep(flat, [(sizes[i][0], sizes[i][1], o) for i, o in zip(chunk, offs)], list(zip(owner, ranks)),
                                                          num_iters, lo, hi, None)
        c_hw = [sizes[chunk[k]] for k in owner]
        sse_vec = ctx.sse_gray_ragged(flat, [(hw[0], hw[1], r, uo, vo, offs[k]) for hw, r, uo, vo, k in zip(c_hw, ranks, u_off, v_off, owner)], U, V)
        row_d = torch.from_numpy(row).to(dev)
        sse = sse_vec[row_d]
        samples = torch.tensor([sizes[i][0] * sizes[i][1] for i in chunk], dtype=torch.int64)  # (on the host: psnr_from_sse groups the columns by count)
        goal_c = goal_t[chunk.start:chunk.stop]
        if budget_mode:
            size = qmf_stream_sizes_gray_ragged(U, V, c_hw, ranks, u_off, v_off, bounds)[row_d]
            index, reached = select_budget(size, sse, goal_c)
            table = psnr_from_sse(sse, samples)[1]
            counted_all.append(size.gather(0, index.reshape(1, -1))[0].cpu())
            size_tables.append(size.cpu())
        else:
            table, index, reached = select_target(sse, samples, goal_c)
        chosen.append(table.gather(0, index.reshape(1, -1))[0].cpu())
        tables.append(table.cpu())
        reached_all.append(reached.cpu())
        index = index.cpu().tolist()
        win = [int(row[index[k], k]) for k in range(n)]
        w_sizes, w_ranks = [sizes[i] for i in chunk], [ranks[j] for j in win]
        if on_device:
            packed = gray_streams_from_device_factors(ctx, U, V, w_sizes, w_ranks, [u_off[j] for j in win], [v_off[j] for j in win], bounds)
        else:  # only the winners' factors come to the host: gathered back to back on the device first
            nus = [_lib.chan_dims(hw[0], hw[1], 1, (8, 8))[2] * r for hw, r in zip(w_sizes, w_ranks)]
            nvs = [64 * r for r in w_ranks]
            Uw = torch.cat([U[u_off[j]:u_off[j] + nu] for j, nu in zip(win, nus)])
            Vw = torch.cat([V[v_off[j]:v_off[j] + nv] for j, nv in zip(win, nvs)])
            Uh, Vh = (x.numpy() for x in ctx.to_host(Uw, Vw))  # waits for the stream, then raises if a launch of this call gave up
            packed = _gray_host_streams(Uh, Vh, w_sizes, w_ranks, np.cumsum([0] + nus[:-1]).tolist(), np.cumsum([0] + nvs[:-1]).tolist(), bounds,
                                        pack_workers)
        for k, i in enumerate(chunk):
            streams[i] = packed[k]
            quality[i] = sorted_q[index[k]]
    if budget_mode:
        counted = torch.cat(counted_all)
        for b, s_ in enumerate(streams):
            if len(s_) != int(counted[b]):
                raise RuntimeError(f"qmf_encode_budget: image {b} at quality {quality[b]}: the stream has {len(s_)} bytes, {int(counted[b])} were counted")
    row_of = [sorted_q.index(q) for q in qualities]
    out = {"streams": streams, "quality": quality, "psnr": torch.cat(chosen), "reached": torch.cat(reached_all),
           "table": torch.cat(tables, dim=1)[row_of]}
    if budget_mode:
        out["nbytes"] = counted
        out["bpp"] = torch.tensor([bits_per_pixel(hw, s_) for hw, s_ in zip(sizes, streams)], dtype=torch.float64)
        out["size_table"] = torch.cat(size_tables, dim=1)[row_of]
    return out


def _svd_init_factors(ctx, dev, ranks, init_sign):
    """num_iters=0 (experiments/ablation_numiters/eval.py:51): the float SVD factors go straight through `.to(int8)`
    (lrf/compression/qmf.py:258-260), i.e. torch's truncating cast, done here with torch itself on the host."""
    H, W = dev.shape[-2:]
    X = ctx.planes_from_rgb(dev)[0]
    factors, off, soff = [], 0, 0
    for (_, _, _, _, M), R in zip(_lib.plane_dims(H, W), ranks):
        x = X[off:off + M * 64].reshape(1, M, 64)
        off += M * 64
        sign = None
        if init_sign is not None:
            sign = torch.as_tensor(init_sign, dtype=torch.int8).reshape(-1)[soff:soff + R].reshape(1, R).contiguous().cuda(dev.device)
        soff += R
        u0, v0 = ctx.svd_init(x, R, sign)
        factors += [u0[0].cpu().to(torch.int8).numpy(), v0[0].cpu().to(torch.int8).numpy()]
    return factors


def parse_stream(encoded_image: bytes):
    """-> (metadata, [u_y, v_y, u_cb, v_cb, u_cr, v_cr]) for the YCbCr branch (lrf/compression/qmf.py:306-327)."""
    encoded_metadata, encoded_factors = separate_bytes(encoded_image, 2)
    metadata = bytes_to_dict(encoded_metadata)
    if metadata["color space"] != "YCbCr" or not metadata["patch"] or list(metadata["patch size"]) != [8, 8]:
        raise NotImplementedError("HIP decode covers the YCbCr / 8x8-patch branch only")
    factors = [decode_tensor(f) for f in separate_bytes(encoded_factors, 6)]
    return metadata, factors


def _factors_python(streams: Sequence[bytes]):
    """The streams' factors by this module's own container code, every shape checked against the stream's metadata
    -> (metadata of each stream, U [B, sum M_c R_c], V [B, 64 sum R_c]) as int8 arrays."""
    metas, Us, Vs = [], [], []
    for s in streams:
        meta, f = parse_stream(s)
        # a truncated or crafted stream must not reach the kernels: they index the factors from the metadata alone
        H0, W0 = meta["original size"][0]
        ranks0 = [int(r) for r in meta["rank"]]
        if len(ranks0) != 3 or min(ranks0) < 1:
            raise ValueError("stream metadata: 'rank' must hold three positive integers")
        for c, (d, R) in enumerate(zip(_lib.plane_dims(H0, W0), ranks0)):
            u, v = f[2 * c], f[2 * c + 1]
            if tuple(u.shape) != (d[4], R) or tuple(v.shape) != (64, R) or u.dtype != np.int8 or v.dtype != np.int8:
                raise ValueError(f"stream factors of plane {c} are {u.dtype}{tuple(u.shape)} / {v.dtype}{tuple(v.shape)}; "
                                 f"the metadata describes int8 {(d[4], R)} / {(64, R)}")
        metas.append(meta)
        Us.append(np.concatenate([np.ascontiguousarray(f[i], dtype=np.int8).ravel() for i in (0, 2, 4)]))
        Vs.append(np.concatenate([np.ascontiguousarray(f[i], dtype=np.int8).ravel() for i in (1, 3, 5)]))
    for m in metas[1:]:
        if m["original size"] != metas[0]["original size"] or m["rank"] != metas[0]["rank"]:
            raise ValueError("streams differ in geometry or ranks")
    return metas, np.stack(Us), np.stack(Vs)


def _factors_native(streams: Sequence[bytes]):
    """The same through liblrf_pack.so (lrf_pack_unpack_qmf_factors: the columns of all streams inflate on host threads; one
    stream 0.21 -> ~0.05 ms, 256 streams 51 -> ~1 ms), or None when the library is absent or refuses a stream — anything
    that is not exactly the int8 / column layout — so that _factors_python can say what is wrong with it."""
    import ctypes
    try:
        lib = _pack_lib()
    except OSError:
        return None
    metas, blobs = [], []
    for s in streams:
        try:
            encoded_metadata, encoded_factors = separate_bytes(s, 2)
            meta = bytes_to_dict(encoded_metadata)
            H0, W0 = meta["original size"][0]
            ranks = [int(r) for r in meta["rank"]]
            ok = (meta["color space"] == "YCbCr" and meta["patch"] and list(meta["patch size"]) == [8, 8] and len(ranks) == 3
                  and min(ranks) >= 1 and int(H0) >= 1 and int(W0) >= 1)
        except Exception:  # malformed: the Python path raises the proper error
            return None
        if not ok or (metas and (meta["original size"] != metas[0]["original size"] or meta["rank"] != metas[0]["rank"])):
            return None
        metas.append(meta)
        blobs.append(encoded_factors)
    H, W = metas[0]["original size"][0]
    ranks = [int(r) for r in metas[0]["rank"]]
    if max(ranks) > 64:
        return None
    dims = _lib.plane_dims(int(H), int(W))
    B = len(streams)
    # the metadata is untrusted and nothing of the payload has been validated yet: a deflate stream expands by at most
    # ~1032x, so a stream that claims more factor bytes than its payload could inflate to is refused before the buffers
    # it asks for are allocated (the Python parser then names the defect, or raises the same way)
    need = sum(d[4] * r for d, r in zip(dims, ranks)) + 64 * sum(ranks)
    if any(need > 1040 * len(b) + 4096 for b in blobs):
        return None
    for m in metas:  # what reaches the kernels is the validated integer form, not the raw JSON values
        m["rank"] = list(ranks)
    U = np.empty((B, sum(d[4] * r for d, r in zip(dims, ranks))), dtype=np.int8)
    V = np.empty((B, 64 * sum(ranks)), dtype=np.int8)
    ptrs = (ctypes.c_char_p * B)(*blobs)
    lens = (ctypes.c_int64 * B)(*[len(b) for b in blobs])
    M = (ctypes.c_int64 * 3)(*[d[4] for d in dims])
    R = (ctypes.c_int * 3)(*ranks)
    rc = lib.lrf_pack_unpack_qmf_factors(ptrs, lens, B, M, R, 0, U.ctypes.data_as(ctypes.c_void_p), U.shape[1],
                                         V.ctypes.data_as(ctypes.c_void_p), V.shape[1])
    return (metas, U, V) if rc == 0 else None


def _check_inflate(inflate) -> bool:
    """True for inflate="device", False for "host"; anything else is refused"""
    if inflate not in ("host", "device"):
        raise ValueError(f'inflate must be "host" or "device", got {inflate!r}')
    return inflate == "device"


_FACTOR_NAMES = ("u_Y", "v_Y", "u_Cb", "v_Cb", "u_Cr", "v_Cr")


def index_columns_native(blobs, Ms, Rs):
    """lrf_pack_index_qmf_columns_ragged: where the columns' zlib streams lie in the factor payloads of n streams -> (col_off int64
    [ncols] within each column's own blob, col_len int32 [ncols], rc); the arrays are None unless rc == 0.  Raises OSError where
    liblrf_pack.so cannot be used."""
    import ctypes
    lib = _pack_lib()
    n = len(blobs)
    ncols = 2 * sum(int(r) for R in Rs for r in R)
    col_off, col_len = np.empty((ncols,), dtype=np.int64), np.empty((ncols,), dtype=np.int32)
    rc = lib.lrf_pack_index_qmf_columns_ragged(
        (ctypes.c_char_p * n)(*blobs), (ctypes.c_int64 * n)(*[len(b) for b in blobs]), n,
        (ctypes.c_int64 * (3 * n))(*[int(m) for M in Ms for m in M]), (ctypes.c_int * (3 * n))(*[int(r) for R in Rs for r in R]),
        col_off.ctypes.data, col_len.ctypes.data, ncols)
    return (col_off, col_len, 0) if rc == 0 else (None, None, rc)


def _factors_ragged_device(streams: Sequence[bytes], device=None):
    """_factors_ragged with the columns inflated on the device (inflate="device") -> (ctx, [(H, W, ranks, u_off, v_off)], U, V):
    flat int8 CUDA tensors in the layout the ragged decoder reads.  The metadata is parsed and checked as _factors_ragged does
    (the branch: NotImplementedError; the ranks, the 1040x expansion bound, ranks <= 64: ValueError); the host only walks the
    container headers (lrf_pack_index_qmf_columns_ragged).  The factor payloads travel as ONE buffer in one copy,
    lrf_inflate_columns_i8 fills U and V, the statuses come back in one small copy, and a stream that does not inflate raises
    ValueError naming stream, factor and column before any decode kernel is launched.  OSError without liblrf_pack.so."""
    if isinstance(streams, (bytes, bytearray, str)) or len(streams) < 1:
        raise ValueError("qmf_decode_ragged takes a non-empty list of byte streams")
    for i, s in enumerate(streams):
        if not isinstance(s, (bytes, bytearray)):
            raise TypeError(f"stream {i} is {type(s).__name__}, not bytes")
    lib_error = None
    try:
        _pack_lib()
    except OSError as e:
        lib_error = e
    if lib_error is not None:
        raise OSError(f'inflate="device" needs liblrf_pack.so to walk the container headers: {lib_error}')
    images, blobs, Ms, uo, vo = [], [], [], 0, 0
    for i, s in enumerate(streams):
        encoded_metadata, encoded_factors = separate_bytes(bytes(s), 2)
        meta = bytes_to_dict(encoded_metadata)
        branch = _ragged_branch(meta)
        if branch:
            raise NotImplementedError(f"stream {i}: qmf_decode_ragged covers the YCbCr / 8x8-patch / chroma (0.5, 0.5) / uint8 branch only, "
                                      f"this stream is of {branch} (qmf_decode takes it)")
        H, W = (int(x) for x in meta["original size"][0])
        ranks = [int(r) for r in meta["rank"]]
        if len(ranks) != 3 or min(ranks) < 1:
            raise ValueError(f"stream {i} metadata: 'rank' must hold three positive integers")
        if max(ranks) > 64:
            raise ValueError(f"stream {i}: ranks {ranks} above 64")
        M = [d[4] for d in _lib.plane_dims(H, W)]
        # untrusted metadata: a deflate stream expands by at most ~1032x (_factors_native's bound)
        if sum(m * r for m, r in zip(M, ranks)) + 64 * sum(ranks) > 1040 * len(encoded_factors) + 4096:
            raise ValueError(f"stream {i}: its payload of {len(encoded_factors)} bytes cannot hold the factors its metadata describes")
        images.append((H, W, ranks, uo, vo))
        blobs.append(encoded_factors)
        Ms.append(M)
        uo += sum(m * r for m, r in zip(M, ranks))
        vo += 64 * sum(ranks)
    v0 = (uo + 255) // 256 * 256  # V starts at a multiple of 256 bytes of the one buffer, as a tensor of its own would
    Rs = [im[2] for im in images]
    col_off, col_len, rc = index_columns_native(blobs, Ms, Rs)
    if rc != 0:  # name the first stream the walk refuses
        for i in range(len(blobs)):
            if index_columns_native(blobs[i:i + 1], Ms[i:i + 1], Rs[i:i + 1])[2] != 0:
                raise ValueError(f"stream {i}: its payload is not six int8 factors packed column by column with the ranks its metadata names")
        raise ValueError("the streams' payloads are not int8 factors packed column by column")
    # the column table: matrix (image, plane, u or v), its streams in the container's order u_Y, v_Y, u_Cb, v_Cb, u_Cr, v_Cr
    mats = np.empty((6 * len(images), 4), dtype=np.int64)
    base = np.empty((len(images),), dtype=np.int64)
    first = at = 0
    for i, ((H, W, ranks, u_off, v_off), M) in enumerate(zip(images, Ms)):
        base[i] = at
        at += len(blobs[i])
        for c in range(3):
            mats[6 * i + 2 * c] = (u_off, M[c], ranks[c], first)
            mats[6 * i + 2 * c + 1] = (v0 + v_off, 64, ranks[c], first + ranks[c])
            first += 2 * ranks[c]
            u_off += M[c] * ranks[c]
            v_off += 64 * ranks[c]
    col_off += np.repeat(base, [2 * sum(r) for r in Rs])
    short = np.flatnonzero(col_len < 8)
    if short.size:
        raise ValueError(_inflate_refusal(int(short[0]), Rs, f"{int(col_len[short[0]])} bytes are no zlib stream"))
    ctx = _lib.context(device)
    src = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).cuda(ctx.device)
    buf = torch.empty((v0 + vo,), dtype=torch.int8, device=src.device)
    status = torch.empty((col_off.shape[0],), dtype=torch.int32, device=src.device)
    ctx.inflate_columns_into(src, mats, col_off, col_len, buf, status)
    st = status.cpu().numpy()
    failed = np.flatnonzero(st)
    if failed.size:
        raise ValueError(_inflate_refusal(int(failed[0]), Rs, f"inflate status {int(st[failed[0]])} (LRFI_E_*, include/lrf_hip.h): "
                                          "the column's zlib stream is corrupt, or the container was cut short"))
    return ctx, images, buf[:uo], buf[v0:]


def _inflate_refusal(k, Rs, what) -> str:
    """the message for column k of a call's column table"""
    for i, R in enumerate(Rs):
        for f in range(6):
            if k < R[f // 2]:
                return f"stream {i}: column {k} of factor {_FACTOR_NAMES[f]} does not inflate to its rows: {what}"
            k -= R[f // 2]
    raise AssertionError("column index outside the table")


def qmf_decode_batch(streams: Sequence[bytes], device=None, inflate: str = "host") -> torch.Tensor:
    """Decodes streams of equal geometry and ranks -> uint8 CUDA tensor [B,3,H,W].  Streams of the other branches (another
    patch size, patch=False, another chroma scale, the RGB colour space) are decoded one by one and stacked, except gray
    streams (RGB colour space, one channel, 8x8 patches) of one size and rank: one call -> [B,1,H,W].  A list that mixes gray
    and colour streams raises ValueError; inflate="device" on gray streams NotImplementedError.
    inflate="device": the columns' zlib streams are inflated on the GPU (_factors_ragged_device) instead of on host threads."""
    on_device = _check_inflate(inflate)
    m_first = bytes_to_dict(separate_bytes(streams[0], 2)[0])
    H0, W0 = (m_first["original size"][0] if m_first["color space"] == "YCbCr" else (0, 0))
    if m_first["color space"] != "YCbCr" or not m_first["patch"] or list(m_first["patch size"]) != [8, 8] \
            or list(m_first["original size"][1]) != [H0 // 2, W0 // 2]:
        if m_first["color space"] == "RGB":
            _refuse_mixed_streams(streams)
            return _qmf_decode_batch_rgbspace(streams, device, on_device)
        return torch.stack([_qmf_decode_anyshape(s) for s in streams])
    if on_device:
        ctx, images, U, V = _factors_ragged_device(streams, device)
        H, W, ranks = images[0][:3]
        if any((im[0], im[1], im[2]) != (H, W, ranks) for im in images[1:]):
            raise ValueError("streams differ in geometry or ranks")
        return ctx.decode_rgb(U.view(len(images), -1), V.view(len(images), -1), H, W, ranks)
    got = _factors_native(streams)
    if got is None:
        _refuse_mixed_streams(streams)
    metas, Uh, Vh = got if got is not None else _factors_python(streams)
    m0 = metas[0]
    for m in metas[1:]:
        if m["original size"] != m0["original size"] or m["rank"] != m0["rank"]:
            raise ValueError("streams differ in geometry or ranks")
    H, W = m0["original size"][0]
    dims = _lib.plane_dims(H, W)
    for c in range(3):  # the stream must describe the geometry the kernels derive from (H, W)
        if list(m0["original size"][c]) != [dims[c][0], dims[c][1]] or list(m0["padded size"][c]) != [dims[c][2], dims[c][3]]:
            raise NotImplementedError("stream geometry is not the scale_factor=(0.5,0.5) / 8x8 layout")
    ctx = _lib.context(device)
    U = torch.from_numpy(Uh).cuda(ctx.device)
    V = torch.from_numpy(Vh).cuda(ctx.device)
    if m0["dtype"] != "uint8":
        raise NotImplementedError("HIP decode writes uint8 images")
    return ctx.decode_rgb(U, V, H, W, m0["rank"])


def _ragged_branch(meta) -> str:
    """'' for a stream of the default branch (YCbCr, 8x8 patches, chroma (0.5, 0.5), uint8), else the name of its branch"""
    if meta["color space"] != "YCbCr":
        return f"the {meta['color space']} colour space"
    if not meta["patch"]:
        return "patch=False"
    if list(meta["patch size"]) != [8, 8]:
        return f"patch size {tuple(meta['patch size'])}"
    H, W = meta["original size"][0]
    dims = _lib.plane_dims(int(H), int(W))
    for c in range(3):
        if list(meta["original size"][c]) != [dims[c][0], dims[c][1]] or list(meta["padded size"][c]) != [dims[c][2], dims[c][3]]:
            return "a chroma scale other than (0.5, 0.5)"
    if meta["dtype"] != "uint8":
        return f"dtype {meta['dtype']}"
    return ""


def unpack_ragged_native(blobs, Ms, Rs, u_off, v_off, u_len, v_len, threads: int = 0):
    """lrf_pack_unpack_qmf_factors_ragged: the factor payloads of n streams of differing (M, R) -> (U int8 [u_len], V int8 [v_len],
    rc); U and V are None unless rc == 0.  Raises OSError where liblrf_pack.so cannot be used."""
    import ctypes
    lib = _pack_lib()
    n = len(blobs)
    U, V = np.empty((u_len,), dtype=np.int8), np.empty((v_len,), dtype=np.int8)
    rc = lib.lrf_pack_unpack_qmf_factors_ragged(
        (ctypes.c_char_p * n)(*blobs), (ctypes.c_int64 * n)(*[len(b) for b in blobs]), n,
        (ctypes.c_int64 * (3 * n))(*[int(m) for M in Ms for m in M]), (ctypes.c_int * (3 * n))(*[int(r) for R in Rs for r in R]),
        (ctypes.c_int64 * n)(*u_off), (ctypes.c_int64 * n)(*v_off), int(threads),
        U.ctypes.data_as(ctypes.c_void_p), u_len, V.ctypes.data_as(ctypes.c_void_p), v_len)
    return (U, V, 0) if rc == 0 else (None, None, rc)


def _factors_ragged(streams: Sequence[bytes]):
    """-> ([(H, W, ranks, u_off, v_off)], U int8 flat, V int8 flat) on the host, every stream checked: the branch
    (NotImplementedError), the ranks, and the factor shapes against the metadata (ValueError).  No GPU is touched."""
    if isinstance(streams, (bytes, bytearray, str)) or len(streams) < 1:
        raise ValueError("qmf_decode_ragged takes a non-empty list of byte streams")
    for i, s in enumerate(streams):
        if not isinstance(s, (bytes, bytearray)):
            raise TypeError(f"stream {i} is {type(s).__name__}, not bytes")
    images, blobs, Ms, uo, vo = [], [], [], 0, 0
    for i, s in enumerate(streams):
        encoded_metadata, encoded_factors = separate_bytes(bytes(s), 2)
        meta = bytes_to_dict(encoded_metadata)
        branch = _ragged_branch(meta)
        if branch:
            raise NotImplementedError(f"stream {i}: qmf_decode_ragged covers the YCbCr / 8x8-patch / chroma (0.5, 0.5) / uint8 branch only, "
                                      f"this stream is of {branch} (qmf_decode takes it)")
        H, W = (int(x) for x in meta["original size"][0])
        ranks = [int(r) for r in meta["rank"]]
        if len(ranks) != 3 or min(ranks) < 1:
            raise ValueError(f"stream {i} metadata: 'rank' must hold three positive integers")
        M = [d[4] for d in _lib.plane_dims(H, W)]
        images.append((H, W, ranks, uo, vo))
        blobs.append(encoded_factors)
        Ms.append(M)
        uo += sum(m * r for m, r in zip(M, ranks))
        vo += 64 * sum(ranks)
    # untrusted metadata, nothing of the payload validated yet: a deflate stream expands by at most ~1032x, so a stream that
    # claims more factor bytes than its payload could inflate to never gets its buffers (_factors_native's bound)
    sizes = [sum(m * r for m, r in zip(M, im[2])) + 64 * sum(im[2]) for M, im in zip(Ms, images)]
    U = V = None
    if max(max(im[2]) for im in images) <= 64 and all(n <= 1040 * len(b) + 4096 for n, b in zip(sizes, blobs)):
        try:
            U, V, _ = unpack_ragged_native(blobs, Ms, [im[2] for im in images], [im[3] for im in images], [im[4] for im in images], uo, vo)
        except OSError:
            pass
    if U is None:  # the library is absent or refused a stream: this module's parser names the defect (or parses what is valid)
        Us, Vs = [], []
        import zlib
        for i, s in enumerate(streams):
            try:
                _, u1, v1 = _factors_python([bytes(s)])
            except (zlib.error, KeyError, IndexError, TypeError) as e:  # cut short or corrupt inside the container
                raise ValueError(f"stream {i}: its payload does not hold the factors its metadata describes ({e})") from e
            Us.append(u1[0])
            Vs.append(v1[0])
        U, V = np.concatenate(Us), np.concatenate(Vs)
    for i, im in enumerate(images):
        if max(im[2]) > 64:
            raise ValueError(f"stream {i}: ranks {im[2]} above 64")
    return images, U, V


def qmf_decode_ragged(streams: Sequence[bytes], device=None, inflate: str = "host") -> list:
    """Decodes streams that differ in size and ranks — what qmf_encode_target writes for a batch, or a dataset of mixed sizes —
    in one call: -> a list of uint8 CUDA tensors [3,H_i,W_i] in input order (views of one buffer), each equal to
    qmf_decode of its stream.  The default branch only (YCbCr, 8x8 patches, chroma (0.5, 0.5), uint8): a stream of another
    branch raises NotImplementedError naming it.  One host-to-device copy of all U factors, one of all V, one kernel call.
    inflate="device": the streams' payloads go up in one copy and are inflated on the GPU (_factors_ragged_device).
    A list whose every stream is a gray stream (RGB colour space, one channel, 8x8 patches, uint8; sizes and ranks may differ)
    takes the gray loader instead: -> uint8 CUDA tensors [1,H_i,W_i], views of one buffer (inflate="device": NotImplementedError)."""
    on_device = _check_inflate(inflate)
    gray = _gray_factors_ragged(streams)
    if gray is not None:
        _refuse_gray_inflate(on_device)
        return _resident(*gray, device, 1).decode()
    if on_device:
        ctx, images, U, V = _factors_ragged_device(streams, device)
        return ctx.decode_ragged(U, V, images)
    images, Uh, Vh = _factors_ragged(streams)
    ctx = _lib.context(device)
    U = torch.from_numpy(Uh).cuda(ctx.device)
    V = torch.from_numpy(Vh).cuda(ctx.device)
    return ctx.decode_ragged(U, V, images)


def _crop_scales(scale, n):
    """scale: one integer or one per crop, out of 1, 2, 4, 8 -> an int64 array [n]"""
    sc = np.asarray(scale)
    if sc.dtype.kind not in "iu" or sc.dtype == np.bool_:
        raise TypeError(f"scale must be an integer or one integer per crop, got {scale!r}")
    if sc.ndim == 0:
        sc = np.full(n, int(sc), dtype=np.int64)
    if sc.ndim != 1 or sc.shape[0] != n:
        raise ValueError(f"scale must be one value or one per crop ({n}), got shape {tuple(sc.shape)}")
    bad = np.flatnonzero(~np.isin(sc, (1, 2, 4, 8)))
    if bad.size:
        raise ValueError(f"crop {bad[0]}: scale {sc[bad[0]]}: 1, 2, 4 or 8 expected")
    return sc.astype(np.int64)


def _split_crops_by_scale(U, V, images, crops, size, scale):
    """The crops of a call with per-crop scales, split for the two kernels calls and validated (no device is touched): ->
    (where the full-scale crops stand in the call, their boxes [n1, 3], where the scaled ones stand, their boxes [n2, 4] of
    (image, scale, y0, x0)); either part may be empty."""
    boxes = _lib._check_boxes(crops, ("image", "y0", "x0"), "decode_crops", most=None)  # (each part takes its own kernel call of 1 to 2^20)
    sc = _crop_scales(scale, boxes.shape[0])
    full, scaled = np.flatnonzero(sc == 1), np.flatnonzero(sc != 1)
    b1 = boxes[full]
    b2 = np.concatenate([boxes[scaled, :1], sc[scaled, None], boxes[scaled, 1:]], axis=1)
    if full.size:
        _lib.check_crop_args(U, V, images, b1, size)
    if scaled.size:
        _lib.check_scaled_args(U, V, images, crops=b2, size=size)
    return full, b1, scaled, b2


def _decode_crops_at_scales(ctx, U, V, images, crops, size, scale, **tensor) -> torch.Tensor:
    """entries at scale 1 take Context.decode_crops, the rest Context.decode_scaled_crops; merged in call order.  tensor: the
    dtype, mean, std, channels_last and out of those two (_tensor_kwargs: checked, empty for uint8), the result in that format (out=:
    written in place)"""
    full, b1, scaled, b2 = _split_crops_by_scale(U, V, images, crops, size, scale)
    if not scaled.size:
        return ctx.decode_crops(U, V, images, b1, size, **tensor)
    if not full.size:
        return ctx.decode_scaled_crops(U, V, images, b2, size, **tensor)
    out, parts = tensor.get("out"), {k: v for k, v in tensor.items() if k != "out"}
    if out is not None:
        _lib._tensor_output("decode_crops", out, full.size + scaled.size, int(size[0]), int(size[1]), tensor["dtype"], tensor.get("channels_last", False), U.device)
    a, b = ctx.decode_crops(U, V, images, b1, size, **parts), ctx.decode_scaled_crops(U, V, images, b2, size, **parts)
    if out is None:
        fmt = torch.channels_last if tensor.get("channels_last", False) else torch.contiguous_format
        out = torch.empty((full.size + scaled.size,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device, memory_format=fmt)
    out[torch.from_numpy(full).to(a.device)] = a
    out[torch.from_numpy(scaled).to(a.device)] = b
    return out


class ResidentFactors:
    """The factors of a list of streams resident on one device (qmf_load_factors): flat int8 U and V, the image table decode_ragged
    takes, and the images' sizes.  A dataset kept this way costs its int8 factors, not its pixels; .decode() gives whole images,
    .decode_crops(crops, size) windows of them, both also at 1/2, 1/4 or 1/8 scale (scale=).
    channels: 3 for colour streams (images: (H, W, ranks, u_off, v_off)), 1 for a list of gray streams (images: (H, W, R, u_off,
    v_off), one factor pair each): the same methods, results [1, H, W] / [n, 1, h, w], served by the gray loader's kernels."""

    def __init__(self, ctx, U, V, images, channels=3):
        self._ctx, self.U, self.V, self.images, self.channels = ctx, U, V, images, channels
        self.sizes = [(im[0], im[1]) for im in images]

    def __len__(self):
        return len(self.images)

    def scaled_sizes(self, scale) -> list:
        """the images' sizes at 1/scale: (ceil(H / scale), ceil(W / scale)); scale 1: their sizes"""
        return list(self.sizes) if type(scale) is int and scale == 1 else [_lib.scaled_dims(H, W, scale) for H, W in self.sizes]

    def decode(self, scale=1) -> list:
        """every image: what qmf_decode_ragged gives for the streams; scale 2, 4, 8: what qmf_decode_scaled gives"""
        if self.channels == 1:
            return self._ctx.decode_gray_ragged(self.U, self.V, self.images, scale)
        if type(scale) is int and scale == 1:
            return self._ctx.decode_ragged(self.U, self.V, self.images)
        return self._ctx.decode_scaled(self.U, self.V, self.images, scale)

    def decode_crops(self, crops, size, scale=1, dtype=torch.uint8, mean=None, std=None, channels_last=False, out=None) -> torch.Tensor:
        """crops: integers [n, 3] of (image, y0, x0) on the host; size: (h, w) -> uint8 CUDA [n, 3, h, w].  scale: 1, 2, 4, 8 or
        one of them per crop: crop j is the window (y0, x0) of its image decoded at 1/scale_j, y0 and x0 in that scaled image.
        dtype, mean, std, channels_last, out: the model's tensor instead of bytes, as qmf_decode_crops describes"""
        tensor = _tensor_kwargs("decode_crops", dtype, mean, std, channels_last, out, self.channels)
        if self.channels == 1:  # per-crop scales go to the device in one call: the gray entry takes scale 1 too
            return self._ctx.decode_gray_crops(self.U, self.V, self.images, _gray_crop_rows(crops, scale), size, **tensor)
        if type(scale) is int and scale == 1:
            return self._ctx.decode_crops(self.U, self.V, self.images, crops, size, **tensor)
        return _decode_crops_at_scales(self._ctx, self.U, self.V, self.images, crops, size, scale, **tensor)

    def decode_resized_crops(self, boxes, size, flip=None, dtype=torch.uint8, mean=None, std=None, channels_last=False, out=None) -> torch.Tensor:
        """boxes: integers [n, 5] of (image, y0, x0, h, w) on the host, full-resolution pixels; size: (oh, ow); flip: None, one
        bool, or one bool per box (mirror the output's columns) -> uint8 CUDA [n, 3, oh, ow]: qmf_decode_resized_crops, which
        also describes dtype, mean, std, channels_last and out"""
        rows = _resized_boxes(boxes, flip)
        return self._decode_resized_rows(rows, size, _tensor_kwargs("decode_resized_crops", dtype, mean, std, channels_last, out, self.channels))

    def _decode_resized_rows(self, rows, size, tensor) -> torch.Tensor:
        """rows: _resized_boxes' [n, 6]; tensor: _tensor_kwargs' keywords"""
        decode = self._ctx.decode_gray_resized_crops if self.channels == 1 else self._ctx.decode_resized_crops
        return decode(self.U, self.V, self.images, rows, size, **tensor)


def _tensor_kwargs(entry, dtype, mean, std, channels_last, out, channels=3) -> dict:
    """the output arguments of the crop entries, checked (no device is touched), as the keywords Context's methods take: none for
    the defaults, which are the uint8 calls as they always were.  channels 1 (a gray source): mean and std are None, one number or
    a sequence of one (three numbers: ValueError)"""
    if _lib._tensor_request(entry, dtype, mean, std, channels_last, out, channels) is None:
        return {}
    return dict(dtype=dtype, mean=mean, std=std, channels_last=channels_last, out=out)


def _gray_crop_rows(crops, scale):
    """crops: integers [n, 3] of (image, y0, x0) on the host; scale: 1, 2, 4, 8 or one of them per crop -> an int64 array [n, 4]
    of (image, scale, y0, x0), the rows Context.decode_gray_crops takes (which validates the windows themselves)"""
    boxes = _lib._check_boxes(crops, ("image", "y0", "x0"), "decode_crops")
    sc = _crop_scales(scale, boxes.shape[0])
    return np.concatenate([boxes[:, :1], sc[:, None], boxes[:, 1:]], axis=1)


def _gray_factors_ragged(streams):
    """None unless every stream of the list is a gray stream (RGB colour space, one channel, 8x8 patches, uint8: _is_gray_stream
    of _two_factor_parts, which validates the factors against the header) — every other list, a malformed one included, is left
    to the code and the errors it always had.  Else ([(H, W, R, u_off, v_off)], U int8 flat, V int8 flat) on the host: image i's
    U [M, R] and V [64, R] back to back.  No GPU is touched."""
    if isinstance(streams, (bytes, bytearray, str)) or not hasattr(streams, "__len__") or len(streams) < 1:
        return None
    parts = []
    for s in streams:
        if not isinstance(s, (bytes, bytearray)):
            return None
        try:
            if bytes_to_dict(separate_bytes(bytes(s), 2)[0])["color space"] != "RGB":
                return None
            part = _two_factor_parts(bytes(s))
        except Exception:
            return None
        if not _is_gray_stream(part[3]):
            return None
        parts.append(part)
    images, uo, vo = [], 0, 0
    for _, u, v, (_, H, W, _, R) in parts:
        images.append((H, W, R, uo, vo))
        uo += u.shape[0] * R
        vo += 64 * R
    U = np.concatenate([np.asarray(p[1], dtype=np.int8).reshape(-1) for p in parts])
    V = np.concatenate([np.asarray(p[2], dtype=np.int8).reshape(-1) for p in parts])
    return images, U, V


def _refuse_gray_inflate(on_device):
    if on_device:
        raise NotImplementedError("inflate='device' is not served for gray streams (two-factor containers inflate on the host)")


def _resized_boxes(boxes, flip):
    """boxes: integers [n, 5] of (image, y0, x0, h, w) on the host; flip: None, one bool, or one bool per box -> an int64 array
    [n, 6] of (image, y0, x0, h, w, flip), the rows Context.decode_resized_crops takes (which validates the boxes themselves)"""
    b = _lib._check_boxes(boxes, ("image", "y0", "x0", "h", "w"), "decode_resized_crops", noun="boxes", most=None)  # (check_resized_args counts them)
    n = b.shape[0]
    if flip is None:
        fl = np.zeros(n, dtype=np.int64)
    else:
        fl = np.asarray(flip.detach().cpu().numpy() if hasattr(flip, "detach") else flip)
        if fl.dtype != np.bool_:
            raise TypeError(f"flip must be None, a bool or one bool per box, got {flip!r}")
        if fl.ndim == 0:
            fl = np.full(n, bool(fl))
        if fl.ndim != 1 or fl.shape[0] != n:
            raise ValueError(f"flip must be one value or one per box ({n}), got shape {tuple(fl.shape)}")
        fl = fl.astype(np.int64)
    return np.concatenate([b, fl[:, None]], axis=1)


def _resident(images, Uh, Vh, device, channels=3) -> ResidentFactors:
    ctx = _lib.context(device)
    return ResidentFactors(ctx, torch.from_numpy(Uh).cuda(ctx.device), torch.from_numpy(Vh).cuda(ctx.device), images, channels)


def qmf_load_factors(streams: Sequence[bytes], device=None, inflate: str = "host") -> ResidentFactors:
    """Parses and validates the streams once (the default branch only, as qmf_decode_ragged: a stream of another branch raises
    NotImplementedError naming it) and uploads their factors once -> ResidentFactors.  inflate="device": the compressed payloads
    are uploaded instead and inflated on the GPU.  A list whose every stream is a gray stream (RGB colour space, one channel, 8x8
    patches, uint8) gives a ResidentFactors with channels == 1 (inflate="device": NotImplementedError)."""
    on_device = _check_inflate(inflate)
    gray = _gray_factors_ragged(streams)
    if gray is not None:
        _refuse_gray_inflate(on_device)
        return _resident(*gray, device, 1)
    if on_device:
        ctx, images, U, V = _factors_ragged_device(streams, device)
        return ResidentFactors(ctx, U, V, images)
    return _resident(*_factors_ragged(streams), device)


def qmf_decode_crops(source, crops, size, device=None, inflate: str = "host", scale=1, dtype=torch.uint8, mean=None, std=None, channels_last=False,
                     out=None) -> torch.Tensor:
    """Windows of compressed images without decoding the images: source is a list of streams (parsed and uploaded for this call)
    or the ResidentFactors of qmf_load_factors (nothing but the crop list travels); crops: integers [n, 3] of (image, y0, x0) on
    the host; size: (h, w) -> uint8 CUDA [n, 3, h, w], crop j equal to qmf_decode(stream)[:, y0:y0+h, x0:x0+w].
    inflate="device" (a list of streams only): their columns are inflated on the GPU.
    scale: 1, 2, 4, 8 or one of them per crop: crop j is then that window of qmf_decode_scaled(stream, scale_j).
    dtype: torch.float32, float16 or bfloat16 gives the tensor a model takes instead, in the same call and with no uint8 batch in
    between: logical shape [n, 3, h, w], element = every byte b above as fl32(fl32(b * scale_k) + bias_k) rounded to dtype, with
    scale_k = float32(1 / (255 std_k)) and bias_k = float32(-mean_k / std_k) — torchvision's ToDtype(scale=True) and
    Normalize(mean, std) to within an fp32 rounding; mean, std: None, one number or three, in [0, 1] units; channels_last=True:
    torch.channels_last memory; out: a tensor of that dtype, shape, device and memory format, written in place and returned.
    With dtype=torch.uint8 (the default) the other four must be left alone: ValueError.
    A gray source (a list of gray streams, or their ResidentFactors): [n, 1, h, w]; mean, std: None, one number or a sequence of
    one (three numbers: ValueError); the crops of every scale leave in one kernel call."""
    gray = source.channels == 1 if isinstance(source, ResidentFactors) else _gray_factors_ragged(source)  # (host only; raises nothing)
    tensor = _tensor_kwargs("qmf_decode_crops", dtype, mean, std, channels_last, out, 1 if gray else 3)  # refused before anything is uploaded
    on_device = _check_inflate(inflate)
    if isinstance(source, ResidentFactors):
        pass
    elif gray:
        _refuse_gray_inflate(on_device)
        images, Uh, Vh = gray
        _lib.check_gray_crop_args(torch.from_numpy(Uh), torch.from_numpy(Vh), images, _gray_crop_rows(crops, scale), size)  # before a GPU is asked for
        source = _resident(images, Uh, Vh, device, 1)
    elif on_device:
        ctx, images, U, V = _factors_ragged_device(source, device)
        source = ResidentFactors(ctx, U, V, images)
    else:
        images, Uh, Vh = _factors_ragged(source)
        if type(scale) is int and scale == 1:
            _lib.check_crop_args(torch.from_numpy(Uh), torch.from_numpy(Vh), images, crops, size)  # refused before a GPU is asked for
        else:
            _split_crops_by_scale(torch.from_numpy(Uh), torch.from_numpy(Vh), images, crops, size, scale)
        source = _resident(images, Uh, Vh, device)
    return source.decode_crops(crops, size, scale, **tensor)


def qmf_decode_resized_crops(source, boxes, size, flip=None, device=None, inflate: str = "host", dtype=torch.uint8, mean=None, std=None,
                             channels_last=False, out=None) -> torch.Tensor:
    """RandomResizedCrop straight from the factors: n boxes of any size and position, out of images of any sizes and ranks,
    resampled to one output size in one call.  source: a list of streams or the ResidentFactors of qmf_load_factors; boxes:
    integers [n, 5] of (image, y0, x0, h, w) on the host, each inside its image with h, w >= 1; size: (oh, ow), sides in
    [1, 16384]; flip: None, one bool, or one bool per box (output column c then holds column ow - 1 - c) -> uint8 CUDA
    [n, 3, oh, ow].  Each box is sampled bilinearly, in fixed point (weights in 1/256, one rounding), from the level of its image
    nearest above the output's size: the image itself, or qmf_decode_scaled at the largest scale f of 8, 4, 2 with f oh <= h and
    f ow <= w; a box more than 16 times the output is sampled from level 8 without further prefiltering.  A box of the output's
    size is qmf_decode_crops' crop byte for byte, a box aligned to f and f times the output the crop at scale f; otherwise
    within 2.5 levels of real-valued bilinear interpolation of the level.  These are NOT torchvision's bytes: torchvision
    interpolates the full-resolution pixels in floating point (and antialiases differently).  Exact definition:
    include/lrf_hip.h, lrf_qmf_decode_resized_crops_rgb_u8.  The default branch only, as qmf_decode_crops: a stream of another
    branch raises NotImplementedError naming it.  inflate="device" (a list of streams only): their columns are inflated on the GPU.
    dtype, mean, std, channels_last, out: as qmf_decode_crops takes them — the resized crop, the flip, to-tensor and normalise in
    one call; under flip the pixels are mirrored, whatever the element size or layout."""
    gray = source.channels == 1 if isinstance(source, ResidentFactors) else _gray_factors_ragged(source)  # (host only; raises nothing)
    # (a gray source: [n, 1, oh, ow]; mean, std: None, one number or a sequence of one)
    tensor = _tensor_kwargs("qmf_decode_resized_crops", dtype, mean, std, channels_last, out, 1 if gray else 3)
    on_device = _check_inflate(inflate)
    rows = _resized_boxes(boxes, flip)
    if isinstance(source, ResidentFactors):
        pass
    elif gray:
        _refuse_gray_inflate(on_device)
        images, Uh, Vh = gray
        _lib.check_gray_resized_args(torch.from_numpy(Uh), torch.from_numpy(Vh), images, rows, size)  # refused before a GPU is asked for
        source = _resident(images, Uh, Vh, device, 1)
    elif on_device:
        ctx, images, U, V = _factors_ragged_device(source, device)
        source = ResidentFactors(ctx, U, V, images)
    else:
        images, Uh, Vh = _factors_ragged(source)
        _lib.check_resized_args(torch.from_numpy(Uh), torch.from_numpy(Vh), images, rows, size)  # refused before a GPU is asked for
        source = _resident(images, Uh, Vh, device)
    return source._decode_resized_rows(rows, size, tensor)


def qmf_decode_scaled(source, scale, device=None, inflate: str = "host") -> list:
    """Thumbnails, previews, the coarse level a resampling loader starts from: the images at 1/2, 1/4 or 1/8 scale straight from
    their factors, without the full-resolution pixels.  source: a list of streams or the ResidentFactors of qmf_load_factors;
    scale: 2, 4 or 8 -> a list of uint8 CUDA tensors [3, ceil(H_i / scale), ceil(W_i / scale)] in input order.  Pixel (i, j) is
    the decoder's image before its colour conversion averaged over the scale x scale block of image pixels it covers (the
    partial blocks at the bottom and right edge over the pixels that exist), then converted, clamped and truncated: within
    half a level on average of block-averaging qmf_decode's bytes, which truncates and clamps before it averages.  The default
    branch only (YCbCr, 8x8 patches, chroma (0.5, 0.5), uint8): a stream of another branch raises NotImplementedError naming it.
    inflate="device" (a list of streams only): their columns are inflated on the GPU."""
    on_device = _check_inflate(inflate)
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)):
        raise TypeError(f"scale must be an integer, got {scale!r}")
    if int(scale) not in _lib.SCALES:
        raise ValueError(f"scale {scale}: 2, 4 or 8 expected")
    if isinstance(source, ResidentFactors):
        return source.decode(int(scale))
    gray = _gray_factors_ragged(source)
    if gray is not None:  # a list of gray streams: [1, ceil(H_i / scale), ceil(W_i / scale)], the gray loader's exact-integer levels
        _refuse_gray_inflate(on_device)
        return _resident(*gray, device, 1).decode(int(scale))
    if on_device:
        ctx, images, U, V = _factors_ragged_device(source, device)
        return ctx.decode_scaled(U, V, images, int(scale))
    return _resident(*_factors_ragged(source), device).decode(int(scale))


def _two_factor_parts(encoded_image: bytes):
    """host only: -> (metadata, u, v, (C, H, W, patch_size, R)) of a stream of the RGB colour-space branch; the geometry from
    _lib.chan_stream_geometry, which refuses factors that do not match the header"""
    encoded_metadata, encoded_factors = separate_bytes(encoded_image, 2)
    metadata = bytes_to_dict(encoded_metadata)
    if metadata["color space"] != "RGB":
        raise ValueError(f"not a stream of the RGB colour-space branch: {metadata['color space']!r}")
    if metadata["dtype"] != "uint8":
        raise NotImplementedError("HIP decode writes uint8 images")
    u, v = (decode_tensor(f) for f in separate_bytes(encoded_factors, 2))
    if u.dtype != np.int8 or v.dtype != np.int8:
        raise ValueError("stream factors are not int8")
    return metadata, u, v, _lib.chan_stream_geometry(metadata, u.shape, v.shape)


def _is_gray_stream(geom) -> bool:
    C, _, _, patch_size, R = geom
    return C == 1 and patch_size == (8, 8) and R <= 64


def _qmf_decode_rgbspace(encoded_image: bytes, device=None) -> torch.Tensor:
    """RGB colour-space branch of qmf_decode (lrf/compression/qmf.py:309-323) -> uint8 CUDA tensor [C,H,W]: C from the factor
    shapes, as in the reference (v.shape[0] / (p q) with patches, u.shape[0] without)."""
    _, u, v, geom = _two_factor_parts(encoded_image)
    C, H, W, patch_size, R = geom
    ctx = _lib.context(device)
    U = torch.from_numpy(np.array(u, dtype=np.int8)).unsqueeze(0).cuda(ctx.device)  # copies: decode_tensor may return read-only views
    V = torch.from_numpy(np.array(v, dtype=np.int8)).unsqueeze(0).cuda(ctx.device)
    if C == 3:
        if patch_size == (8, 8):
            return ctx.qmf_rgbspace_decode(U, V, H, W)[0]
        return ctx.qmf_rgbspace_decode_any(U, V, H, W, patch_size)[0]
    if _is_gray_stream(geom):
        return ctx.decode_gray(U, V, H, W)
    return ctx.chan_decode(U, V, C, H, W, patch_size)[0]


def _qmf_decode_batch_rgbspace(streams: Sequence[bytes], device, on_device: bool) -> torch.Tensor:
    """qmf_decode_batch of RGB colour-space streams: gray 8x8 streams of one size and rank in ONE lrf_qmf_decode_gray_u8 call
    -> [B,1,H,W]; colour streams one by one and stacked, as before.  A list that mixes the two raises ValueError."""
    parts = [_two_factor_parts(s) for s in streams]
    gray = [_is_gray_stream(p[3]) for p in parts]
    if not any(gray):
        if any(p[3][0] != parts[0][3][0] for p in parts):
            raise ValueError("streams differ in channel count")
        return torch.stack([_qmf_decode_rgbspace(s, device) for s in streams])
    if not all(gray):
        raise ValueError("the list mixes gray and colour streams")
    if on_device:
        raise NotImplementedError("inflate='device' is not served for gray streams (two-factor containers inflate on the host)")
    if any(p[3] != parts[0][3] for p in parts):
        raise ValueError("streams differ in geometry or ranks")
    _, H, W, _, _ = parts[0][3]
    ctx = _lib.context(device)
    U = torch.from_numpy(np.stack([np.asarray(p[1], dtype=np.int8) for p in parts])).cuda(ctx.device)
    V = torch.from_numpy(np.stack([np.asarray(p[2], dtype=np.int8) for p in parts])).cuda(ctx.device)
    return ctx.decode_gray(U, V, H, W).unsqueeze(1)


def _refuse_mixed_streams(streams: Sequence[bytes]):
    """ValueError when a list of default-branch streams also holds streams of the RGB colour space (gray among them)"""
    spaces = {bytes_to_dict(separate_bytes(s, 2)[0])["color space"] for s in streams}
    if len(spaces) > 1:
        raise ValueError(f"the list mixes streams of different colour spaces ({', '.join(sorted(spaces))}): gray and colour streams "
                         "decode in calls of their own")


def qmf_decode(encoded_image: bytes) -> torch.Tensor:
    """Decode a QMF stream -> uint8 tensor [3,H,W] on the CPU, like the reference's lrf.qmf_decode
    (lrf/compression/qmf.py:295-353); [C,H,W] for an RGB colour-space stream of C channels."""
    meta = bytes_to_dict(separate_bytes(encoded_image, 2)[0])
    if meta["color space"] == "RGB":
        return _qmf_decode_rgbspace(encoded_image).cpu()
    H, W = meta["original size"][0]
    if not meta["patch"] or list(meta["patch size"]) != [8, 8] or list(meta["original size"][1]) != [H // 2, W // 2]:
        return _qmf_decode_anyshape(encoded_image).cpu()
    return qmf_decode_batch([encoded_image])[0].cpu()
