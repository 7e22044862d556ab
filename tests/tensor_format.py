"""The tensor format of the model-ready decode entries (lrf_tensor_format, include/lrf_hip.h) restated with torch CPU ops, and the
inputs test_decode_tensor_gpu.py decodes.  For the byte b of (crop, channel k, row, column)

    t = fl32(float(b) * scale[k]);   v = fl32(t + bias[k]);   out = v rounded to nearest even into dtype

two fp32 roundings, not a fused multiply-add: `apply_format` below IS that chain on the CPU (torch's mul, add and .to() each
round once), and every comparison of a kernel's output with it is bitwise, on the values viewed as integers (`bits`).
test_decode_tensor_host.py checks the restatement itself and that the GPU tests' inputs would expose a contracted kernel."""
import numpy as np
import torch

from resized_decode import resized_level

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
FORMATS = [(d, cl) for d in DTYPES for cl in (False, True)]  # (dtype, channels_last)
FORMAT_IDS = [f"{str(d).split('.')[1]}_{'nhwc' if cl else 'nchw'}" for d, cl in FORMATS]


def constants(mean=None, std=None):
    """(scale, bias) float32 [3]: float32(1 / (255 std_k)) and float32(-mean_k / std_k), from Python doubles, rounded once"""
    three = lambda v, d: [float(d)] * 3 if v is None else ([float(v)] * 3 if np.isscalar(v) else [float(x) for x in v])
    m, s = three(mean, 0.0), three(std, 1.0)
    return np.array([1.0 / (255.0 * x) for x in s]).astype(np.float32), np.array([-a / x for a, x in zip(m, s)]).astype(np.float32)


def apply_format(b, scale, bias, dtype):
    """b: uint8 [..., 3, h, w] (numpy or a CPU tensor) -> the definition's tensor of `dtype`, same shape, on the CPU"""
    b = torch.as_tensor(np.ascontiguousarray(b) if isinstance(b, np.ndarray) else b)
    assert b.dtype == torch.uint8 and not b.is_cuda and b.shape[-3] == 3
    s, o = torch.from_numpy(np.asarray(scale, np.float32)).view(3, 1, 1), torch.from_numpy(np.asarray(bias, np.float32)).view(3, 1, 1)
    return b.float().mul(s).add(o).to(dtype)


def bits(t):
    """a float tensor's values as integers of its width, logical order (so NCHW and channels_last results compare)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def fused(scale, bias):
    """float32 [3, 256]: fl32(b * scale_k + bias_k) with ONE rounding, what an fma contraction would give.  In float64 the product
    of two float32 is exact (48 bits) and so is the sum here: |b scale| < 2^9 and a bias within 2^-12 .. 2^9 keep every bit above
    2^-53 of the larger term; asserted rather than assumed"""
    b = np.arange(256, dtype=np.float64)[None, :]
    s, o = np.asarray(scale, np.float32).astype(np.float64)[:, None], np.asarray(bias, np.float32).astype(np.float64)[:, None]
    p = b * s
    v = p + o
    assert np.array_equal(v - o, p) and np.array_equal(v - p, np.broadcast_to(o, v.shape)), "the float64 sum is not exact for these constants"
    return v.astype(np.float32)


def unfused(scale, bias):
    """float32 [3, 256]: the definition in fp32, every byte value of every channel"""
    b = torch.arange(256, dtype=torch.uint8).view(1, 256).expand(3, 256).reshape(3, 256, 1)
    return apply_format(b.contiguous(), scale, bias, torch.float32).reshape(3, 256).numpy()


def fma_differs(scale, bias):
    """bool [3, 256]: the byte values on which a contracted kernel's fp32 value differs from the definition's"""
    return fused(scale, bias).view(np.int32) != unfused(scale, bias).view(np.int32)


# ---- the inputs of the GPU tests: random int8 factors (case_factors), one seed per image ----
# the resized crops: 16-aligned, odd (padded planes), the smallest; ranks <= 8, past 8, the largest
RESIZED_GEOMETRIES = [(64, 96), (45, 61), (9, 9)]
RESIZED_TRIPLES = [(7, 3, 3), (26, 13, 13), (64, 64, 64)]
RESIZED_SIZES = [(5, 7), (17, 33)]  # tails narrower than four pixels; two rows of tiles
BIG = (173, 264, (7, 3, 3))  # where the box list meets every level and both paths
# crops and scaled crops: on the aligned image the tiled classes (rank bounds 8/4, 16/8, 32/16), on the odd one k_decode8_crops
# and k_decode_crops_any
CROP_CASES = [(64, 96, (8, 4, 4)), (64, 96, (16, 8, 8)), (64, 96, (32, 16, 16)), (45, 61, (7, 3, 3)), (45, 61, (26, 13, 13))]
WINDOWS = [(1, 1), (3, 5), (16, 16), (13, 37)]
# the cases whose oracle bytes must, each alone, cover the byte values an fma would change (the gate of test_decode_tensor_host.py);
# 9x9 holds 81 pixels a channel and is left to the others
GATE_CASES = [(H, W, r) for (H, W) in RESIZED_GEOMETRIES[:2] for r in RESIZED_TRIPLES] + [BIG] + CROP_CASES
GATE_MIN = 100


def case_seed(H, W, ranks):
    return 100003 * H + 101 * W + ranks[0]


def case_factors(H, W, ranks):
    """flat int8 (u, v) of the image of one case: uniform in [-a, a), a = 16 up to luma rank 16, 10 up to 32, 8 above — the
    planes' spread grows with sqrt(rank) a^2 / 3, and at a = 16 the large ranks saturate most bytes to 0 or 255, which would leave
    the gate of test_decode_tensor_host.py too few byte values"""
    from scaled_decode import random_factors
    a = 16 if ranks[0] <= 16 else (10 if ranks[0] <= 32 else 8)
    return random_factors(np.random.default_rng(case_seed(H, W, ranks)), H, W, ranks, lo=-a, hi=a)


def oracle_image(oracle, u, v, H, W, ranks):
    """uint8 [3, H, W]: the CPU oracle's decode of the factors"""
    from lrf_amd.codec import split_factors
    f6 = split_factors(u, v, (H, W), ranks)
    return oracle.planes_to_rgb(f6[0::2], f6[1::2], H, W)


# the staged path's tiles (lrf_plan.h: LRF_RS_TH, LRF_RS_TW, LRF_RS_FH, LRF_RS_FW and resized_staged), to say which path a box takes
TH, TW, FH, FW = 16, 64, 44, 192


def staged(hb, wb, oh, ow):
    f = resized_level(hb, wb, oh, ow)
    bound = lambda tile, n_out, nb: (min(tile, n_out) - 1) * nb // (n_out * f) + 3
    return bound(TH, oh, hb) <= FH and bound(TW, ow, wb) <= FW


def boxes_of(H, W, size, seed):
    """(y0, x0, hb, wb) of one image for one output size: the list of test_decode_resized_gpu.py restated — the whole image, 1 x 1
    and 3 x 3 boxes, the plain crop, the crops of levels 2, 4, 8 aligned and not and one row short or past, the corner where the
    taps clamp, the extreme aspect ratios (the direct path where W is large), four random boxes"""
    oh, ow = size
    out = [(0, 0, H, W), (H // 2, W // 3, 1, 1), (H - 3, W - 3, 3, 3), (1, 2, 3, 3)]
    if oh <= H and ow <= W:
        out += [(H - oh, W - ow, oh, ow), ((H - oh) // 2, (W - ow) // 3, oh, ow)]
    for f in (2, 4, 8):
        if f * oh <= H and f * ow <= W:
            y, x = (H - f * oh) // f * f, (W - f * ow) // f * f
            out += [(y, x, f * oh, f * ow), (0, 0, f * oh, f * ow), (H - f * oh, W - f * ow, f * oh, f * ow), (1, 0, f * oh - 1, f * ow)]
            if f * oh + 1 <= H and f * ow + 1 <= W:
                out += [(0, 0, f * oh + 1, f * ow + 1)]
    hb, wb = min(H, 2 * oh + 1), min(W, 3 * ow + 2)
    out += [(H - hb, W - wb, hb, wb), (H - 8, 0, 8, W), (0, W - 8, H, 8)]
    rng = np.random.default_rng(seed)
    for _ in range(4):
        hb, wb = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        out.append((int(rng.integers(0, H - hb + 1)), int(rng.integers(0, W - wb + 1)), hb, wb))
    return out
