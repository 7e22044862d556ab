"""The definitions of the gray loader (lrf_qmf_decode_gray_ragged_u8, lrf_qmf_decode_gray_crops_u8,
lrf_qmf_decode_gray_resized_crops_u8 and the _tensor forms; include/lrf_hip.h) in numpy, exact integers, and the inputs
test_gray_loader.py, test_gray_loader_plan.py and test_gray_loader_gpu.py share.  Every comparison of the kernels with these
functions is bitwise.

  P        scaled_decode.int_plane(u, v, H, W): int64 u @ v.T, depatchified, centre-cropped
  level 1  clip(P, 0, 255)
  level f  f = 2, 4, 8: s = the exact sum of P over the f x f block of image pixels (blocks aligned to the image, the partial ones
           at the bottom and right edge holding the n pixels that exist), clip(s, 0, 255 n) // n: pooled before the clamp
  resized  resized_decode.reference_resized on the level resized_level names, as a [1, Hs, Ws] array
  tensor   t = fl32(b * scale[0]); v = fl32(t + bias[0]); rounded to nearest even into the dtype: torch's mul, add, .to() on the CPU"""
import functools

import numpy as np

from resized_decode import reference_resized, resized_level
from scaled_decode import block_sum, int_plane

SIZES = [(8, 8), (16, 24), (37, 53), (64, 96), (56, 440), (173, 264)]  # M = 1, 6, 35, 96, 385, 726
RANKS = [1, 4, 7, 8, 9, 16, 17, 32, 33, 64]  # R % 4 != 0 byte reads of U, ranks above M
TONES = {"dark": None, "mid": (8, 15), "bright": (15, 17)}  # constants that overwrite column 0 of u / v
LEVELS = (1, 2, 4, 8)
MEAN, STD = 0.449, 0.226  # the tensor tests' constants: a contracted multiply-add differs on 124 of the 256 byte values


def padded(H, W):
    return H + (-H) % 8, W + (-W) % 8


def patches(H, W):
    hp, wp = padded(H, W)
    return (hp // 8) * (wp // 8)


def scaled_dims(H, W, f):
    return -(-H // f), -(-W // f)


@functools.lru_cache(maxsize=None)
def case_factors(H, W, R, tone):
    """int8 (u [M, R], v [64, R]) of one case: uniform in [-a, a), a = 6 up to rank 16 and 4 above; u is drawn first"""
    rng = np.random.default_rng(100003 * H + 101 * W + R)
    a = 6 if R <= 16 else 4
    u = rng.integers(-a, a, (patches(H, W), R), dtype=np.int8)
    v = rng.integers(-a, a, (64, R), dtype=np.int8)
    if TONES[tone] is not None:
        u[:, 0], v[:, 0] = TONES[tone]
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def level_of_plane(P, f):
    """int64 [H, W] -> uint8 [ceil(H / f), ceil(W / f)]"""
    if f == 1:
        return np.clip(P, 0, 255).astype(np.uint8)
    s, n = block_sum(P, f), block_sum(np.ones(P.shape, np.int64), f)
    assert int(np.abs(s).max()) <= 2 ** 26
    return (np.clip(s, 0, 255 * n) // n).astype(np.uint8)


def level(u, v, H, W, f):
    return level_of_plane(int_plane(u, v, H, W), f)


def resized(u, v, H, W, box, size, flip=False):
    """box: (y0, x0, hb, wb) in full-resolution pixels; size: (oh, ow) -> uint8 [oh, ow]"""
    f = resized_level(box[2], box[3], *size)
    return reference_resized(level(u, v, H, W, f)[None], box, size, flip)[0]


def constants(mean=None, std=None):
    """(scale, bias) as float32 numbers: float32(1 / (255 std)) and float32(-mean / std), from Python doubles, rounded once"""
    m, s = (0.0 if mean is None else float(mean)), (1.0 if std is None else float(std))
    return np.float32(1.0 / (255.0 * s)), np.float32(-m / s)


def tensor_of(b, scale, bias, dtype):
    """b: uint8 array -> the definition's CPU tensor of `dtype`, same shape"""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(b))
    return t.float().mul(torch.tensor(float(scale), dtype=torch.float32)).add(torch.tensor(float(bias), dtype=torch.float32)).to(dtype)


def flat_list(cases):
    """cases: [(H, W, R, tone)] -> ([(H, W, R, u_off, v_off)], U int8 flat, V int8 flat): the factors back to back, as
    qmf_load_factors lays out a list of gray streams"""
    images, us, vs, uo, vo = [], [], [], 0, 0
    for H, W, R, tone in cases:
        u, v = case_factors(H, W, R, tone)
        images.append((H, W, R, uo, vo))
        us.append(u.reshape(-1))
        vs.append(v.reshape(-1))
        uo += u.size
        vo += v.size
    return images, np.concatenate(us), np.concatenate(vs)


ALL_CASES = [(H, W, R, tone) for (H, W) in SIZES for R in RANKS for tone in TONES]


def shuffled_cases(seed=5):
    order = np.random.default_rng(seed).permutation(len(ALL_CASES))
    return [ALL_CASES[i] for i in order]
