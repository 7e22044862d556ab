"""The reference of the decode at 1/2, 1/4, 1/8 scale (lrf_qmf_decode_scaled_rgb_u8) in numpy and the CPU oracle: the decoder
with an area pooling in front of its colour conversion.  Per plane the decoder's integers are summed exactly (int64) over the
image pixels an output pixel covers — blocks aligned to the image, the partial ones at the bottom and right edge holding the
pixels that exist — the mean is float32(sum) / float32(count), and the means go through the oracle's lrf_oracle_ycbcr_to_rgb
and to_u8.  test_decode_scaled_host.py, test_decode_scaled_plan.py and test_decode_scaled_gpu.py share it; every comparison of
the kernels with it is bitwise."""
import ctypes

import numpy as np

SCALES = (2, 4, 8)


def scaled_dims(H, W, f):
    return -(-H // f), -(-W // f)


def int_plane(u, v, h, w):
    """int8 [M, R], [64, R] -> int64 [h, w]: the decoder's plane (u @ v.mT, depatchify, unpad)"""
    hp, wp = h + (-h) % 8, w + (-w) % 8
    X = u.astype(np.int64) @ v.astype(np.int64).T
    pl = X.reshape(hp // 8, wp // 8, 8, 8).transpose(0, 2, 1, 3).reshape(hp, wp)
    t, l = (hp - h) // 2, (wp - w) // 2
    return pl[t:t + h, l:l + w]


def nearest_idx(n_out, n_in):
    """ATen's nearest source index of every output index, the scale in fp32"""
    s = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * s).astype(np.int64), n_in - 1)


def block_sum(a, f):
    """int64 [H, W] -> [ceil(H / f), ceil(W / f)]: sums over the f x f blocks, the partial ones over what exists"""
    H, W = a.shape
    Hs, Ws = scaled_dims(H, W, f)
    return np.pad(a, ((0, Hs * f - H), (0, Ws * f - W))).reshape(Hs, f, Ws, f).sum(axis=(1, 3))


def ycc_to_u8(ycc, oracle):
    """float32 [3, h, w] plane means -> uint8 [3, h, w] through the oracle's colour conversion and to_dtype"""
    ycc = np.ascontiguousarray(ycc, dtype=np.float32)
    _, h, w = ycc.shape
    out = np.empty_like(ycc)
    fp = ctypes.POINTER(ctypes.c_float)
    oracle.lib().lrf_oracle_ycbcr_to_rgb(ycc.ctypes.data_as(fp), ctypes.c_long(h), ctypes.c_long(w), out.ctypes.data_as(fp))
    return oracle.to_u8(out)


def reference_scaled(f6, H, W, f, oracle):
    """f6 = [u_y, v_y, u_cb, v_cb, u_cr, v_cr] int8 -> uint8 [3, ceil(H / f), ceil(W / f)]"""
    hc, wc = H // 2, W // 2
    iy, ix = nearest_idx(H, hc), nearest_idx(W, wc)
    planes = [int_plane(f6[0], f6[1], H, W)] + [int_plane(f6[2 * c], f6[2 * c + 1], hc, wc)[iy][:, ix] for c in (1, 2)]
    n = block_sum(np.ones((H, W), np.int64), f).astype(np.float32)
    sums = [block_sum(p, f) for p in planes]
    assert all(int(np.abs(s).max()) < 2 ** 31 for s in sums)
    return ycc_to_u8(np.stack([s.astype(np.float32) / n for s in sums]), oracle)


def block_average_u8(img, f):
    """uint8 [3, H, W] -> float64 [3, ceil(H / f), ceil(W / f)]: the decoded image block-averaged, what a caller had before"""
    n = block_sum(np.ones(img.shape[1:], np.int64), f)
    return np.stack([block_sum(img[c].astype(np.int64), f) / n for c in range(3)])


def random_factors(rng, H, W, ranks, lo=-16, hi=16, vlo=None, vhi=None):
    """flat int8 (U, V) of one image in encode_rgb's layout: U in [lo, hi), V in [vlo, vhi) (default: as U)"""
    from lrf_amd import _lib
    dims = _lib.plane_dims(H, W)
    vlo, vhi = (lo if vlo is None else vlo), (hi if vhi is None else vhi)
    return (rng.integers(lo, hi, sum(d[4] * r for d, r in zip(dims, ranks)), dtype=np.int8), rng.integers(vlo, vhi, 64 * sum(ranks), dtype=np.int8))
