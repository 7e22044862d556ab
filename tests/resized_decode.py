"""The definition of the resized crops (lrf_qmf_decode_resized_crops_rgb_u8) in numpy, exact integers.  A box of an image is
sampled bilinearly from a level L of it: the uniform decoder's image (f = 1: the oracle's full decode) or
scaled_decode.reference_scaled at f = 2, 4, 8.  test_decode_resized_host.py, test_decode_resized_plan.py and
test_decode_resized_gpu.py share it; every comparison of the kernels with it is bitwise."""
import numpy as np


def resized_level(hb, wb, oh, ow):
    """the largest f of 8, 4, 2 with f oh <= hb and f ow <= wb, else 1"""
    for f in (8, 4, 2):
        if f * oh <= hb and f * ow <= wb:
            return f
    return 1


def taps(n_out, b0, nb, f, n_lvl):
    """-> (i0, i1, t) int64 [n_out]: the two level rows (columns) every output row (column) reads and the second's weight in 1/256"""
    r = np.arange(n_out, dtype=np.int64)
    N = (2 * r + 1) * nb + 2 * n_out * b0 - n_out * f
    D = 2 * n_out * f
    q = np.clip((256 * N) // D, 0, 256 * (n_lvl - 1))  # (numpy's // floors)
    i0 = q >> 8
    return i0, np.minimum(i0 + 1, n_lvl - 1), q & 255


def reference_resized(L, box, size, flip=False):
    """L: uint8 [3, Hs, Ws], the level resized_level names for the box; box: (y0, x0, hb, wb) in full-resolution pixels;
    size: (oh, ow) -> uint8 [3, oh, ow]"""
    y0, x0, hb, wb = box
    oh, ow = size
    f = resized_level(hb, wb, oh, ow)
    _, Hs, Ws = L.shape
    iy0, iy1, ty = taps(oh, y0, hb, f, Hs)
    ix0, ix1, tx = taps(ow, x0, wb, f, Ws)
    A = L.astype(np.int64)
    ty, tx = ty[None, :, None], tx[None, None, :]
    out = ((256 - ty) * (256 - tx) * A[:, iy0][:, :, ix0] + (256 - ty) * tx * A[:, iy0][:, :, ix1] + ty * (256 - tx) * A[:, iy1][:, :, ix0]
           + ty * tx * A[:, iy1][:, :, ix1] + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    return np.ascontiguousarray(out[:, :, ::-1]) if flip else out


def float_bilinear(L, box, size):
    """real-valued bilinear interpolation of L at the same centres, taps clamped into the level: float64 [3, oh, ow]"""
    y0, x0, hb, wb = box
    oh, ow = size
    f = resized_level(hb, wb, oh, ow)
    _, Hs, Ws = L.shape

    def axis(n_out, b0, nb, n_lvl):
        p = np.clip(((np.arange(n_out) + 0.5) * nb / n_out + b0) / f - 0.5, 0, n_lvl - 1)
        i0 = np.minimum(np.floor(p).astype(np.int64), n_lvl - 1)
        return i0, np.minimum(i0 + 1, n_lvl - 1), p - i0

    iy0, iy1, ty = axis(oh, y0, hb, Hs)
    ix0, ix1, tx = axis(ow, x0, wb, Ws)
    A = L.astype(np.float64)
    ty, tx = ty[None, :, None], tx[None, None, :]
    return ((1 - ty) * (1 - tx) * A[:, iy0][:, :, ix0] + (1 - ty) * tx * A[:, iy0][:, :, ix1] + ty * (1 - tx) * A[:, iy1][:, :, ix0]
            + ty * tx * A[:, iy1][:, :, ix1])
