"""The image pairs tests/test_metrics_device.py and tests/test_metrics_gpu.py score, and the exact-integer restatement of the SSIM
contract of lrf_image_metrics_u8 (include/lrf_hip.h; DESIGN.md, "Metrics on the device") both lean on."""
import math

import numpy as np

SSIM_BAR = 1e-9   # float64 rounding of ~20 operations per window and the order of <= 1.2e6 additions: n 2^-53 ~ 1.3e-10 at worst
PSNR_BAR = 1e-4   # dB: metrics.psnr is float32 (2 ulp at 64 dB = 1.5e-5 dB)
SIZES = [(512, 768), (61, 47), (7, 7), (8, 200), (333, 129)]


def pairs_of_size(H, W, rng, C=3):
    """(name, a, b) uint8 [C,H,W] pairs: uniform noise of amplitude 0/1/6/40/255 on a random image, a ramp image, and a
    constant-128 image with one pixel changed (data_range 1) against itself and against noise"""
    a = rng.integers(0, 256, (C, H, W), dtype=np.uint8)
    for amp in (0, 1, 6, 40, 255):
        yield f"{H}x{W} noise {amp}", a, np.clip(a.astype(int) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    g = ((yy * 3 + xx * 2) % 256).astype(np.uint8)
    a = np.stack([g, g // 2, 255 - g][:C])
    yield f"{H}x{W} ramp", a, np.clip(a.astype(int) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    a = np.full((C, H, W), 128, np.uint8)
    a[0, 0, 0] = 129
    yield f"{H}x{W} range 1, equal", a, a.copy()
    yield f"{H}x{W} range 1, noise", a, np.clip(a.astype(int) + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)


def cases():
    """the 40 pairs of the five sizes"""
    rng = np.random.default_rng(1)
    for H, W in SIZES:
        yield from pairs_of_size(H, W, rng)


def _box(x):
    """sums over every 7x7 window that lies inside x, int64, from the integral image"""
    c = np.cumsum(np.cumsum(np.pad(x, ((1, 0), (1, 0))), 0), 1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim_contract(a, b):
    """The contract: integer window sums, 49 Sxx - Sx^2 etc. in integers, one conversion to float64, then the formula."""
    L = int(a.max()) - int(a.min())
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    out = []
    for x, y in zip(a.astype(np.int64), b.astype(np.int64)):
        sx, sy, sxx, syy, sxy = _box(x), _box(y), _box(x * x), _box(y * y), _box(x * y)
        ux, uy = sx / 49.0, sy / 49.0
        vx, vy, vxy = (49 * sxx - sx * sx) / (49.0 * 48.0), (49 * syy - sy * sy) / (49.0 * 48.0), (49 * sxy - sx * sy) / (49.0 * 48.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        out.append(s.mean())
    return float(np.mean(out))


def sse_exact(a, b):
    return int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())


def psnr_contract(a, b, max_value=255):
    sse = sse_exact(a, b)
    return 20 * math.log10(max_value / math.sqrt(sse / a.size)) if sse else float("inf")
