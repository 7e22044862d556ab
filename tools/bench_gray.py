#!/usr/bin/env python
"""The gray route (lrf_qmf_encode_gray_u8 / lrf_qmf_decode_gray_u8) beside the colour route it was modelled on, on 256 images of
512x768: bilinear-upsampled noise plus N(0, 4), one channel for the gray calls, three for the colour calls.

  encode   gray at rank 7 and at quality 7 (R = 4)   against   lrf_qmf_encode_rgb_u8 at (7,3,3) and (4,2,2), K = 10, bounds (-16, 15)
  decode   lrf_qmf_decode_gray_u8 at R = 7 and 4      against   lrf_qmf_decode_rgb_u8 at (7,3,3) and (4,2,2), on the encoders' factors
  general  lrf_qmf_chan_matrix_u8 + lrf_qmf_decompose_f32 and lrf_qmf_chan_decode_u8 on the same gray batch (figures only)

The bar follows from the work: a gray image has 6144 of the colour image's 9216 plane rows, no colour conversion and a third of
the output bytes, so each gray call must take no longer than the colour call beside it (bar.met).  Also recorded: the gray
encode's share of the 8 TB/s peak at 1 + 4 + 4 (K + 1) = 49 bytes per pixel (image read, X written, X read again by the
initialisation and the K iterations).

Everything runs at the C ABI.  A run is `--calls` calls between two HIP events, the routes alternated in one process; the figure is
the median of `--runs` runs per call, with the smallest and the largest beside it.  Before timing, the gray routes' outputs are
compared bitwise with the general route's; a difference ends the run with an error.  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from lrf_amd import _lib  # noqa: E402

B, H, W, K, LO, HI = 256, 512, 768, 10, -16, 15
PAIRS = {"r7": (7, (7, 3, 3)), "q7": (4, (4, 2, 2))}
PEAK = 8.0e12


def images(C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.rand((B, C, H // 8, W // 8), device="cuda", generator=g) * 255
    img = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    return (img + torch.randn(img.shape, device="cuda", generator=g) * 4).clamp(0, 255).to(torch.uint8).contiguous()


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def time_routes(routes, runs, calls, warmup):
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(runs):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r22_gray.json"))
    args = ap.parse_args()
    if args.runs < 7 or args.calls < 3:
        ap.error("at least 7 runs of at least 3 calls")
    assert torch.cuda.is_available(), "needs a GPU"
    lib = _lib.load()
    ctx = _lib.context(0)
    ctx.use_torch_stream()
    h = ctx._h
    gray, rgb = images(1, 22), images(3, 23)
    M = _lib.chan_dims(H, W, 1, (8, 8))[2]
    dims = _lib.plane_dims(H, W)
    X = torch.empty((B, M, 64), dtype=torch.float32, device="cuda")
    result = dict(tool="tools/bench_gray.py", device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_run=args.calls, batch=[B, H, W],
                  num_iters=K, bounds=[LO, HI], pairs={})
    met = {}
    for name, (R, triple) in PAIRS.items():
        Ug = torch.empty((B, M, R), dtype=torch.int8, device="cuda")
        Vg = torch.empty((B, 64, R), dtype=torch.int8, device="cuda")
        Ua, Va = torch.empty_like(Ug), torch.empty_like(Vg)
        Uc = torch.empty((B, sum(d[4] * r for d, r in zip(dims, triple))), dtype=torch.int8, device="cuda")
        Vc = torch.empty((B, 64 * sum(triple)), dtype=torch.int8, device="cuda")
        Rc = (ctypes.c_int * 3)(*triple)
        out_g = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
        out_a = torch.empty_like(out_g)
        out_c = torch.empty((B, 3, H, W), dtype=torch.uint8, device="cuda")

        def gray_encode():
            _lib.check(lib.lrf_qmf_encode_gray_u8(h, p(gray), B, H, W, R, K, LO, HI, None, None, None, p(Ug), p(Vg)))

        def general_encode():
            _lib.check(lib.lrf_qmf_chan_matrix_u8(h, p(gray), B, 1, H, W, 8, 8, p(X)))
            _lib.check(lib.lrf_qmf_decompose_f32(h, p(X), B, M, 64, R, K, LO, HI, None, p(Ua), p(Va)))

        def colour_encode():
            _lib.check(lib.lrf_qmf_encode_rgb_u8(h, p(rgb), B, H, W, Rc, K, LO, HI, None, p(Uc), p(Vc)))

        def gray_decode():
            _lib.check(lib.lrf_qmf_decode_gray_u8(h, p(Ug), p(Vg), B, H, W, R, p(out_g)))

        def general_decode():
            _lib.check(lib.lrf_qmf_chan_decode_u8(h, p(Ug), p(Vg), B, 1, H, W, 8, 8, R, p(out_a)))

        def colour_decode():
            _lib.check(lib.lrf_qmf_decode_rgb_u8(h, p(Uc), p(Vc), B, H, W, Rc, p(out_c)))

        for fn in (gray_encode, general_encode, colour_encode, gray_decode, general_decode, colour_decode):
            fn()
        torch.cuda.synchronize()
        ctx.check()
        if not (torch.equal(Ug, Ua) and torch.equal(Vg, Va)):  # bits first: nothing is timed that computes something else
            sys.exit(f"{name}: the gray encode differs from lrf_qmf_decompose_f32 on the same X: not timed")
        if not torch.equal(out_g, out_a):
            sys.exit(f"{name}: the gray decode differs from the general decoder: not timed")
        mse = torch.mean((out_g.float() - gray[:, 0].float()) ** 2).item()
        r = time_routes({"gray_encode": gray_encode, "colour_encode": colour_encode, "general_encode": general_encode,
                         "gray_decode": gray_decode, "colour_decode": colour_decode, "general_decode": general_decode}, args.runs, args.calls,
                        args.warmup)
        r["bitwise_equal"] = True
        r["gray_rank"], r["colour_ranks"] = R, list(triple)
        r["gray_psnr_db"] = 10 * torch.log10(torch.tensor(255.0 ** 2 / mse)).item()
        r["ratio_gray_over_colour_encode"] = r["gray_encode"]["median_ms"] / r["colour_encode"]["median_ms"]
        r["ratio_gray_over_colour_decode"] = r["gray_decode"]["median_ms"] / r["colour_decode"]["median_ms"]
        r["gray_encode_bytes_per_pixel"] = 1 + 4 + 4 * (K + 1)
        r["gray_encode_share_of_8TBps"] = (1 + 4 + 4 * (K + 1)) * B * H * W / (r["gray_encode"]["median_ms"] * 1e-3) / PEAK
        r["gray_decode_GBps_written"] = B * H * W / (r["gray_decode"]["median_ms"] * 1e-3) / 1e9
        met[name + "_encode"] = r["ratio_gray_over_colour_encode"] <= 1.0
        met[name + "_decode"] = r["ratio_gray_over_colour_decode"] <= 1.0
        result["pairs"][name] = r
        print(name, json.dumps(r), flush=True)
    result["bar"] = dict(what="each gray call takes no longer than the colour call beside it (medians)", calls=met, met=bool(all(met.values())))
    line = json.dumps(result, indent=1)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
