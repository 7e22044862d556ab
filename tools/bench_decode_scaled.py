#!/usr/bin/env python
"""Images at 1/2, 1/4, 1/8 scale straight from the factors (lrf_qmf_decode_scaled_rgb_u8) against the route there was before it:
the full decode followed by block averaging, on random int8 factors.

  (a) 256 x 512x768 at (7,3,3)        sides multiples of 16: the tiled kernel
  (b) 256 x 512x768 at (26,13,13)
  (c) 512 x 1365x2048 at (7,3,3)      odd height: the general kernel (a figure only)

Per case and scale three routes alternate in one process: `scaled` (one call), `full_decode` (lrf_qmf_decode_rgb_u8 of the same
factors alone: what had to run before any pooling) and `full_decode_avg_pool` (that plus torch.nn.functional.avg_pool2d on the
float image, the partial blocks over the pixels that exist).  The decodes run at the C ABI with buffers made beforehand.  A run is
`--calls` calls between two HIP events; the figure is the median of `--runs` runs per call, with the smallest and the largest
beside it.  Before timing, the scaled call's bytes are compared with the pooled full decode (mean absolute difference in
levels: the definition pools before the colour conversion, so the two differ by the truncation bias).  The bar: scaled <
full_decode at every scale on (a) and (b).  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from lrf_amd import _lib  # noqa: E402

SCALES = (2, 4, 8)
CASES = {"a_256x512x768_r7_3_3": (256, 512, 768, (7, 3, 3)), "b_256x512x768_r26_13_13": (256, 512, 768, (26, 13, 13)),
         "c_512x1365x2048_r7_3_3": (512, 1365, 2048, (7, 3, 3))}
ALIGNED = ("a_256x512x768_r7_3_3", "b_256x512x768_r26_13_13")


class Case:
    def __init__(self, ctx, n, H, W, ranks, seed):
        self.ctx, self.lib, self.n, self.H, self.W = ctx, _lib.load(), n, H, W
        dims = _lib.plane_dims(H, W)
        nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
        g = torch.Generator().manual_seed(seed)
        self.U = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g).cuda()
        self.V = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g).cuda()
        self.R = (ctypes.c_int * 3)(*ranks)
        self.whole = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        self.desc, self.out = {}, {}
        for f in SCALES:
            hs, ws = _lib.scaled_dims(H, W, f)
            self.desc[f] = (_lib.RaggedImage * n)()
            for b, d in enumerate(self.desc[f]):
                d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, b * nu, b * nv, b * 3 * hs * ws
                d.R[0], d.R[1], d.R[2] = ranks
            self.out[f] = torch.empty((n, 3, hs, ws), dtype=torch.uint8, device="cuda")
        self.factor_bytes, self.pixel_bytes = n * (nu + nv), 3 * n * H * W

    def scaled(self, f):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.lrf_qmf_decode_scaled_rgb_u8(self.ctx._h, self.n, self.desc[f], f, p(self.U), self.U.numel(), p(self.V), self.V.numel(),
                                                         p(self.out[f]), self.out[f].numel()))

    def full_decode(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.lrf_qmf_decode_rgb_u8(self.ctx._h, p(self.U), p(self.V), self.n, self.H, self.W, self.R, p(self.whole)))

    def full_decode_avg_pool(self, f):
        self.full_decode()
        return torch.nn.functional.avg_pool2d(self.whole.float(), f, ceil_mode=True, count_include_pad=False)

    def difference(self, f):
        """mean |scaled - pooled full decode| in levels, over one eighth of the images"""
        self.scaled(f)
        self.full_decode()
        k = max(1, self.n // 8)
        pooled = torch.nn.functional.avg_pool2d(self.whole[:k].float(), f, ceil_mode=True, count_include_pad=False)
        torch.cuda.synchronize()
        return float((self.out[f][:k].float() - pooled).abs().mean())


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
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-clic", action="store_true", help="leave out case (c): 4.3 GB of pixels, 17 GB as floats")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r15_decode_scaled.json"))
    args = ap.parse_args()
    if args.runs < 7 or args.calls < 20:
        ap.error("at least 7 runs of at least 20 calls")
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = _lib.context(0)
    ctx.use_torch_stream()
    result = dict(tool="tools/bench_decode_scaled.py", device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_run=args.calls, cases={})
    for name, (n, H, W, ranks) in CASES.items():
        if args.skip_clic and name not in ALIGNED:
            continue
        c = Case(ctx, n, H, W, ranks, seed=len(name) + n)
        result["cases"][name] = dict(factor_bytes=c.factor_bytes, pixel_bytes=c.pixel_bytes, scales={})
        for f in SCALES:
            diff = c.difference(f)
            r = time_routes({"scaled": lambda: c.scaled(f), "full_decode": c.full_decode, "full_decode_avg_pool": lambda: c.full_decode_avg_pool(f)},
                            args.runs, args.calls, args.warmup)
            r["ratio_scaled_over_full_decode"] = r["scaled"]["median_ms"] / r["full_decode"]["median_ms"]
            r["ratio_scaled_over_full_decode_avg_pool"] = r["scaled"]["median_ms"] / r["full_decode_avg_pool"]["median_ms"]
            r["scaled_bytes"], r["mean_abs_difference_from_pooled_full_decode"] = c.out[f].numel(), diff
            result["cases"][name]["scales"][str(f)] = r
            print(name, f, json.dumps(r), flush=True)
        del c
        ctx.trim()
        torch.cuda.empty_cache()
    ratios = {f"{name}/{f}": result["cases"][name]["scales"][str(f)]["ratio_scaled_over_full_decode"] for name in ALIGNED for f in SCALES}
    result["bar"] = dict(what="scaled < full_decode at every scale on the 16-aligned cases", scaled_over_full_decode=ratios,
                         met=bool(all(v < 1.0 for v in ratios.values())))
    line = json.dumps(result, indent=1)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
