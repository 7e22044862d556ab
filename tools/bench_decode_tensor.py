#!/usr/bin/env python
"""Model-ready resized crops in one call (lrf_qmf_decode_resized_crops_tensor) against what a caller had before it: the uint8
entry followed by torch's to-tensor and normalise chain into a preallocated result.  Random int8 factors, 256 images of 512x768,
one box per image drawn as torchvision's RandomResizedCrop draws it, resampled to 224x224, the ImageNet constants.

  cases     (7,3,3): the decode8 fill (the bar); (26,13,13): the general fill (a figure only)
  formats   float16 NCHW, bfloat16 NHWC

Routes, alternated in one process:
  tensor      lrf_qmf_decode_resized_crops_tensor into a preallocated tensor
  u8_chain    lrf_qmf_decode_resized_crops_rgb_u8 into a preallocated uint8 batch, then
              x.float().mul_(scale).add_(bias) and result.copy_(...) — the copy converts to the dtype and, for NHWC, to
              channels_last memory in one kernel: what `.to(dtype).contiguous(memory_format=...)` does, without its allocations
  u8          the uint8 entry alone (the ratio tensor / u8 is recorded, not barred)
The decodes run at the C ABI.  A run is `--calls` calls between two HIP events; the figure is the median of `--runs` runs per
call, with the smallest and the largest beside it.  Before timing the two routes' tensors are compared bitwise: a difference ends
the run with an error.  The bar: tensor < u8_chain for both formats at (7,3,3).  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_decode_resized import SIZE, level_of, random_resized_crop_box  # noqa: E402
from lrf_amd import _lib  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = {"a_256x512x768_r7_3_3": (256, 512, 768, (7, 3, 3)), "b_256x512x768_r26_13_13": (256, 512, 768, (26, 13, 13))}
FORMATS = {"float16_nchw": (torch.float16, False), "bfloat16_nhwc": (torch.bfloat16, True)}
BAR = "a_256x512x768_r7_3_3"


class Case:
    def __init__(self, ctx, n, H, W, ranks, seed):
        self.ctx, self.lib, self.n = ctx, _lib.load(), n
        dims = _lib.plane_dims(H, W)
        nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
        g = torch.Generator().manual_seed(seed)
        self.U = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g).cuda()
        self.V = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g).cuda()
        rng = np.random.default_rng(seed)
        self.boxes = [random_resized_crop_box(rng, H, W) for _ in range(n)]
        self.levels = [level_of(b[2], b[3]) for b in self.boxes]
        self.crops = (_lib.ResizedCrop * n)()
        for j, (c, (y0, x0, hb, wb)) in enumerate(zip(self.crops, self.boxes)):
            c.image, c.y0, c.x0, c.h, c.w, c.flip = j, y0, x0, hb, wb, int(rng.integers(0, 2))
        self.desc = (_lib.RaggedImage * n)()
        for b, d in enumerate(self.desc):
            d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, b * nu, b * nv, 0
            d.R[0], d.R[1], d.R[2] = ranks
        self.u8 = torch.empty((n, 3) + SIZE, dtype=torch.uint8, device="cuda")
        self.f32 = torch.empty((n, 3) + SIZE, dtype=torch.float32, device="cuda")

    def set_format(self, dtype, channels_last):
        self.fmt = _lib.check_tensor_format(dtype, MEAN, STD, channels_last)
        mf = torch.channels_last if channels_last else torch.contiguous_format
        self.out = torch.empty((self.n, 3) + SIZE, dtype=dtype, device="cuda", memory_format=mf)
        self.chain_out = torch.empty_like(self.out, memory_format=mf)
        self.scale = torch.tensor(list(self.fmt.scale), dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
        self.bias = torch.tensor(list(self.fmt.bias), dtype=torch.float32, device="cuda").view(1, 3, 1, 1)

    def _args(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        return (self.ctx._h, self.n, self.desc, p(self.U), self.U.numel(), p(self.V), self.V.numel(), self.n, self.crops, SIZE[0], SIZE[1])

    def tensor(self):
        _lib.check(self.lib.lrf_qmf_decode_resized_crops_tensor(*self._args(), ctypes.byref(self.fmt), ctypes.c_void_p(self.out.data_ptr()),
                                                                self.out.numel() * self.out.element_size()))

    def u8_only(self):
        _lib.check(self.lib.lrf_qmf_decode_resized_crops_rgb_u8(*self._args(), ctypes.c_void_p(self.u8.data_ptr()), self.u8.numel()))

    def u8_chain(self):
        self.u8_only()
        self.f32.copy_(self.u8)  # x.float() into a preallocated buffer
        self.f32.mul_(self.scale).add_(self.bias)
        self.chain_out.copy_(self.f32)  # .to(dtype).contiguous(memory_format=...) in one kernel


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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r21_decode_tensor.json"))
    args = ap.parse_args()
    if args.runs < 7 or args.calls < 20:
        ap.error("at least 7 runs of at least 20 calls")
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = _lib.context(0)
    ctx.use_torch_stream()
    result = dict(tool="tools/bench_decode_tensor.py", device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_run=args.calls, size=list(SIZE),
                  mean=list(MEAN), std=list(STD), cases={})
    for name, (n, H, W, ranks) in CASES.items():
        c = Case(ctx, n, H, W, ranks, seed=len(name) + n)
        result["cases"][name] = dict(boxes_per_level={str(f): c.levels.count(f) for f in sorted(set(c.levels))}, formats={})
        for fname, (dtype, cl) in FORMATS.items():
            c.set_format(dtype, cl)
            c.tensor()
            c.u8_chain()
            torch.cuda.synchronize()
            bits = lambda t: t.contiguous().view(torch.int16)
            if not torch.equal(bits(c.out), bits(c.chain_out)):  # bits first: nothing is timed that computes something else
                sys.exit(f"{name} {fname}: the two routes differ on {int((bits(c.out) != bits(c.chain_out)).sum())} elements: not timed")
            r = time_routes({"tensor": c.tensor, "u8_chain": c.u8_chain, "u8": c.u8_only}, args.runs, args.calls, args.warmup)
            r["bitwise_equal"] = True
            r["ratio_tensor_over_u8_chain"] = r["tensor"]["median_ms"] / r["u8_chain"]["median_ms"]
            r["ratio_tensor_over_u8"] = r["tensor"]["median_ms"] / r["u8"]["median_ms"]
            r["output_bytes"], r["u8_bytes"] = c.out.numel() * c.out.element_size(), c.u8.numel()
            result["cases"][name]["formats"][fname] = r
            print(name, fname, json.dumps(r), flush=True)
        del c
        ctx.trim()
        torch.cuda.empty_cache()
    a = result["cases"][BAR]["formats"]
    result["bar"] = dict(what="tensor < u8_chain for both formats at (7,3,3)", ratios={k: v["ratio_tensor_over_u8_chain"] for k, v in a.items()},
                         met=bool(all(v["ratio_tensor_over_u8_chain"] < 1.0 for v in a.values())))
    line = json.dumps(result, indent=1)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
