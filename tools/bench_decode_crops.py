#!/usr/bin/env python
"""Windows straight from the factors (lrf_qmf_decode_crops_rgb_u8) against the full decode, on random int8 factors.

  (a) 256 crops of 224x224 out of 256 x 512x768 at (7,3,3)       one crop per image
  (b) the same at (26,13,13)
  (c) 512 crops of 224x224 out of 512 x 1365x2048 at (7,3,3)

Three routes per case, alternating in one process: `crops` (one call, the boxes fresh and random at EVERY call, so the crop table
travels each time), `full_decode` (lrf_qmf_decode_rgb_u8 of the same factors: what had to run before any slicing) and
`full_decode_slice_stack` (that plus the slices stacked into the tensor the crop call returns).  All at the C ABI with buffers
made beforehand.  A run is `--calls` calls between two HIP events; the figure is the median of `--runs` runs per call, with the
smallest and the largest beside it.  Before timing, the crop call's bytes are compared with the sliced full decode.  The bar
(case a): crops < 0.5 x full_decode.  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lrf_amd import _lib  # noqa: E402


class Case:
    def __init__(self, ctx, n, H, W, ranks, size, nlists, seed):
        self.ctx, self.lib, self.n, self.H, self.W, self.size = ctx, _lib.load(), n, H, W, size
        dims = _lib.plane_dims(H, W)
        nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
        g = torch.Generator().manual_seed(seed)
        self.U = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g).cuda()
        self.V = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g).cuda()
        self.R = (ctypes.c_int * 3)(*ranks)
        self.desc = (_lib.RaggedImage * n)()
        for b, d in enumerate(self.desc):
            d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, b * nu, b * nv, 0
            d.R[0], d.R[1], d.R[2] = ranks
        h, w = size
        rng = np.random.default_rng(seed)
        self.lists = [np.ascontiguousarray(np.stack([np.arange(n), rng.integers(0, H - h + 1, n), rng.integers(0, W - w + 1, n)], axis=1), dtype=np.int32)
                      for _ in range(nlists)]
        self.at = 0
        self.out = torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda")
        self.whole = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        self.factor_bytes, self.pixel_bytes = n * (nu + nv), 3 * n * H * W

    def _next(self):
        boxes = self.lists[self.at % len(self.lists)]
        self.at += 1
        return boxes

    def crops(self, boxes=None):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        boxes = self._next() if boxes is None else boxes
        _lib.check(self.lib.lrf_qmf_decode_crops_rgb_u8(self.ctx._h, self.n, self.desc, p(self.U), self.U.numel(), p(self.V), self.V.numel(), self.n,
                                                        boxes.ctypes.data_as(ctypes.POINTER(_lib.Crop)), self.size[0], self.size[1], p(self.out), self.out.numel()))

    def full_decode(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.lrf_qmf_decode_rgb_u8(self.ctx._h, p(self.U), p(self.V), self.n, self.H, self.W, self.R, p(self.whole)))

    def full_decode_slice_stack(self, boxes=None):
        self.full_decode()
        h, w = self.size
        boxes = self._next() if boxes is None else boxes
        return torch.stack([self.whole[b, :, y:y + h, x:x + w] for b, y, x in boxes.tolist()])

    def verify(self):
        for boxes in self.lists[:2]:
            self.crops(boxes)
            want = self.full_decode_slice_stack(boxes)
            torch.cuda.synchronize()
            if not torch.equal(self.out, want):
                raise SystemExit("the crop call differs from the sliced full decode")


def time_routes(routes, runs, calls, warmup):
    for f in routes.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(runs):
        for k, f in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-clic", action="store_true", help="leave out case (c): 4.3 GB of pixels")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r11_decode_crops.json"))
    args = ap.parse_args()
    if args.runs < 7 or args.calls < 20:
        ap.error("at least 7 runs of at least 20 calls")
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = _lib.context(0)
    ctx.use_torch_stream()
    cases = {"a_256x512x768_r7_3_3": (256, 512, 768, (7, 3, 3)), "b_256x512x768_r26_13_13": (256, 512, 768, (26, 13, 13))}
    if not args.skip_clic:
        cases["c_512x1365x2048_r7_3_3"] = (512, 1365, 2048, (7, 3, 3))
    result = dict(tool="tools/bench_decode_crops.py", device=torch.cuda.get_device_name(0), crop=[224, 224], runs=args.runs, calls_per_run=args.calls,
                  fresh_boxes_every_call=True, cases={})
    for name, (n, H, W, ranks) in cases.items():
        c = Case(ctx, n, H, W, ranks, (224, 224), nlists=args.calls, seed=len(name) + n)
        c.verify()
        r = time_routes({"crops": c.crops, "full_decode": c.full_decode, "full_decode_slice_stack": c.full_decode_slice_stack}, args.runs, args.calls,
                        args.warmup)
        r["ratio_crops_over_full_decode"] = r["crops"]["median_ms"] / r["full_decode"]["median_ms"]
        r["ratio_crops_over_full_decode_slice_stack"] = r["crops"]["median_ms"] / r["full_decode_slice_stack"]["median_ms"]
        r["factor_bytes"], r["pixel_bytes"], r["crop_bytes"] = c.factor_bytes, c.pixel_bytes, c.out.numel()
        result["cases"][name] = r
        print(name, json.dumps(r), flush=True)
        del c
        ctx.trim()
        torch.cuda.empty_cache()
    a = result["cases"]["a_256x512x768_r7_3_3"]["ratio_crops_over_full_decode"]
    result["bar"] = dict(case="a_256x512x768_r7_3_3", crops_over_full_decode=a, below=0.5, met=bool(a < 0.5))
    line = json.dumps(result, indent=1)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
