#!/usr/bin/env python
"""Resized crops straight from the factors (lrf_qmf_decode_resized_crops_rgb_u8) against the route a caller had before it, on
random int8 factors: one box per image, drawn as torchvision's RandomResizedCrop draws it (area fraction uniform in [0.08, 1],
aspect ratio log-uniform in [3/4, 4/3], the centre fallback), resampled to 224x224.

  (a) 256 x 512x768 at (7,3,3)        ranks <= 8: the decode8 fill                    (the bar)
  (b) 256 x 512x768 at (26,13,13)     the general fill                                (a figure only)
  (c) 512 x 1365x2048 at (7,3,3)      larger boxes: levels 2 and 4 take most of them  (a figure only)

Three routes alternate in one process: `resized` (one call), `levels_interpolate` (lrf_qmf_decode_rgb_u8 /
lrf_qmf_decode_scaled_rgb_u8 once per level the boxes use, then per crop a slice of its level and
torch.nn.functional.interpolate(mode="bilinear", antialias=False), then a stack: the same tensor shape) and `full_decode`
(lrf_qmf_decode_rgb_u8 alone).  The decodes run at the C ABI with buffers made beforehand.  A run is `--calls` calls between two
HIP events; the figure is the median of `--runs` runs per call, with the smallest and the largest beside it.  Before timing the
bytes of the two routes are compared: they are not the same definition (the old route interpolates in floating point over a
slice rounded outwards to whole level pixels), so the figures are the mean and the largest absolute difference in levels, over
all crops and over those sampled from level 1 out of boxes no smaller than the output, where the two differ by the 2.5 levels of the fixed-point taps and torch's
rounding only: more than 3 levels there ends the run with an error before anything is timed.  The bar: resized < levels_interpolate on (a).  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lrf_amd import _lib  # noqa: E402

SIZE = (224, 224)
CASES = {"a_256x512x768_r7_3_3": (256, 512, 768, (7, 3, 3)), "b_256x512x768_r26_13_13": (256, 512, 768, (26, 13, 13)),
         "c_512x1365x2048_r7_3_3": (512, 1365, 2048, (7, 3, 3))}
BAR = "a_256x512x768_r7_3_3"


def random_resized_crop_box(rng, H, W):
    for _ in range(10):
        area = H * W * rng.uniform(0.08, 1.0)
        ar = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
    r = W / H
    w, h = (W, int(round(W / (4 / 3)))) if r > 4 / 3 else ((int(round(H * 3 / 4)), H) if r < 3 / 4 else (W, H))
    return (H - h) // 2, (W - w) // 2, h, w


def level_of(hb, wb):
    for f in (8, 4, 2):
        if f * SIZE[0] <= hb and f * SIZE[1] <= wb:
            return f
    return 1


class Case:
    def __init__(self, ctx, n, H, W, ranks, seed):
        self.ctx, self.lib, self.n, self.H, self.W = ctx, _lib.load(), n, H, W
        dims = _lib.plane_dims(H, W)
        nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
        g = torch.Generator().manual_seed(seed)
        self.U = torch.randint(-16, 16, (n, nu), dtype=torch.int8, generator=g).cuda()
        self.V = torch.randint(-16, 16, (n, nv), dtype=torch.int8, generator=g).cuda()
        self.R = (ctypes.c_int * 3)(*ranks)
        rng = np.random.default_rng(seed)
        self.boxes = [random_resized_crop_box(rng, H, W) for _ in range(n)]
        self.flips = [int(rng.integers(0, 2)) for _ in range(n)]
        self.levels = [level_of(b[2], b[3]) for b in self.boxes]
        self.crops = (_lib.ResizedCrop * n)()
        for j, (c, (y0, x0, hb, wb)) in enumerate(zip(self.crops, self.boxes)):
            c.image, c.y0, c.x0, c.h, c.w, c.flip = j, y0, x0, hb, wb, self.flips[j]
        self.desc, self.lvl = {}, {}
        for f in sorted(set(self.levels) | {1}):
            hs, ws = (H, W) if f == 1 else _lib.scaled_dims(H, W, f)
            self.desc[f] = (_lib.RaggedImage * n)()
            for b, d in enumerate(self.desc[f]):
                d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, b * nu, b * nv, b * 3 * hs * ws
                d.R[0], d.R[1], d.R[2] = ranks
            self.lvl[f] = torch.empty((n, 3, hs, ws), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((n, 3) + SIZE, dtype=torch.uint8, device="cuda")
        self.factor_bytes, self.level1_bytes = n * (nu + nv), 3 * n * H * W

    def resized(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.lrf_qmf_decode_resized_crops_rgb_u8(self.ctx._h, self.n, self.desc[1], p(self.U), self.U.numel(), p(self.V), self.V.numel(), self.n,
                                                                self.crops, SIZE[0], SIZE[1], p(self.out), self.out.numel()))

    def full_decode(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.lrf_qmf_decode_rgb_u8(self.ctx._h, p(self.U), p(self.V), self.n, self.H, self.W, self.R, p(self.lvl[1])))

    def levels_interpolate(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        for f in sorted(set(self.levels)):
            if f == 1:
                self.full_decode()
            else:
                _lib.check(self.lib.lrf_qmf_decode_scaled_rgb_u8(self.ctx._h, self.n, self.desc[f], f, p(self.U), self.U.numel(), p(self.V), self.V.numel(),
                                                                 p(self.lvl[f]), self.lvl[f].numel()))
        outs = []
        for j, ((y0, x0, hb, wb), f) in enumerate(zip(self.boxes, self.levels)):
            sl = self.lvl[f][j:j + 1, :, y0 // f:-(-(y0 + hb) // f), x0 // f:-(-(x0 + wb) // f)].float()
            o = torch.nn.functional.interpolate(sl, size=SIZE, mode="bilinear", antialias=False)
            outs.append(o.flip(3) if self.flips[j] else o)
        return torch.cat(outs).add_(0.5).clamp_(0, 255).to(torch.uint8)

    def difference(self):
        self.resized()
        old = self.levels_interpolate()
        torch.cuda.synchronize()
        d = (self.out.float() - old.float()).abs()
        # level-1 boxes no smaller than the output: every tap lies inside the box, so the old route's slice holds it too (a smaller
        # box reads, by the definition, the level pixels around it, where interpolate clamps to the slice's edge)
        one = torch.tensor([f == 1 and b[2] >= SIZE[0] and b[3] >= SIZE[1] for f, b in zip(self.levels, self.boxes)], device="cuda")
        r = dict(mean_abs=float(d.mean()), max_abs=float(d.max()))
        if bool(one.any()):
            r.update(level1_mean_abs=float(d[one].mean()), level1_max_abs=float(d[one].max()), level1_within_3_levels=bool(d[one].max() <= 3.0))
        return r


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
    ap.add_argument("--skip-clic", action="store_true", help="leave out case (c): 4.3 GB of pixels")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r16_decode_resized.json"))
    args = ap.parse_args()
    if args.runs < 7 or args.calls < 20:
        ap.error("at least 7 runs of at least 20 calls")
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = _lib.context(0)
    ctx.use_torch_stream()
    result = dict(tool="tools/bench_decode_resized.py", device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_run=args.calls, size=list(SIZE), cases={})
    for name, (n, H, W, ranks) in CASES.items():
        if args.skip_clic and name.startswith("c_"):
            continue
        c = Case(ctx, n, H, W, ranks, seed=len(name) + n)
        diff = c.difference()  # bytes first: a wrong box mapping ends the run here, before anything is timed
        if "level1_max_abs" in diff and diff["level1_max_abs"] > 3.0:
            sys.exit(f"{name}: the two routes differ by {diff['level1_max_abs']} levels on the level-1 crops no smaller than the output (at most 3 expected): not timed")
        r = time_routes({"resized": c.resized, "levels_interpolate": c.levels_interpolate, "full_decode": c.full_decode}, args.runs, args.calls, args.warmup)
        r["difference_in_levels"] = diff
        r["ratio_resized_over_levels_interpolate"] = r["resized"]["median_ms"] / r["levels_interpolate"]["median_ms"]
        r["ratio_resized_over_full_decode"] = r["resized"]["median_ms"] / r["full_decode"]["median_ms"]
        r["boxes_per_level"] = {str(f): c.levels.count(f) for f in sorted(set(c.levels))}
        r["factor_bytes"], r["level1_bytes"], r["output_bytes"] = c.factor_bytes, c.level1_bytes, c.out.numel()
        result["cases"][name] = r
        print(name, json.dumps(r), flush=True)
        del c
        ctx.trim()
        torch.cuda.empty_cache()
    a = result["cases"][BAR]
    result["bar"] = dict(what="resized < levels_interpolate on (a)", resized_ms=a["resized"]["median_ms"], levels_interpolate_ms=a["levels_interpolate"]["median_ms"],
                         ratio=a["ratio_resized_over_levels_interpolate"], met=bool(a["ratio_resized_over_levels_interpolate"] < 1.0))
    line = json.dumps(result, indent=1)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
