#!/usr/bin/env python
"""The gray loader (lrf_qmf_decode_gray_crops_u8, lrf_qmf_decode_gray_resized_crops_u8 / _tensor, lrf_qmf_decode_gray_ragged_u8)
against what a caller of gray streams had before it: lrf_qmf_decode_gray_u8 of batches of one size and rank, and torch ops on the
decoded bytes.  Random int8 factors (u, v uniform in [-6, 6), column 0 set to 8 / 15: mid-gray images that reach both clamps),
256 gray images of 512x768 at rank 7 and at rank 26.

  (a) crops      one 224x224 window per image at a random origin.  new: lrf_qmf_decode_gray_crops_u8.  old: the full decode of
                 the batch, then slice-and-stack into a preallocated [n,1,224,224] (torch.stack(out=)).  full: that decode alone.
  (b) resized    one box per image drawn as torchvision's RandomResizedCrop draws it, resampled to 224x224.  new: the _u8 entry
                 and the _tensor entry (float16, mean 0.449, std 0.226).  old: the full decode, avg_pool2d (ceil_mode) for every
                 level the boxes use, F.interpolate(bilinear) per crop into a preallocated float batch, then clamp-and-convert to
                 uint8, or (float16) the to-tensor chain mul_ / add_ / copy_.  The old route's pixels are torch's, not the
                 entry's definition: the largest difference of the uint8 results is recorded, and the new _tensor result is
                 compared bitwise with the torch chain on the new _u8 result.
  (c) ragged     256 images of 32 sizes around 512x768 (8 of each).  new: one lrf_qmf_decode_gray_ragged_u8.  old: one
                 lrf_qmf_decode_gray_u8 per size.  uniform: 256 x 512x768 through the ragged entry against the uniform decoder
                 itself (a few percent slower is expected there: the item table and the window arithmetic; reported, not barred).

The decodes run at the C ABI.  Routes are alternated in one process; a run is `--calls` calls between two HIP events, the figure
the median of `--runs` runs per call with the smallest and the largest beside it.  Bytes are compared before timing wherever two
routes define the same bytes ((a), (c)): a difference ends the run with an error.  The bar (bar.met): in (a), (b) and (c, mixed)
the new call's median is below the old route's smallest run, at both ranks.  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_decode_resized import SIZE, level_of, random_resized_crop_box  # noqa: E402
from lrf_amd import _lib  # noqa: E402

MEAN, STD = 0.449, 0.226
N, H0, W0 = 256, 512, 768
RANKS = (7, 26)
MIXED_SIZES = [(512 - 64 + 16 * (k % 8) + k % 3, 768 - 96 + 24 * (k // 8) + k % 5) for k in range(32)]
p = lambda t: ctypes.c_void_p(t.data_ptr())


def factors(sizes, R, seed):
    """flat int8 (U, V) of the images of `sizes` back to back and their (H, W, R, u_off, v_off)"""
    rng = np.random.default_rng(seed)
    images, us, vs, uo, vo = [], [], [], 0, 0
    for Hh, Ww in sizes:
        M = _lib.chan_dims(Hh, Ww, 1, (8, 8))[2]
        u, v = rng.integers(-6, 6, (M, R), dtype=np.int8), rng.integers(-6, 6, (64, R), dtype=np.int8)
        u[:, 0], v[:, 0] = 8, 15
        images.append((Hh, Ww, R, uo, vo))
        us.append(u.reshape(-1))
        vs.append(v.reshape(-1))
        uo, vo = uo + u.size, vo + v.size
    return images, torch.from_numpy(np.concatenate(us)).cuda(), torch.from_numpy(np.concatenate(vs)).cuda()


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


class Uniform:
    """256 x 512x768 at rank R: sections (a), (b) and the uniform half of (c)"""

    def __init__(self, ctx, R, seed):
        self.ctx, self.lib, self.R = ctx, _lib.load(), R
        self.images, self.U, self.V = factors([(H0, W0)] * N, R, seed)
        self.desc = _lib._gray_images(self.images)
        self.full = torch.empty((N, H0, W0), dtype=torch.uint8, device="cuda")
        rng = np.random.default_rng(seed + 1)
        self.origins = [(int(rng.integers(0, H0 - SIZE[0] + 1)), int(rng.integers(0, W0 - SIZE[1] + 1))) for _ in range(N)]
        self.crops = np.ascontiguousarray([(i, 1, y, x) for i, (y, x) in enumerate(self.origins)], dtype=np.int32)
        self.boxes = [random_resized_crop_box(rng, H0, W0) for _ in range(N)]
        self.levels = [level_of(b[2], b[3]) for b in self.boxes]
        self.rboxes = np.ascontiguousarray([(i, *b, int(rng.integers(0, 2))) for i, b in enumerate(self.boxes)], dtype=np.int32)
        self.new_u8 = torch.empty((N, 1) + SIZE, dtype=torch.uint8, device="cuda")
        self.old_u8 = torch.empty_like(self.new_u8)
        self.f32 = torch.empty((N, 1) + SIZE, dtype=torch.float32, device="cuda")
        self.new_f16 = torch.empty((N, 1) + SIZE, dtype=torch.float16, device="cuda")
        self.old_f16 = torch.empty_like(self.new_f16)
        self.fmt = _lib.check_tensor_format(torch.float16, MEAN, STD)
        self.ragged_out = torch.empty((N * H0 * W0,), dtype=torch.uint8, device="cuda")
        self.ragged_desc = _lib._gray_images(self.images, [i * H0 * W0 for i in range(N)])

    def _lead(self):
        return (self.ctx._h, N, self.desc, p(self.U), self.U.numel(), p(self.V), self.V.numel(), N)

    def full_decode(self):
        _lib.check(self.lib.lrf_qmf_decode_gray_u8(self.ctx._h, p(self.U), p(self.V), N, H0, W0, self.R, p(self.full)))

    # (a)
    def crops_new(self):
        _lib.check(self.lib.lrf_qmf_decode_gray_crops_u8(*self._lead(), self.crops.ctypes.data_as(ctypes.POINTER(_lib.ScaledCrop)), SIZE[0], SIZE[1],
                                                         p(self.new_u8), self.new_u8.numel()))

    def crops_old(self):
        self.full_decode()
        torch.stack([self.full[i, y:y + SIZE[0], x:x + SIZE[1]] for i, (y, x) in enumerate(self.origins)], out=self.old_u8[:, 0])

    # (b)
    def resized_new(self):
        _lib.check(self.lib.lrf_qmf_decode_gray_resized_crops_u8(*self._lead(), self.rboxes.ctypes.data_as(ctypes.POINTER(_lib.ResizedCrop)), SIZE[0], SIZE[1],
                                                                 p(self.new_u8), self.new_u8.numel()))

    def resized_new_f16(self):
        _lib.check(self.lib.lrf_qmf_decode_gray_resized_crops_tensor(*self._lead(), self.rboxes.ctypes.data_as(ctypes.POINTER(_lib.ResizedCrop)), SIZE[0], SIZE[1],
                                                                     ctypes.byref(self.fmt), p(self.new_f16), self.new_f16.numel() * 2))

    def _resized_old_f32(self):
        self.full_decode()
        x = self.full[:, None].float()
        lvl = {1: x}
        for f in sorted(set(self.levels) - {1}):
            lvl[f] = F.avg_pool2d(x, f, ceil_mode=True)
        for i, ((y0, x0, hb, wb), f, flip) in enumerate(zip(self.boxes, self.levels, self.rboxes[:, 5].tolist())):
            src = lvl[f][i:i + 1, :, y0 // f:max(y0 // f + 1, (y0 + hb) // f), x0 // f:max(x0 // f + 1, (x0 + wb) // f)]
            r = F.interpolate(src, size=SIZE, mode="bilinear", align_corners=False)
            self.f32[i:i + 1] = r.flip(-1) if flip else r

    def resized_old(self):
        self._resized_old_f32()
        self.old_u8.copy_(self.f32.add_(0.5).clamp_(0, 255))

    def resized_old_f16(self):
        self._resized_old_f32()
        self.old_f16.copy_(self.f32.round_().clamp_(0, 255).mul_(self.fmt.scale[0]).add_(self.fmt.bias[0]))

    # (c), uniform
    def ragged(self):
        _lib.check(self.lib.lrf_qmf_decode_gray_ragged_u8(self.ctx._h, N, self.ragged_desc, 1, p(self.U), self.U.numel(), p(self.V), self.V.numel(),
                                                          p(self.ragged_out), self.ragged_out.numel()))


class Mixed:
    """256 images of 32 sizes (8 consecutive images each) at rank R: the mixed half of (c)"""

    def __init__(self, ctx, R, seed):
        self.ctx, self.lib, self.R = ctx, _lib.load(), R
        sizes = [s for s in MIXED_SIZES for _ in range(8)]
        self.images, self.U, self.V = factors(sizes, R, seed)
        offs, off = [], 0
        for Hh, Ww in sizes:
            offs.append(off)
            off += Hh * Ww
        self.offs = offs
        self.desc = _lib._gray_images(self.images, offs)
        self.new, self.old = torch.empty((off,), dtype=torch.uint8, device="cuda"), torch.empty((off,), dtype=torch.uint8, device="cuda")

    def ragged(self):
        _lib.check(self.lib.lrf_qmf_decode_gray_ragged_u8(self.ctx._h, len(self.images), self.desc, 1, p(self.U), self.U.numel(), p(self.V), self.V.numel(),
                                                          p(self.new), self.new.numel()))

    def per_size(self):
        for k in range(0, len(self.images), 8):
            Hh, Ww, R, uo, vo = self.images[k]
            _lib.check(self.lib.lrf_qmf_decode_gray_u8(self.ctx._h, ctypes.c_void_p(self.U.data_ptr() + uo), ctypes.c_void_p(self.V.data_ptr() + vo), 8, Hh, Ww, R,
                                                       ctypes.c_void_p(self.old.data_ptr() + self.offs[k])))


def same(a, b, what):
    torch.cuda.synchronize()
    if not torch.equal(a, b):
        sys.exit(f"{what}: the two routes differ on {int((a != b).sum())} bytes: not timed")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r23_gray_loader.json"))
    args = ap.parse_args()
    if args.runs < 7 or args.calls < 5:
        ap.error("at least 7 runs of at least 5 calls")
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = _lib.context(0)
    ctx.use_torch_stream()
    result = dict(tool="tools/bench_gray_loader.py", device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_run=args.calls, images=N,
                  size=[H0, W0], output=list(SIZE), mean=MEAN, std=STD, ranks={})
    t = lambda routes: time_routes(routes, args.runs, args.calls, args.warmup)
    below = lambda r, new, old: bool(r[new]["median_ms"] < r[old]["min_ms"])
    met = {}
    for R in RANKS:
        c = Uniform(ctx, R, seed=100 + R)
        out = {}
        c.crops_new(); c.crops_old()
        same(c.new_u8, c.old_u8, f"(a) rank {R}")
        out["a_crops"] = r = t({"new": c.crops_new, "old_decode_slice_stack": c.crops_old, "full_decode": c.full_decode})
        r["bitwise_equal"], r["ratio_new_over_old"], r["ratio_new_over_full_decode"] = True, r["new"]["median_ms"] / r["old_decode_slice_stack"]["median_ms"], \
            r["new"]["median_ms"] / r["full_decode"]["median_ms"]
        met[f"a_r{R}"] = below(r, "new", "old_decode_slice_stack")
        c.resized_new(); c.resized_old()
        torch.cuda.synchronize()
        diff = int((c.new_u8.int() - c.old_u8.int()).abs().max())
        c.resized_new_f16()
        chain = c.new_u8.float().mul(c.fmt.scale[0]).add(c.fmt.bias[0]).to(torch.float16)
        same(c.new_f16.view(torch.int16), chain.view(torch.int16), f"(b) rank {R}, the tensor form against the torch chain on the u8 form")
        out["b_resized_u8"] = r = t({"new": c.resized_new, "old_decode_pool_interpolate": c.resized_old})
        r["largest_difference_from_the_torch_route"], r["ratio_new_over_old"] = diff, r["new"]["median_ms"] / r["old_decode_pool_interpolate"]["median_ms"]
        r["boxes_per_level"] = {str(f): c.levels.count(f) for f in sorted(set(c.levels))}
        met[f"b_u8_r{R}"] = below(r, "new", "old_decode_pool_interpolate")
        out["b_resized_f16"] = r = t({"new": c.resized_new_f16, "old_decode_pool_interpolate_chain": c.resized_old_f16})
        r["tensor_bitwise_equal_to_chain_on_u8"], r["ratio_new_over_old"] = True, r["new"]["median_ms"] / r["old_decode_pool_interpolate_chain"]["median_ms"]
        met[f"b_f16_r{R}"] = below(r, "new", "old_decode_pool_interpolate_chain")
        c.ragged(); c.full_decode()
        same(c.ragged_out, c.full.view(-1), f"(c) uniform, rank {R}")
        out["c_ragged_uniform"] = r = t({"ragged": c.ragged, "uniform_decoder": c.full_decode})
        r["bitwise_equal"], r["ratio_ragged_over_uniform"] = True, r["ragged"]["median_ms"] / r["uniform_decoder"]["median_ms"]
        del c
        m = Mixed(ctx, R, seed=200 + R)
        m.ragged(); m.per_size()
        same(m.new, m.old, f"(c) mixed, rank {R}")
        out["c_ragged_mixed"] = r = t({"new": m.ragged, "old_one_call_per_size": m.per_size})
        r["bitwise_equal"], r["ratio_new_over_old"], r["sizes"] = True, r["new"]["median_ms"] / r["old_one_call_per_size"]["median_ms"], len(MIXED_SIZES)
        met[f"c_mixed_r{R}"] = below(r, "new", "old_one_call_per_size")
        del m
        result["ranks"][str(R)] = out
        print(R, json.dumps(out), flush=True)
        ctx.trim()
        torch.cuda.empty_cache()
    result["bar"] = dict(what="in (a), (b) and (c, mixed) the new call's median is below the old route's smallest run, at both ranks", parts=met,
                         met=bool(all(met.values())))
    line = json.dumps(result, indent=1)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
