#!/usr/bin/env python
"""The ragged encode (lrf_qmf_encode_ragged_rgb_u8) against the uniform encoder's bucketed routes, at K = 10, bounds (-16, 15).

  (a) mixed ranks   256 x 512x768, the 25 distinct rank triples of qualities 1..32 dealt round-robin.  Ragged: one call.
                    Bucketed: the images gathered by triple, one lrf_qmf_encode_rgb_u8 per triple.
  (b) mixed sizes   128 x 512x768 + 128 x 768x512 at (7,3,3): one ragged call against two uniform calls.
  (c) uniform       256 x 512x768 at (7,3,3): one ragged call against lrf_qmf_encode_rgb_u8 itself.
  (d) small mixed   24 images of six sizes (four each) at (7,3,3): one ragged call against six uniform calls.

Both sides are timed at the C ABI on the same pixels, with descriptors, rank arrays, buckets and output buffers made beforehand.
Before timing, each case's ragged factors are compared with the other route's byte for byte.  The routes of a case alternate in
one process; a run is `--calls` calls between two HIP events, the figure the median of `--runs` runs per call, with the smallest
and the largest run beside it.  Writes one JSON document to --out (default: stdout only)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

import lrf_amd  # noqa: E402
from lrf_amd import _lib  # noqa: E402

K, LO, HI = 10, -16, 15
SIX_SIZES = [(512, 768), (768, 512), (384, 512), (480, 640), (341, 512), (173, 264)]


def sizes_of(H, W, ranks):
    dims = _lib.plane_dims(H, W)
    return sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)


class Case:
    """images: [(H, W, ranks)] in input order"""

    def __init__(self, ctx, images, seed):
        self.ctx, self.lib, self.images = ctx, _lib.load(), images
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.n = len(images)
        nu, nv = zip(*[sizes_of(*im) for im in images])
        self.desc = (_lib.RaggedEncodeImage * self.n)()
        uo = vo = ro = 0
        for d, (H, W, ranks), a, b in zip(self.desc, images, nu, nv):
            d.H, d.W, d.rgb_off, d.u_off, d.v_off, d.sign_off = H, W, ro, uo, vo, -1
            d.R[0], d.R[1], d.R[2] = ranks
            uo, vo, ro = uo + a, vo + b, (ro + 3 * H * W + 15) // 16 * 16
        self.rgb = torch.randint(0, 256, (ro,), dtype=torch.uint8, device="cuda", generator=g)
        self.U = torch.empty((uo,), dtype=torch.int8, device="cuda")
        self.V = torch.empty((vo,), dtype=torch.int8, device="cuda")
        # the bucketed route: the images of one (H, W, ranks) gathered into a batch of their own (once, outside the timing: that is how
        # the caller of the uniform encoder holds them), one call per bucket
        self.groups = []
        keys = []
        for im in images:
            if im not in keys:
                keys.append(im)
        for key in keys:
            idx = [i for i, im in enumerate(images) if im == key]
            H, W, ranks = key
            a, b = sizes_of(*key)
            batch = torch.stack([self.rgb[self.desc[i].rgb_off:self.desc[i].rgb_off + 3 * H * W].view(3, H, W) for i in idx]).contiguous()
            self.groups.append((key, idx, batch, torch.empty((len(idx), a), dtype=torch.int8, device="cuda"),
                                torch.empty((len(idx), b), dtype=torch.int8, device="cuda"), (ctypes.c_int * 3)(*ranks)))

    def ragged(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.lrf_qmf_encode_ragged_rgb_u8(self.ctx._h, self.n, self.desc, p(self.rgb), self.rgb.numel(), K, LO, HI, None, 0,
                                                         p(self.U), self.U.numel(), p(self.V), self.V.numel()))

    def bucketed(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        for (H, W, _), idx, batch, Ug, Vg, R in self.groups:
            _lib.check(self.lib.lrf_qmf_encode_rgb_u8(self.ctx._h, p(batch), len(idx), H, W, R, K, LO, HI, None, p(Ug), p(Vg)))

    def verify(self):
        self.ragged()
        self.bucketed()
        torch.cuda.synchronize()
        self.ctx.check()
        for key, idx, _, Ug, Vg, _ in self.groups:
            a, b = sizes_of(*key)
            for j, i in enumerate(idx):
                d = self.desc[i]
                if not (torch.equal(self.U[d.u_off:d.u_off + a], Ug[j]) and torch.equal(self.V[d.v_off:d.v_off + b], Vg[j])):
                    raise SystemExit(f"image {i} {key}: the ragged encode differs from the uniform encoder")


def time_routes(routes, runs, calls, warmup):
    """routes: {name: callable}; -> {name: {median_ms, min_ms, max_ms}} per call, the routes alternating run by run"""
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 7:
        ap.error("--runs: at least 7")
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = _lib.context(0)
    ctx.use_torch_stream()
    B = args.batch
    triples = []
    for q in range(1, 33):
        t = tuple(lrf_amd.qmf_ranks((512, 768), quality=q))
        if t not in triples:
            triples.append(t)
    cases = {
        "a_mixed_ranks": [(512, 768, triples[i % len(triples)]) for i in range(B)],
        "b_mixed_sizes": [(512, 768, (7, 3, 3))] * (B // 2) + [(768, 512, (7, 3, 3))] * (B // 2),
        "c_uniform": [(512, 768, (7, 3, 3))] * B,
        "d_small_mixed": [SIX_SIZES[i % 6] + ((7, 3, 3),) for i in range(24)],
    }
    other = {"a_mixed_ranks": "one_call_per_triple", "b_mixed_sizes": "two_uniform_calls", "c_uniform": "uniform_call", "d_small_mixed": "six_uniform_calls"}
    result = dict(tool="tools/bench_encode_ragged.py", device=torch.cuda.get_device_name(0), batch=B, K=K, bounds=[LO, HI], runs=args.runs,
                  calls_per_run=args.calls, distinct_triples=len(triples), cases={})
    for name, images in cases.items():
        c = Case(ctx, images, seed=len(name))
        c.verify()
        r = time_routes({"ragged": c.ragged, other[name]: c.bucketed}, args.runs, args.calls, args.warmup)
        r["images"] = len(images)
        r["buckets"] = len(c.groups)
        r["mpixel"] = sum(H * W for H, W, _ in images) / 1e6
        r["ratio_ragged_over_other"] = r["ragged"]["median_ms"] / r[other[name]]["median_ms"]
        result["cases"][name] = r
        print(name, json.dumps(r), flush=True)
        del c
        ctx.trim()
        torch.cuda.empty_cache()
    line = json.dumps(result, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
