#!/usr/bin/env python
"""The ragged decode (lrf_qmf_decode_ragged_rgb_u8) against the uniform decoder's batched routes, on random int8 factors.

  (a) mixed ranks   256 x 512x768, the 25 distinct rank triples of qualities 1..32 dealt round-robin.  Ragged: one call.
                    Grouped: the images grouped by triple, one lrf_qmf_decode_rgb_u8 per group, index_copy_ back into input order.
  (b) uniform       256 x 512x768 at (7,3,3): one ragged call against one lrf_qmf_decode_rgb_u8.
  (c) mixed sizes   128 x 512x768 + 128 x 768x512 at (7,3,3): one ragged call against two uniform calls.

Both sides are timed at the C ABI, with descriptors, rank arrays and output buffers made beforehand.  The routes of a case
alternate in one process; a run is `--calls` calls between two HIP events, the figure the median of `--runs` runs per call,
with the smallest and the largest run beside it.  Before timing, each case's ragged result is compared with the other route's
byte for byte.  Writes one JSON document to --out (default: stdout only)."""
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


def sizes_of(H, W, ranks):
    dims = _lib.plane_dims(H, W)
    return sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)


class Case:
    """images: [(H, W, ranks)] in input order"""

    def __init__(self, ctx, images, seed):
        self.ctx, self.lib, self.images = ctx, _lib.load(), images
        g = torch.Generator().manual_seed(seed)
        self.n = len(images)
        nu, nv = zip(*[sizes_of(*im) for im in images])
        self.U = torch.randint(-16, 16, (sum(nu),), dtype=torch.int8, generator=g).cuda()
        self.V = torch.randint(-16, 16, (sum(nv),), dtype=torch.int8, generator=g).cuda()
        self.desc = (_lib.RaggedImage * self.n)()
        uo = vo = ro = 0
        for d, (H, W, ranks), a, b in zip(self.desc, images, nu, nv):
            d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, uo, vo, ro
            d.R[0], d.R[1], d.R[2] = ranks
            uo, vo, ro = uo + a, vo + b, (ro + 3 * H * W + 15) // 16 * 16
        self.rgb = torch.empty((ro,), dtype=torch.uint8, device="cuda")
        # the grouped route: images of one (H, W, ranks) gathered into buffers of their own (done once, outside the timing: the
        # caller of the uniform decoder holds its factors that way), one call per group, results copied back into input order
        self.groups = []
        keys = []
        for im in images:
            if im not in keys:
                keys.append(im)
        for key in keys:
            idx = [i for i, im in enumerate(images) if im == key]
            a, b = sizes_of(*key)
            Ug = torch.stack([self.U[self.desc[i].u_off:self.desc[i].u_off + a] for i in idx]).contiguous()
            Vg = torch.stack([self.V[self.desc[i].v_off:self.desc[i].v_off + b] for i in idx]).contiguous()
            out = torch.empty((len(idx), 3, key[0], key[1]), dtype=torch.uint8, device="cuda")
            self.groups.append((key, torch.tensor(idx, device="cuda"), Ug, Vg, out, (ctypes.c_int * 3)(*key[2])))
        self.same_size = len({im[:2] for im in images}) == 1
        if self.same_size:
            self.ordered = torch.empty((self.n, 3) + images[0][:2], dtype=torch.uint8, device="cuda")

    def ragged(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.lrf_qmf_decode_ragged_rgb_u8(self.ctx._h, self.n, self.desc, p(self.U), self.U.numel(), p(self.V), self.V.numel(),
                                                         p(self.rgb), self.rgb.numel()))

    def grouped(self):
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        for (H, W, _), idx, Ug, Vg, out, R in self.groups:
            _lib.check(self.lib.lrf_qmf_decode_rgb_u8(self.ctx._h, p(Ug), p(Vg), Ug.shape[0], H, W, R, p(out)))
            if self.same_size and len(self.groups) > 1:
                self.ordered.index_copy_(0, idx, out)

    def verify(self):
        self.ragged()
        self.grouped()
        torch.cuda.synchronize()
        for (H, W, _), idx, _, _, out, _ in self.groups:
            for j, i in enumerate(idx.tolist()):
                d = self.desc[i]
                if not torch.equal(self.rgb[d.rgb_off:d.rgb_off + 3 * H * W].view(3, H, W), out[j]):
                    raise SystemExit(f"image {i}: the ragged decode differs from the uniform decoder")


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
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of liblrf_hip.so to measure (default: the package's)")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
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
        "b_uniform": [(512, 768, (7, 3, 3))] * B,
        "c_mixed_sizes": [(512, 768, (7, 3, 3))] * (B // 2) + [(768, 512, (7, 3, 3))] * (B // 2),
    }
    other = {"a_mixed_ranks": "grouped_by_triple", "b_uniform": "uniform_call", "c_mixed_sizes": "two_uniform_calls"}
    result = dict(tool="tools/bench_decode_ragged.py", lib=os.path.basename(_lib.LIB_PATH), device=torch.cuda.get_device_name(0), batch=B, runs=args.runs, calls_per_run=args.calls,
                  distinct_triples=len(triples), cases={})
    for name, images in cases.items():
        c = Case(ctx, images, seed=len(name))
        c.verify()
        r = time_routes({"ragged": c.ragged, other[name]: c.grouped}, args.runs, args.calls, args.warmup)
        r["launch_groups"] = len(c.groups)
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
