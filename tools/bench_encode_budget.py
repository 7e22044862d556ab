#!/usr/bin/env python
"""Encoding to a byte budget: what counting the stream sizes on the GPU costs, and what qmf_encode_budget saves.

  (a) lrf_deflate_sizes_i8 against lrf_deflate_columns_i8 on the SAME tables (the U matrices and the V matrices of a batch's
      factors, one launch each), HIP-event time, the two alternated in one process, median of --runs:
        a1  256 x 512x768 at ranks (7,3,3)
        a2   24 x 512x768 at the rank triples of qualities 1..32
        a3  256 x 512x768 at the rank triples of qualities 1..32
      `bar`: counting is faster than writing on every table (a margin of zero).
  (b) qmf_encode_budget over qualities 1..32 against the brute force from the public functions that do not know it —
      qmf_encode_batch(deflate="device") per quality, qmf_decode_batch + psnr_batch, then the pick on the host — wall time
      (time.perf_counter around the call, the device idle before it), alternated, median of --wall-runs:
        b1   24 x 512x768        b2  256 x 512x768
      The budget is the median of the size table of a first call.

Images: the config-3 stand-in set (twenty smooth synthetic images and four crops of the natural fixture image), repeated.
Writes one JSON document to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import lrf_amd  # noqa: E402
from lrf_amd import _lib  # noqa: E402
from lrf_amd.codec import target_candidates  # noqa: E402

QUALITIES = list(range(1, 33))


def images(n):
    from conftest import config3_image
    base = torch.stack([config3_image(i) for i in range(24)])
    return base[torch.arange(n) % 24].contiguous().cuda()


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def tables(pairs, triples, hw):
    """(flat U, its table, flat V, its table) over all matrices of a sweep's factors, in deflate_table's layout"""
    Ms = [d[4] for d in _lib.plane_dims(*hw)]
    B = pairs[0][0].shape[0]
    mu, mv, uo, vo = [], [], 0, 0
    for t in triples:
        for _ in range(B):
            for M, R in zip(Ms, t):
                mu.append((uo, M, R))
                mv.append((vo, 64, R))
                uo, vo = uo + M * R, vo + 64 * R
    return _lib.flat_views([p[0] for p in pairs]), _lib.deflate_table(mu), _lib.flat_views([p[1] for p in pairs]), _lib.deflate_table(mv)


def count_against_write(dev, triples, runs):
    ctx = _lib.context()
    hw = tuple(dev.shape[-2:])
    pairs = ctx.encode_sweep_rgb(dev, triples, 10, -16, 15) if len(triples) > 1 else [lrf_amd.qmf_factorize_batch(dev, list(triples[0]))]
    U, (tu, nbu, ncu), V, (tv, nbv, ncv) = tables(pairs, triples, hw)
    su, sv = (torch.empty((n,), dtype=torch.uint8, device="cuda") for n in (nbu, nbv))
    lu, lv, cu, cv = (torch.empty((n,), dtype=torch.int32, device="cuda") for n in (ncu, ncv, ncu, ncv))

    def count():
        ctx.deflate_sizes_into(U, tu, cu)
        ctx.deflate_sizes_into(V, tv, cv)

    def write():
        ctx.deflate_columns_into(U, tu, su, lu)
        ctx.deflate_columns_into(V, tv, sv, lv)
    ms = {"count": [], "write": []}
    for i in range(runs + 2):
        for name, fn in (("count", count), ("write", write)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms[name].append(a.elapsed_time(b))
    ctx.check()
    assert torch.equal(cu, lu) and torch.equal(cv, lv), "the count and the coder disagree"
    rec = {"images": int(dev.shape[0]), "size": list(hw), "triples": len(triples), "columns": ncu + ncv, "factor_bytes": U.numel() + V.numel(),
           "slot_bytes": nbu + nbv, "count": summary(ms["count"]), "write": summary(ms["write"])}
    rec["count_over_write"] = round(statistics.median(ms["count"]) / statistics.median(ms["write"]), 4)
    return rec


def brute_force(dev, budget):
    """the parent's public functions only: every quality packed, decoded and scored, then the pick per image on the host"""
    H, W = dev.shape[-2:]
    size, psnr, streams = [], [], []
    for q in QUALITIES:
        s = lrf_amd.qmf_encode_batch(dev, quality=q, deflate="device")
        streams.append(s)
        size.append([len(x) for x in s])
        psnr.append(lrf_amd.psnr_batch(dev, lrf_amd.qmf_decode_batch(s)).cpu().tolist())
    out = []
    for b in range(dev.shape[0]):
        fit = [i for i in range(len(QUALITIES)) if size[i][b] <= budget]
        i = min(fit, key=lambda i: (-psnr[i][b], size[i][b], i)) if fit else min(range(len(QUALITIES)), key=lambda i: (size[i][b], i))
        out.append(streams[i][b])
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def budget_against_brute_force(dev, runs, warmup):
    first = lrf_amd.qmf_encode_budget(dev, nbytes=0)
    budget = int(first["size_table"].flatten().median())
    ours, brute, a, b = [], [], None, None
    for i in range(warmup + runs):
        ta, a = wall(lambda: lrf_amd.qmf_encode_budget(dev, nbytes=budget))
        tb, b = wall(lambda: brute_force(dev, budget))
        if i >= warmup:
            ours.append(ta)
            brute.append(tb)
    assert a["streams"] == b, "qmf_encode_budget and the brute force disagree"
    return {"images": int(dev.shape[0]), "size": list(dev.shape[-2:]), "qualities": [QUALITIES[0], QUALITIES[-1]], "budget_bytes": budget,
            "chosen_qualities": sorted(set(a["quality"])), "reached": int(a["reached"].sum()), "qmf_encode_budget": summary(ours), "brute_force": summary(brute),
            "budget_over_brute_force": round(statistics.median(ours) / statistics.median(brute), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--wall-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="a1,a2,a3,b1,b2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_encode_budget.json"))
    args = ap.parse_args()
    sweep = target_candidates((512, 768), QUALITIES)[0]
    cases = {"a1": (256, [(7, 3, 3)]), "a2": (24, sweep), "a3": (256, sweep), "b1": (24, None), "b2": (256, None)}
    doc = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "wall_runs": args.wall_runs, "warmup": args.warmup,
           "columns_per_workgroup": _lib.LRF_DEFLATE_CG, "pack_threads": lrf_amd.codec.default_pack_threads(), "cases": {}}
    for key in args.cases.split(","):
        n, triples = cases[key]
        dev = images(n)
        rec = count_against_write(dev, triples, args.runs) if triples else budget_against_brute_force(dev, args.wall_runs, args.warmup)
        doc["cases"][key] = rec
        print(key, json.dumps(rec), flush=True)
        del dev
        torch.cuda.empty_cache()
    counted = {k: r["count_over_write"] for k, r in doc["cases"].items() if "count_over_write" in r}
    if counted:
        doc["bar"] = {"count_over_write": counted, "below": 1.0, "met": all(v < 1.0 for v in counted.values())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("bar", {})))


if __name__ == "__main__":
    main()
