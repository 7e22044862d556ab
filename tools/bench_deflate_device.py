#!/usr/bin/env python
"""deflate="device" against deflate="host": wall time from images in HBM to final byte streams, both paths alternated in one
process on the same images.

  (a) 256 x 512x768 at ranks (7,3,3)          qmf_encode_batch
  (b) 256 x 512x768 at ranks (26,13,13)       qmf_encode_batch
  (c) 64 x 1365x2048 at quality 7             qmf_encode_batch
  (d) 24 x 512x768, (e) 256 x 512x768         qmf_encode_target to 32 dB over qualities 1..32

Images: the config-3 stand-in set (twenty smooth synthetic images and four crops of the natural fixture image), repeated; the
1365x2048 ones are those resized.  Per case: `--warmup` untimed rounds, then `--runs` rounds of (host call, device call); the figure
is the median wall time (time.perf_counter around the call, the device idle before it), with the smallest and the largest beside
it.  For the batch cases also: the HIP-event time of the two lrf_deflate_columns_i8 launches alone on that batch's factors (median
of --runs), the bytes the device path brings to the host, and the total stream bytes of both paths.  `bar`: case (a), device wall
time / host wall time < 0.5.  Writes one JSON document to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lrf_amd  # noqa: E402
from lrf_amd import _lib  # noqa: E402
from lrf_amd.codec import qmf_factorize_batch, qmf_ranks  # noqa: E402


def images(n, size):
    from conftest import config3_image
    base = torch.stack([config3_image(i) for i in range(24)])
    if tuple(size) != (512, 768):
        base = torch.nn.functional.interpolate(base.float(), size=size, mode="bilinear", align_corners=False).round().clamp(0, 255).to(torch.uint8)
    return base[torch.arange(n) % 24].contiguous().cuda()


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def deflate_alone(dev, ranks, runs):
    """event time of the two deflate launches on the batch's factors, and the bytes the device path copies to the host"""
    ctx = _lib.context()
    H, W = dev.shape[-2:]
    U, V = qmf_factorize_batch(dev, ranks)
    B = U.shape[0]
    Ms = [d[4] for d in _lib.plane_dims(H, W)]
    mu, mv, uo, vo = [], [], 0, 0
    for b in range(B):
        for M, R in zip(Ms, ranks):
            mu.append((uo, M, R))
            mv.append((vo, 64, R))
            uo, vo = uo + M * R, vo + 64 * R
    tu, nbu, ncu = _lib.deflate_table(mu)
    tv, nbv, ncv = _lib.deflate_table(mv)
    su, lu = torch.empty((nbu,), dtype=torch.uint8, device="cuda"), torch.empty((ncu,), dtype=torch.int32, device="cuda")
    sv, lv = torch.empty((nbv,), dtype=torch.uint8, device="cuda"), torch.empty((ncv,), dtype=torch.int32, device="cuda")
    times = []
    for i in range(runs + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.deflate_columns_into(U.reshape(-1), tu, su, lu)
        ctx.deflate_columns_into(V.reshape(-1), tv, sv, lv)
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            times.append(a.elapsed_time(b))
    return summary(times), nbu + nbv + 4 * (ncu + ncv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_deflate_device.json"))
    args = ap.parse_args()
    cases = {"a": ("batch", 256, (512, 768), {"rank": [7, 3, 3]}), "b": ("batch", 256, (512, 768), {"rank": [26, 13, 13]}),
             "c": ("batch", 64, (1365, 2048), {"quality": 7}), "d": ("target", 24, (512, 768), {}), "e": ("target", 256, (512, 768), {})}
    doc = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "pack_threads": lrf_amd.codec.default_pack_threads(), "cases": {}}
    for key in args.cases.split(","):
        kind, n, size, kw = cases[key]
        dev = images(n, size)
        if kind == "batch":
            call = lambda mode: lrf_amd.qmf_encode_batch(dev, deflate=mode, **kw)
            streams_of = lambda out: out
        else:
            call = lambda mode: lrf_amd.qmf_encode_target(dev, 32.0, deflate=mode)
            streams_of = lambda out: out["streams"]
        host_ms, dev_ms, out_h, out_d = [], [], None, None
        for i in range(args.warmup + args.runs):
            th, out_h = wall(lambda: call("host"))
            td, out_d = wall(lambda: call("device"))
            if i >= args.warmup:
                host_ms.append(th)
                dev_ms.append(td)
        rec = {"kind": kind, "images": n, "size": list(size), "params": kw, "host": summary(host_ms), "device": summary(dev_ms),
               "device_over_host": round(statistics.median(dev_ms) / statistics.median(host_ms), 4),
               "stream_bytes_host": sum(len(s) for s in streams_of(out_h)), "stream_bytes_device": sum(len(s) for s in streams_of(out_d))}
        rec["stream_bytes_device_over_host"] = round(rec["stream_bytes_device"] / rec["stream_bytes_host"], 4)
        if kind == "batch":
            ranks = qmf_ranks(size, kw.get("rank"), kw.get("quality"))
            rec["ranks"] = [int(r) for r in ranks]
            rec["deflate_launches_event"], rec["bytes_to_host"] = deflate_alone(dev, ranks, args.runs)
        doc["cases"][key] = rec
        print(key, json.dumps(rec), flush=True)
        del dev
        torch.cuda.empty_cache()
    if "a" in doc["cases"]:
        doc["bar"] = {"case": "a", "device_over_host": doc["cases"]["a"]["device_over_host"], "below": 0.5,
                      "met": doc["cases"]["a"]["device_over_host"] < 0.5}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("bar", {})))


if __name__ == "__main__":
    main()
