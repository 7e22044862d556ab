#!/usr/bin/env python
"""inflate="device" against inflate="host": wall time from byte streams on the host to resident factors (qmf_load_factors) and to
pixels (qmf_decode_batch), both paths alternated in one process on the same streams.

  (a) 256 x 512x768 at ranks (7,3,3)      zlib-9 streams        (a_dev) the same images as deflate="device" streams
  (b) 256 x 512x768 at ranks (26,13,13)   zlib-9 streams        (b_dev) likewise
  (c) 64 x 1365x2048 at quality 7         zlib-9 streams

Images: the config-3 stand-in set (twenty smooth synthetic images and four crops of the natural fixture image), repeated; the
1365x2048 ones are those resized.  Per case: `--warmup` untimed rounds, then `--runs` rounds of (host call, device call) for each
of the two entry points; the figure is the median wall time (time.perf_counter around the call and a device synchronisation, the
device idle before it), with the smallest and the largest beside it.  Also: the HIP-event time of the inflate launch alone
(LRF_K_INFLATE of the context's timers, median over the device-path calls) and the bytes each path moves host to device (host:
the int8 factors; device: the compressed payloads; the column table of the launch is counted apart).  `bar`: case (a), device wall
time to resident factors <= host wall time, same run.  Writes one JSON document to --out."""
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
from lrf_amd.container import separate_bytes  # noqa: E402


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
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="a,a_dev,b,b_dev,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_inflate_device.json"))
    args = ap.parse_args()
    cases = {"a": (256, (512, 768), {"rank": [7, 3, 3]}, "host"), "a_dev": (256, (512, 768), {"rank": [7, 3, 3]}, "device"),
             "b": (256, (512, 768), {"rank": [26, 13, 13]}, "host"), "b_dev": (256, (512, 768), {"rank": [26, 13, 13]}, "device"),
             "c": (64, (1365, 2048), {"quality": 7}, "host")}
    ctx = _lib.context()
    doc = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "pack_threads": lrf_amd.codec.default_pack_threads(), "cases": {}}
    for key in args.cases.split(","):
        n, size, kw, deflate = cases[key]
        dev = images(n, size)
        streams = lrf_amd.qmf_encode_batch(dev, deflate=deflate, **kw)
        del dev
        torch.cuda.empty_cache()
        rec = {"images": n, "size": list(size), "params": kw, "streams": "zlib-9" if deflate == "host" else 'deflate="device"',
               "stream_bytes": sum(len(s) for s in streams)}
        launch = []
        for name, call in (("load_factors", lambda mode: lrf_amd.qmf_load_factors(streams, inflate=mode)),
                           ("decode_batch", lambda mode: lrf_amd.qmf_decode_batch(streams, inflate=mode))):
            host_ms, dev_ms = [], []
            for i in range(args.warmup + args.runs):
                th, out = wall(lambda: call("host"))
                del out
                ctx.profile_kernels([_lib.LRF_K_INFLATE])
                ctx.profile(True)
                ctx.profile_reset()
                td, out = wall(lambda: call("device"))
                ms, launches = ctx.kernel_time(_lib.LRF_K_INFLATE)
                ctx.profile(False)
                assert launches == 1
                if name == "load_factors" and i == 0:
                    rec["columns"] = 2 * sum(sum(im[2]) for im in out.images)
                    rec["h2d_bytes_host_path"] = out.U.numel() + out.V.numel()
                    rec["h2d_bytes_device_path"] = sum(len(separate_bytes(s, 2)[1]) for s in streams)
                    rec["h2d_bytes_column_table"] = 32 * rec["columns"]
                del out
                if i >= args.warmup:
                    host_ms.append(th)
                    dev_ms.append(td)
                    launch.append(ms)
            rec[name] = {"host": summary(host_ms), "device": summary(dev_ms),
                         "device_over_host": round(statistics.median(dev_ms) / statistics.median(host_ms), 4)}
        rec["inflate_launch_event"] = summary(launch)
        doc["cases"][key] = rec
        print(key, json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    if "a" in doc["cases"]:
        r = doc["cases"]["a"]["load_factors"]
        doc["bar"] = {"case": "a", "what": "wall time to resident factors, device path <= host path", "host_ms": r["host"]["median_ms"],
                      "device_ms": r["device"]["median_ms"], "met": r["device"]["median_ms"] <= r["host"]["median_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("bar", {})))


if __name__ == "__main__":
    main()
