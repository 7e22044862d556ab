"""Device metrics (lrf_image_metrics_u8): what the kernels cost and what the R-D sweep gains.
  python tools/bench_metrics.py kernel [B H W]      one warmed call per size (default 256 x 512x768 and 512 x 1365x2048, C = 3), HIP-event
                                                    time of the call and effective read bandwidth 2 B C H W / t; run it under
                                                    `rocprofv3 --kernel-trace --stats` for the per-kernel times
  python tools/bench_metrics.py sweep [out.json]    BASELINE config 3 (24 x 512x768, qualities 1..32) through rd_sweep_batched with
                                                    metrics="host" and metrics="device": wall time and the metrics stage of each"""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import lrf_amd
from lrf_amd import _lib


def kernel_leg(B, H, W, reps=5):
    g = torch.Generator().manual_seed(1)
    one = torch.randint(0, 256, (8, 3, H, W), dtype=torch.uint8, generator=g)
    a = one.repeat((B + 7) // 8, 1, 1, 1)[:B].cuda()
    b = (a.to(torch.int16) + torch.randint(-9, 10, (1, 3, H, W), generator=g).to(torch.int16).cuda()).clamp(0, 255).to(torch.uint8)
    ctx = _lib.context(0)
    out = {}
    for want_ssim in (True, False):
        for _ in range(2):
            ctx.image_metrics(a, b, want_ssim)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.image_metrics(a, b, want_ssim)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = sorted(ts)[len(ts) // 2]
        out["sse+ssim" if want_ssim else "sse only"] = {"ms": round(ms, 4), "all_ms": [round(t, 4) for t in ts],
                                                        "read_TB_s_of_2BCHW": round(2 * a.numel() / (ms * 1e-3) / 1e12, 3)}
    return {"B": B, "H": H, "W": W, "bytes_2BCHW": 2 * a.numel(), **out}


def sweep_leg(path):
    from conftest import config3_image
    imgs = torch.stack([config3_image(i) for i in range(24)])
    qualities = list(range(1, 33))
    lrf_amd.rd_sweep_batched(imgs[:2], qualities[:2], metrics="device")  # warm-up: code objects, workspaces
    lrf_amd.rd_sweep_batched(imgs, qualities[:1], metrics="device")
    res = {"workload": "24 x 512x768 (BASELINE config 3 stand-ins), qualities 1..32: rd_sweep_batched, fused encode"}
    for mode in ("device", "host", "device", "device"):  # (the host sweep once: it takes minutes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = lrf_amd.rd_sweep_batched(imgs, qualities, metrics=mode)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        r = res.setdefault(mode, {"wall_s": [], "metrics_s": []})
        r["wall_s"].append(round(wall, 4))
        if mode == "device":
            r["metrics_s"].append(round(sum(x["metrics time (ms)"] for x in recs) / 1e3, 5))
        else:  # what the sweep spends outside its timed encode and decode calls: D2H bookkeeping aside, psnr + ssim per image
            r["metrics_s"].append(round(wall - sum(x["encoding time (ms)"] + x["decoding time (ms)"] for x in recs) / 1e3, 4))
        r["records"] = len(recs)
        print(f"# {mode}: wall {wall:.3f} s, metrics stage {r['metrics_s'][-1]:.4f} s", file=sys.stderr, flush=True)
    for mode in ("host", "device"):
        r = res[mode]
        r["metrics_share_of_wall"] = round(min(r["metrics_s"]) / min(r["wall_s"]), 4)
    res["host_over_device_metrics_stage"] = round(min(res["host"]["metrics_s"]) / min(res["device"]["metrics_s"]), 1)
    res["host_over_device_wall"] = round(min(res["host"]["wall_s"]) / min(res["device"]["wall_s"]), 2)
    print(json.dumps(res, indent=1))
    if path:
        json.dump(res, open(path, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "sweep":
        sweep_leg(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        sizes = [tuple(int(v) for v in sys.argv[2:5])] if len(sys.argv) >= 5 else [(256, 512, 768), (512, 1365, 2048)]
        for B, H, W in sizes:
            print(json.dumps(kernel_leg(B, H, W)), flush=True)
