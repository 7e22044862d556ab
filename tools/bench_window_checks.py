#!/usr/bin/env python
"""What the host pays to check a crop list, alone: each of the five bodies behind the ten C entries that decode crops
(lrf_qmf_decode_crops_rgb_u8, _scaled_crops_, _resized_crops_, lrf_qmf_decode_gray_crops_u8, _gray_resized_crops_) is handed the
longest list it takes, 2^20 crops, whose last crop names an image that does not exist.  The call walks the whole list, refuses
(LRF_EINVAL) and launches nothing: its wall time is the prologue, the image table and check_windows (lrf_plan.cpp).  Two images,
24x48 and 45x61; windows of 8x8 (the scaled shapes: at scale 2), boxes of 11x13 resized to 8x8.  The output is allocated at its
full size all the same, so that a build that failed to refuse would still write inside it.

A run is `--calls` calls timed on the host; the figure is the median of `--runs` runs per call, the smallest and the largest
beside it.  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lrf_amd import _lib  # noqa: E402

N = 2 ** 20
SIZES = [(24, 48), (45, 61)]
# body: (the C entry, gray, crop type, one good row)
BODIES = {"crops": ("lrf_qmf_decode_crops_rgb_u8", False, _lib.Crop, (1, 3, 5)),
          "scaled_crops": ("lrf_qmf_decode_scaled_crops_rgb_u8", False, _lib.ScaledCrop, (1, 2, 3, 5)),
          "resized_crops": ("lrf_qmf_decode_resized_crops_rgb_u8", False, _lib.ResizedCrop, (1, 3, 5, 11, 13, 1)),
          "gray_crops": ("lrf_qmf_decode_gray_crops_u8", True, _lib.ScaledCrop, (1, 2, 3, 5)),
          "gray_resized_crops": ("lrf_qmf_decode_gray_resized_crops_u8", True, _lib.ResizedCrop, (1, 3, 5, 11, 13, 1))}


def images(gray):
    desc, uo, vo = ((_lib.GrayImage if gray else _lib.RaggedImage) * 2)(), 0, 0
    for d, (H, W) in zip(desc, SIZES):
        d.H, d.W, d.u_off, d.v_off = H, W, uo, vo
        if gray:
            d.R = 7
            uo, vo = uo + 7 * _lib.chan_dims(H, W, 1, (8, 8))[2], vo + 7 * 64
        else:
            d.R[0], d.R[1], d.R[2] = 7, 3, 3
            uo, vo = uo + sum(p[4] * r for p, r in zip(_lib.plane_dims(H, W), (7, 3, 3))), vo + 13 * 64
    return desc, torch.zeros(uo, dtype=torch.int8, device="cuda"), torch.zeros(vo, dtype=torch.int8, device="cuda")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", required=True, help="where the JSON document goes (profiles/r24_window_host_cost.json holds three of them beside the other benches' documents)")
    a = ap.parse_args()
    ctx, lib = _lib.context(0), _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    result = {"tool": "tools/bench_window_checks.py", "device": torch.cuda.get_device_name(0), "crops": N, "runs": a.runs, "calls_per_run": a.calls, "cases": {}}
    for body, (entry, gray, crop_type, row) in BODIES.items():
        desc, U, V = images(gray)
        rows = np.tile(np.array(row, dtype=np.int32), (N, 1))
        rows[N - 1, 0] = 2  # the last crop: no such image
        out = torch.empty(((1 if gray else 3) * 64 * N,), dtype=torch.uint8, device="cuda")
        call = lambda: getattr(lib, entry)(ctx._h, 2, desc, ptr(U), U.numel(), ptr(V), V.numel(), N, rows.ctypes.data_as(ctypes.POINTER(crop_type)), 8, 8,
                                           ptr(out), out.numel())
        ctx.use_torch_stream()
        assert call() == -1 and lib.lrf_last_error().decode() == f"crop {N - 1}: image 2 out of range [0,2)", lib.lrf_last_error().decode()
        for _ in range(a.warmup):
            call()
        per_call = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            per_call.append((time.perf_counter() - t0) * 1e3 / a.calls)
        r = {"refused_last_crop": {"median_ms": statistics.median(per_call), "min_ms": min(per_call), "max_ms": max(per_call)}}
        result["cases"][body] = r
        print(body, json.dumps(r), flush=True)
    line = json.dumps(result, indent=1)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
