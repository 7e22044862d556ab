"""Scoring a sweep straight from its factors (lrf_qmf_sweep_sse_rgb_u8) against the pair it replaces, and qmf_encode_target
against the brute force it replaces.
  python tools/bench_sweep_sse.py kernel [out.json]   256 x 512x768 at (7,3,3) and 24 x 512x768 over qualities 1..32: HIP-event time of
                                                      Context.sweep_sse and of decode_rgb + image_metrics(want_ssim=False) per triple on the
                                                      same factors, the two ALTERNATED in one process; bytes the new call reads per second
  python tools/bench_sweep_sse.py profile             the 24-image sweep scored ten times, nothing else: run it under
                                                      `rocprofv3 --kernel-trace --stats` for the per-kernel times
  python tools/bench_sweep_sse.py target [out.json]   qmf_encode_target on 24 and 256 images over qualities 1..32 against qmf_encode_sweep ->
                                                      qmf_decode_batch -> psnr_batch per quality: wall time of both, and what the packing
                                                      (zlib-9) takes of each"""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import lrf_amd
from lrf_amd import _lib, codec


def _images(B):
    from conftest import config3_image
    base = torch.stack([config3_image(i) for i in range(24)])
    return base.repeat((B + 23) // 24, 1, 1, 1)[:B].contiguous()


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_case(B, triples, reps=7):
    ctx = _lib.context(0)
    dev = _images(B).cuda()
    H, W = dev.shape[-2:]
    factors = ctx.encode_sweep_rgb(dev, triples, 10, -16, 15)

    def fused():
        return ctx.sweep_sse(dev, factors, triples)

    def pair():
        return [ctx.image_metrics(dev, ctx.decode_rgb(U, V, H, W, list(t)), want_ssim=False)[0] for (U, V), t in zip(factors, triples)]
    assert torch.equal(fused(), torch.stack(pair()))
    for _ in range(2):
        fused(), pair()
    torch.cuda.synchronize()
    tf, tp = [], []
    for _ in range(reps):  # alternated: both see the same clocks and the same neighbours
        tf.append(_timed(fused))
        tp.append(_timed(pair))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    read = len(triples) * dev.numel() + sum(U.numel() + V.numel() for U, V in factors)  # source per triple + the factors
    return {"B": B, "H": H, "W": W, "triples": len(triples), "sweep_sse_ms": round(med(tf), 4), "decode_plus_metrics_ms": round(med(tp), 4),
            "sweep_sse_all_ms": [round(t, 4) for t in tf], "decode_plus_metrics_all_ms": [round(t, 4) for t in tp],
            "pair_over_sweep_sse": round(med(tp) / med(tf), 3), "bytes_read": read, "sweep_sse_TB_s": round(read / (med(tf) * 1e-3) / 1e12, 3)}


def sweep_triples():
    return codec.target_candidates((512, 768), range(1, 33))[0]


def target_case(B, reps=3):
    images = _images(B)
    qualities = list(range(1, 33))
    out = {"B": B, "qualities": "1..32", "target_s": [], "brute_s": [], "target_pack_s": [], "brute_pack_s": []}
    pack_t = [0.0]
    real_pack = codec.pack_streams_native

    def timed_pack(*a, **k):
        t0 = time.perf_counter()
        r = real_pack(*a, **k)
        pack_t[0] += time.perf_counter() - t0
        return r
    codec.pack_streams_native = timed_pack
    try:
        lrf_amd.qmf_encode_target(images[:2], 30.0)  # warm-up: code objects, workspaces
        for _ in range(reps):
            torch.cuda.synchronize()
            pack_t[0] = 0.0
            t0 = time.perf_counter()
            res = lrf_amd.qmf_encode_target(images, 32.0)
            out["target_s"].append(round(time.perf_counter() - t0, 4))
            out["target_pack_s"].append(round(pack_t[0], 4))
            pack_t[0] = 0.0
            t0 = time.perf_counter()
            sweep = lrf_amd.qmf_encode_sweep(images, qualities=qualities)
            table = torch.stack([lrf_amd.psnr_batch(images, lrf_amd.qmf_decode_batch(s)) for s in sweep]).cpu()
            out["brute_s"].append(round(time.perf_counter() - t0, 4))
            out["brute_pack_s"].append(round(pack_t[0], 4))
            assert torch.equal(table, res["table"])
    finally:
        codec.pack_streams_native = real_pack
    out["chosen_qualities"] = sorted(set(res["quality"]))
    out["brute_over_target"] = round(min(out["brute_s"]) / min(out["target_s"]), 2)
    out["pack_share_of_target"] = round(min(out["target_pack_s"]) / min(out["target_s"]), 3)
    out["pack_share_of_brute"] = round(min(out["brute_pack_s"]) / min(out["brute_s"]), 3)
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    path = sys.argv[2] if len(sys.argv) > 2 else None
    if mode == "profile":
        ctx = _lib.context(0)
        dev = _images(24).cuda()
        triples = sweep_triples()
        factors = ctx.encode_sweep_rgb(dev, triples, 10, -16, 15)
        for _ in range(10):
            ctx.sweep_sse(dev, factors, triples)
        torch.cuda.synchronize()
        sys.exit(0)
    res = [kernel_case(256, [(7, 3, 3)]), kernel_case(24, sweep_triples())] if mode == "kernel" else [target_case(24), target_case(256)]
    for r in res:
        print(json.dumps(r), flush=True)
    if path:
        json.dump(res, open(path, "w"), indent=1)
