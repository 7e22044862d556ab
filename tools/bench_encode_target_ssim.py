#!/usr/bin/env python
"""Encode to a target SSIM: what the scoring from the factors costs, against the route that existed before it.

  (a) lrf_qmf_ssim_ragged_rgb_u8 (Context.ssim_ragged) on the factors of 256 x 512x768 at the rank triples of qualities 1..32
      and (b) on 256 images of 32 sizes, against decode_ragged of ALL candidates into one buffer followed by image_metrics once
      per size group.  `bar`: not slower than that route, with peak extra memory at most the cap (the scratch buffer is read back
      from the context's workspace; the other route's buffer is Q x B decoded images).
  (c) image_metrics_ragged's entry (Context.metrics_ragged) on 256 equal-size pairs against image_metrics: the ratio only.
  (d) qmf_encode_target(images, ssim=0.95) on the 256 mixed images end to end, and its stages timed on their own: the sweep
      encode, the scoring, the selection, the packing of the winners.

Every pair is checked for equal results first, alternated in one process, timed with HIP events around the call (the stream idle
before it), median of --runs.  Writes one JSON document to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_encode_target_ragged import QUALITIES, alternate, mixed_images, summary, wall  # noqa: E402


def sweep_of(images):
    """the ragged sweep encode of every (image, candidate triple) -> (ctx, flat sources, items [m, 8], U, V, row [Q, n])"""
    import numpy as np
    import torch
    from lrf_amd import _lib
    from lrf_amd.codec import qmf_ranks, target_candidates
    ctx = _lib.context()
    sizes = [tuple(im.shape[1:]) for im in images]
    n = len(images)
    offs, off = [], 0
    for H, W in sizes:
        offs.append(off)
        off = (off + 3 * H * W + 15) // 16 * 16
    flat = torch.empty((off,), dtype=torch.uint8, device="cuda")
    for im, o in zip(images, offs):
        flat[o:o + im.numel()].view(im.shape).copy_(im)
    per = [target_candidates(hw, QUALITIES)[0] for hw in sizes]
    counts = np.array([len(t) for t in per], dtype=np.int64)
    owner = np.repeat(np.arange(n, dtype=np.int64), counts)
    ranks = np.array([t for ts in per for t in ts], dtype=np.int64)
    cands = np.concatenate([owner.reshape(-1, 1), ranks], axis=1)
    ims = [(H, W, o) for (H, W), o in zip(sizes, offs)]
    enc = lambda: ctx.encode_ragged_sweep(flat, ims, cands, 10, -16, 15)
    U, V, u_off, v_off = enc()
    hw = np.array(sizes, dtype=np.int64)[owner]
    items = np.concatenate([hw, ranks, np.asarray(u_off).reshape(-1, 1), np.asarray(v_off).reshape(-1, 1), np.asarray(offs)[owner].reshape(-1, 1)], axis=1)
    first = np.cumsum(counts) - counts
    row = first.reshape(1, n) + np.array([[ts.index(tuple(qmf_ranks(s_, None, q))) for q in QUALITIES] for ts, s_ in zip(per, sizes)]).T
    return ctx, flat, items, U, V, row, enc


def case_scoring(images, runs, warmup, cap):
    import numpy as np
    import torch
    ctx, flat, items, U, V, _, _ = sweep_of(images)
    m = items.shape[0]
    px = 3 * items[:, 0] * items[:, 1]
    dec_off = np.cumsum((px + 15) // 16 * 16) - (px + 15) // 16 * 16
    groups = {}
    for j in range(m):
        groups.setdefault((int(items[j, 0]), int(items[j, 1])), []).append(j)

    def parent_route():
        # every candidate decoded into one buffer, then the uniform metrics once per size group
        dec = ctx.decode_ragged(U, V, [(int(r[0]), int(r[1]), [int(r[2]), int(r[3]), int(r[4])], int(r[5]), int(r[6])) for r in items])
        sse = torch.empty((m,), dtype=torch.int64, device="cuda")
        ssim = torch.empty((m,), dtype=torch.float64, device="cuda")
        for (H, W), idx in groups.items():
            src = torch.stack([flat[int(items[j, 7]):int(items[j, 7]) + 3 * H * W].view(3, H, W) for j in idx])
            a, b = ctx.image_metrics(src, torch.stack([dec[j] for j in idx]))
            sel = torch.tensor(idx, device="cuda")
            sse[sel], ssim[sel] = a, b
        return sse, ssim
    ctx.trim()
    base = ctx.workspace_bytes()
    ctx.ssim_ragged(flat, items, U, V, scratch_bytes=cap)
    extra = ctx.workspace_bytes() - base
    ms, last = alternate({"from_factors": lambda: ctx.ssim_ragged(flat, items, U, V, scratch_bytes=cap), "decode_all_then_groups": parent_route}, runs, warmup)
    assert torch.equal(last["from_factors"][0], last["decode_all_then_groups"][0]), "the squared errors differ"
    assert torch.equal(last["from_factors"][1].view(torch.int64), last["decode_all_then_groups"][1].view(torch.int64)), "the SSIM bits differ"
    ratio = statistics.median(ms["from_factors"]["events"]) / statistics.median(ms["decode_all_then_groups"]["events"])
    return {"items": int(m), "size_groups": len(groups), "decoded_bytes_of_all_candidates": int(dec_off[-1] + px[-1]), "scratch_cap": cap,
            "workspace_bytes_of_the_call": int(extra), "from_factors": summary(ms["from_factors"]["events"]),
            "decode_all_then_groups": summary(ms["decode_all_then_groups"]["events"]), "from_factors_wall": summary(ms["from_factors"]["wall"]),
            "from_factors_over_parent_route": round(ratio, 4)}


def case_pairs(n, runs, warmup):
    import numpy as np
    import torch
    from conftest import config3_image
    from lrf_amd import _lib
    ctx = _lib.context()
    H, W = 512, 768
    a = torch.stack([config3_image(i) for i in range(24)])[torch.arange(n) % 24].contiguous().cuda()
    b = (a.to(torch.int16) + torch.randint(-6, 7, a.shape, device="cuda", dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
    pairs = np.array([(H, W, 3 * H * W * i, 3 * H * W * i) for i in range(n)], dtype=np.int64)
    ms, last = alternate({"ragged": lambda: ctx.metrics_ragged(a.reshape(-1), b.reshape(-1), pairs, 3), "uniform": lambda: ctx.image_metrics(a, b)}, runs, warmup)
    assert torch.equal(last["ragged"][0], last["uniform"][0]) and torch.equal(last["ragged"][1].view(torch.int64), last["uniform"][1].view(torch.int64))
    return {"pairs": n, "size": [H, W], "ragged": summary(ms["ragged"]["events"]), "uniform": summary(ms["uniform"]["events"]),
            "ragged_over_uniform": round(statistics.median(ms["ragged"]["events"]) / statistics.median(ms["uniform"]["events"]), 4)}


def case_end_to_end(images, runs, warmup, target):
    import torch
    import lrf_amd
    from lrf_amd.codec import select_target_ssim
    from lrf_amd.metrics import psnr_from_sse
    ms, last = alternate({"ssim": lambda: lrf_amd.qmf_encode_target(images, ssim=target, qualities=QUALITIES),
                          "psnr": lambda: lrf_amd.qmf_encode_target(images, 32.0, qualities=QUALITIES)}, runs, warmup)
    out = last["ssim"]
    ctx, flat, items, U, V, row, enc = sweep_of(images)
    enc_ms, _ = wall(enc)
    score_ms, (sse, ssim) = wall(lambda: ctx.ssim_ragged(flat, items, U, V))
    sse_ms, _ = wall(lambda: ctx.sse_ragged(flat, items, U, V))
    row_d = torch.from_numpy(row).cuda()
    samples = torch.tensor([3 * im.shape[1] * im.shape[2] for im in images], dtype=torch.int64)
    sel_ms, _ = wall(lambda: [x.cpu() for x in select_target_ssim(ssim[row_d], psnr_from_sse(sse[row_d], samples)[1], torch.full((len(images),), target, dtype=torch.float64))])
    total = statistics.median(ms["ssim"]["wall"])
    return {"images": len(images), "target_ssim": target, "ssim_target": summary(ms["ssim"]["events"]), "ssim_target_wall": summary(ms["ssim"]["wall"]),
            "psnr_target_32dB": summary(ms["psnr"]["events"]), "chosen_qualities": sorted(set(out["quality"])), "reached": int(out["reached"].sum()),
            "stages_ms": {"timer": "time.perf_counter, device idle before and after, median of 5", "encode_sweep": enc_ms, "scoring_ssim_ragged": score_ms,
                          "scoring_sse_ragged_for_comparison": sse_ms, "selection": sel_ms,
                          "packing_and_the_rest": round(total - enc_ms - score_ms - sel_ms, 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--per-size", type=int, default=8)
    ap.add_argument("--cap", type=int, default=256 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_encode_target_ssim.json"))
    args = ap.parse_args()
    import torch
    from conftest import config3_image
    doc = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "qualities": [QUALITIES[0], QUALITIES[-1]],
           "timer": "HIP events around the call, the stream idle before it", "cases": {}}
    cases = args.cases.split(",")
    n = 32 * args.per_size
    if "a" in cases:
        uniform = [config3_image(i % 24).cuda() for i in range(n)]
        doc["cases"]["a_scoring_uniform"] = case_scoring(uniform, args.runs, args.warmup, args.cap)
        print("a", json.dumps(doc["cases"]["a_scoring_uniform"]), flush=True)
        del uniform
    mixed = mixed_images(args.per_size) if ("b" in cases or "d" in cases) else None
    if "b" in cases:
        doc["cases"]["b_scoring_mixed"] = case_scoring(mixed, args.runs, args.warmup, args.cap)
        print("b", json.dumps(doc["cases"]["b_scoring_mixed"]), flush=True)
    if "c" in cases:
        doc["cases"]["c_pairs_of_one_size"] = case_pairs(n, args.runs, args.warmup)
        print("c", json.dumps(doc["cases"]["c_pairs_of_one_size"]), flush=True)
    if "d" in cases:
        doc["cases"]["d_end_to_end"] = case_end_to_end(mixed, args.runs, args.warmup, 0.95)
        print("d", json.dumps(doc["cases"]["d_end_to_end"]), flush=True)
    scored = [doc["cases"][k] for k in ("a_scoring_uniform", "b_scoring_mixed") if k in doc["cases"]]
    if scored:
        doc["bar"] = {"from_factors_over_parent_route": [c["from_factors_over_parent_route"] for c in scored], "at_most": 1.0,
                      "workspace_bytes_of_the_call": [c["workspace_bytes_of_the_call"] for c in scored],
                      "met": all(c["from_factors_over_parent_route"] <= 1.0 for c in scored)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("bar", {})))


if __name__ == "__main__":
    main()
