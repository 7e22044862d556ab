#!/usr/bin/env python
"""Rate control on a list of mixed image sizes: qmf_encode_target / qmf_encode_budget given a LIST, against what a caller could
do before lists were taken — group the images by size and call the tensor form once per group.

  (a) mixed list: 256 images of 32 distinct sizes around 512x768 (16-aligned, even and odd sides, landscape and portrait), 8 of
      each, qualities 1..32.  `bar`: the list call is faster than the loop over size groups, for both functions (a margin of
      zero).  Next to it the stages of one list call, each timed on its own in one run with one timer (time.perf_counter, the
      device idle before and after): the sweep encode (and inside it planes, Gram, initialisation, BCD from the kernel profile),
      the squared errors, the size count, the selection, and the packing of the winners the list call chose — gather, copy
      and zlib-9 host pack for the target, device deflate plus fold for the budget.
  (b) uniform list: the same 256 images cropped to 512x768, as a list against the tensor call.  The ratio only: the tensor call
      stays the documented choice for uniform batches.
  (c) lrf_qmf_sse_ragged_rgb_u8 alone on the factors of 256 x 512x768 at the rank triples of qualities 1..32 against
      lrf_qmf_sweep_sse_rgb_u8 on the same factors.

Every pair is checked for equal results first, alternated in one process, timed with HIP events around the call (the stream idle
before it) and with time.perf_counter, median of --runs.  Images: the config-3 stand-in set, cropped.  Writes one JSON document
to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

QUALITIES = list(range(1, 33))
K_PLANES, K_INIT, K_BCD, K_VUPDATE, K_GRAM, K_PERSIST = 0, 1, 2, 3, 5, 6


def sizes32():
    """32 distinct sizes around 512x768: rows of four heights x four widths, landscape, then the same portrait"""
    hs, ws = (512, 496, 487, 450), (768, 752, 731, 700)  # 16-aligned, 16-aligned, odd, even
    land = [(h, w) for h in hs for w in ws]
    return land + [(w, h) for h, w in land]


def mixed_images(n_per_size=8):
    import torch
    from conftest import config3_image
    base = [config3_image(i) for i in range(24)]
    out = []
    for k, (H, W) in enumerate(sizes32()):
        for j in range(n_per_size):
            im = base[(k * n_per_size + j) % 24]
            if H > W:
                im = im.transpose(1, 2)
            out.append(im[:, :H, :W].contiguous().cuda())
    order = torch.randperm(len(out), generator=torch.Generator().manual_seed(1)).tolist()  # a folder is not sorted by size
    return [out[i] for i in order]


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t) * 1e3, out


def alternate(routes, runs, warmup):
    """routes: {name: fn} -> ({name: {"events": [...], "wall": [...]}}, {name: last result})"""
    ms = {k: {"events": [], "wall": []} for k in routes}
    last = {}
    for i in range(warmup + runs):
        for k, fn in routes.items():
            ev, wall, last[k] = timed(fn)
            if i >= warmup:
                ms[k]["events"].append(ev)
                ms[k]["wall"].append(wall)
    return ms, last


def by_size_group(fn, images, **kw):
    """the parent's route: the tensor form once per size group, results put back in list order"""
    import torch
    groups = {}
    for i, im in enumerate(images):
        groups.setdefault(tuple(im.shape), []).append(i)
    streams, quality = [None] * len(images), [None] * len(images)
    for idx in groups.values():
        out = fn(torch.stack([images[i] for i in idx]), qualities=QUALITIES, **kw)
        for k, i in enumerate(idx):
            streams[i], quality[i] = out["streams"][k], out["quality"][k]
    return {"streams": streams, "quality": quality}


def wall(fn, reps=5):
    """median wall time of fn in ms, the device idle before and after"""
    import torch
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms), 3), out


def stages(images, chosen):
    """one list call taken apart.  chosen: {"target": [quality per image], "budget": [...]}, what the list calls picked"""
    import numpy as np
    import torch
    import lrf_amd
    from lrf_amd import _lib
    from lrf_amd.codec import (default_pack_threads, pack_streams_ragged_native, qmf_ranks, select_budget, select_target, streams_from_device_factors,
                               target_candidates)
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
    ctx.encode_ragged_sweep(flat, ims, cands, 10, -16, 15)  # (tables resident, workspaces allocated)
    enc_ms, (U, V, u_off, v_off) = wall(lambda: ctx.encode_ragged_sweep(flat, ims, cands, 10, -16, 15))
    ctx.profile(True)
    ctx.profile_reset()
    ctx.encode_ragged_sweep(flat, ims, cands, 10, -16, 15)
    torch.cuda.synchronize()
    prof = {name: round(ctx.kernel_time(k)[0], 3) for name, k in (("planes", K_PLANES), ("gram", K_GRAM), ("init", K_INIT), ("bcd", K_BCD),
                                                                    ("vupdate", K_VUPDATE), ("bcd_persist", K_PERSIST))}
    ctx.profile(False)
    hw = np.array(sizes, dtype=np.int64)[owner]
    items = np.concatenate([hw, ranks, np.asarray(u_off).reshape(-1, 1), np.asarray(v_off).reshape(-1, 1), np.asarray(offs)[owner].reshape(-1, 1)], axis=1)
    sse_ms, sse = wall(lambda: ctx.sse_ragged(flat, items, U, V))
    cnt_ms, size = wall(lambda: lrf_amd.qmf_stream_sizes_ragged(U, V, hw, ranks, u_off, v_off))
    first = np.cumsum(counts) - counts
    row = torch.from_numpy(first.reshape(1, n) + np.array([[ts.index(tuple(qmf_ranks(s_, None, q))) for q in QUALITIES] for ts, s_ in zip(per, sizes)]).T).cuda()
    samples = torch.tensor([3 * H * W for H, W in sizes], dtype=torch.int64)
    sel_t_ms, _ = wall(lambda: [x.cpu() for x in select_target(sse[row], samples, torch.full((n,), 32.0, dtype=torch.float64))])
    budget = torch.tensor([int(0.25 * H * W / 8) for H, W in sizes], dtype=torch.int64)
    sel_b_ms, _ = wall(lambda: [x.cpu() for x in select_budget(size[row], sse[row], budget)])
    rec = {"candidates": int(cands.shape[0]), "x_bytes": 4 * 64 * sum(sum(d[4] for d in _lib.plane_dims(*s_)) for s_ in sizes), "factor_bytes": U.numel() + V.numel(),
           "timer": "time.perf_counter, device idle before and after, median of 5", "encode_sweep_ms": enc_ms, "encode_sweep_kernels_ms": prof, "sse_ms": sse_ms,
           "sizes_ms": cnt_ms, "select_target_ms": sel_t_ms, "select_budget_ms": sel_b_ms}
    for name in ("target", "budget"):
        win = [int(first[k]) + per[k].index(tuple(qmf_ranks(sizes[k], None, q))) for k, q in enumerate(chosen[name])]
        w_triples = [ranks[j].tolist() for j in win]
        nus = [sum(d[4] * r for d, r in zip(_lib.plane_dims(*s_), t)) for s_, t in zip(sizes, w_triples)]
        nvs = [64 * sum(t) for t in w_triples]

        def pack_host():
            Uw = torch.cat([U[u_off[j]:u_off[j] + nu] for j, nu in zip(win, nus)])
            Vw = torch.cat([V[v_off[j]:v_off[j] + nv] for j, nv in zip(win, nvs)])
            Uh, Vh = (x.numpy() for x in ctx.to_host(Uw, Vw))
            return pack_streams_ragged_native(Uh, Vh, sizes, w_triples, np.cumsum([0] + nus[:-1]).tolist(), np.cumsum([0] + nvs[:-1]).tolist(), (-16, 15),
                                              threads=default_pack_threads())[0]

        def pack_device():
            return streams_from_device_factors(ctx, U, V, sizes, w_triples, [u_off[j] for j in win], [v_off[j] for j in win], (-16, 15), default_pack_threads())
        rec["pack_" + name + "_ms"], streams = wall(pack_host if name == "target" else pack_device, reps=3)
        rec["pack_" + name + "_bytes"] = sum(len(x) for x in streams)
    return rec


def case_lists(images, runs, warmup, with_stages):
    import lrf_amd
    rec = {"images": len(images), "sizes": len({tuple(im.shape) for im in images})}
    chosen = {}
    for name, fn, kw in (("target", lrf_amd.qmf_encode_target, dict(psnr=32.0)), ("budget", lrf_amd.qmf_encode_budget, dict(bpp=0.25))):
        ms, last = alternate({"list": lambda: fn(images, qualities=QUALITIES, **kw), "size_groups": lambda: by_size_group(fn, images, **kw)}, runs, warmup)
        assert last["list"]["streams"] == last["size_groups"]["streams"] and last["list"]["quality"] == last["size_groups"]["quality"], name
        rec[name] = {"list": summary(ms["list"]["events"]), "size_groups": summary(ms["size_groups"]["events"]),
                     "list_wall": summary(ms["list"]["wall"]), "size_groups_wall": summary(ms["size_groups"]["wall"]),
                     "list_over_size_groups": round(statistics.median(ms["list"]["events"]) / statistics.median(ms["size_groups"]["events"]), 4),
                     "chosen_qualities": sorted(set(last["list"]["quality"])), "reached": int(last["list"]["reached"].sum())}
        chosen[name] = last["list"]["quality"]
        print(name, json.dumps(rec[name]), flush=True)
    if with_stages:
        rec["stages_of_one_list_call"] = stages(images, chosen)
    return rec


def case_uniform(images, runs, warmup):
    import torch
    import lrf_amd
    crops = [im[:, :512, :768] if im.shape[1] >= 512 and im.shape[2] >= 768 else None for im in images]
    from conftest import config3_image
    base = [config3_image(i).cuda() for i in range(24)]
    crops = [c.contiguous() if c is not None else base[i % 24] for i, c in enumerate(crops)]
    batch = torch.stack(crops)
    rec = {"images": len(crops), "size": [512, 768]}
    for name, fn, kw in (("target", lrf_amd.qmf_encode_target, dict(psnr=32.0)), ("budget", lrf_amd.qmf_encode_budget, dict(bpp=0.25))):
        ms, last = alternate({"list": lambda: fn(crops, qualities=QUALITIES, **kw), "tensor": lambda: fn(batch, qualities=QUALITIES, **kw)}, runs, warmup)
        assert last["list"]["streams"] == last["tensor"]["streams"], name
        rec[name] = {"list": summary(ms["list"]["events"]), "tensor": summary(ms["tensor"]["events"]),
                     "list_over_tensor": round(statistics.median(ms["list"]["events"]) / statistics.median(ms["tensor"]["events"]), 4)}
        print(name, json.dumps(rec[name]), flush=True)
    return rec


def case_sse(n, runs, warmup):
    import torch
    from conftest import config3_image
    from lrf_amd import _lib
    from lrf_amd.codec import target_candidates
    ctx = _lib.context()
    H, W = 512, 768
    base = torch.stack([config3_image(i) for i in range(24)])
    dev = base[torch.arange(n) % 24].contiguous().cuda()
    triples = target_candidates((H, W), QUALITIES)[0]
    pairs = ctx.encode_sweep_rgb(dev, triples, 10, -16, 15)
    U, V = _lib.flat_views([p[0] for p in pairs]), _lib.flat_views([p[1] for p in pairs])
    items, uo, vo = [], 0, 0
    for t, (Uq, Vq) in zip(triples, pairs):
        for b in range(n):
            items.append((H, W, t[0], t[1], t[2], uo + b * Uq.shape[1], vo + b * Vq.shape[1], b * 3 * H * W))
        uo, vo = uo + Uq.numel(), vo + Vq.numel()
    import numpy as np
    items = np.array(items, dtype=np.int64)
    flat = dev.reshape(-1)
    ms, last = alternate({"ragged": lambda: ctx.sse_ragged(flat, items, U, V), "uniform": lambda: ctx.sweep_sse(dev, pairs, triples)}, runs, warmup)
    assert torch.equal(last["ragged"].view(len(triples), n), last["uniform"]), "the ragged and the uniform scorer disagree"
    return {"images": n, "size": [H, W], "triples": len(triples), "items": len(items),
            "ragged": summary(ms["ragged"]["events"]), "uniform": summary(ms["uniform"]["events"]), "ragged_wall": summary(ms["ragged"]["wall"]),
            "ragged_over_uniform": round(statistics.median(ms["ragged"]["events"]) / statistics.median(ms["uniform"]["events"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--per-size", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_rate_control_ragged.json"))
    args = ap.parse_args()
    import torch
    import lrf_amd
    doc = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "qualities": [QUALITIES[0], QUALITIES[-1]],
           "pack_threads": lrf_amd.codec.default_pack_threads(), "timer": "HIP events around the call, the stream idle before it", "cases": {}}
    cases = args.cases.split(",")
    images = mixed_images(args.per_size) if ("a" in cases or "b" in cases) else None
    if "a" in cases:
        doc["cases"]["a_mixed_list"] = case_lists(images, args.runs, args.warmup, True)
        r = doc["cases"]["a_mixed_list"]
        ratios = {k: r[k]["list_over_size_groups"] for k in ("target", "budget")}
        doc["bar"] = {"list_over_size_groups": ratios, "below": 1.0, "met": all(v < 1.0 for v in ratios.values())}
    if "b" in cases:
        doc["cases"]["b_uniform_list"] = case_uniform(images, args.runs, args.warmup)
    del images
    torch.cuda.empty_cache()
    if "c" in cases:
        doc["cases"]["c_sse_alone"] = case_sse(32 * args.per_size, args.runs, args.warmup)
        print("c", json.dumps(doc["cases"]["c_sse_alone"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("bar", {})))


if __name__ == "__main__":
    main()
