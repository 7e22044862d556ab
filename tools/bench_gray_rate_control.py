#!/usr/bin/env python
"""Gray image lists on the encode side: the one-call routes against what a caller could do before them.

  (a) 256 gray images of 32 sizes around 512x768 at rank 7: Context.encode_gray_ragged (one lrf_qmf_encode_gray_ragged_u8 call)
      against one lrf_qmf_encode_gray_u8 call per size group (Context.encode_gray on the stacked group).
  (b) the same list through qmf_encode_target(32 dB) and qmf_encode_budget(0.25 bpp) with color_space="RGB" over qualities 1..32,
      against the route that existed before: per size group and per distinct rank one qmf_encode_batch(color_space="RGB"), then
      qmf_decode_ragged of all streams, the squared errors, and the choice on the host.  For the target the two routes' streams
      are compared first.  For the budget the earlier route can only measure zlib-9 streams (there was no device coder for
      two-factor containers), so its choice is made on those sizes and only the times are set side by side.  Next to it the
      stages of one list call, each timed on its own: sweep, squared errors, size count, selection, packing of the winners.
  (c) 256 x 512x768 uniform: qmf_encode_ragged(color_space="RGB") of the list against qmf_encode_batch(color_space="RGB") of the
      tensor.  Reported, not barred: the uniform call stays the one to use.

The routes of a pair alternate in one process, timed with HIP events around the call (the stream idle before it) and with
time.perf_counter: median of --runs with the smallest and the largest beside it.  Images: the config-3 stand-in set as integer
luma, cropped.  `bar`: on (a) and (b) the one-call route is faster.  Writes one JSON document to --out."""
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


def sizes32():
    """32 distinct sizes around 512x768: rows of four heights x four widths, landscape, then the same portrait"""
    hs, ws = (512, 496, 487, 450), (768, 752, 731, 700)  # 16-aligned, 16-aligned, odd, even
    land = [(h, w) for h in hs for w in ws]
    return land + [(w, h) for h, w in land]


def gray_of(rgb):
    """integer luma of a uint8 [3,H,W] image -> uint8 [1,H,W]"""
    r, g, b = (rgb[c].int() for c in range(3))
    return ((77 * r + 150 * g + 29 * b) >> 8).to(rgb.dtype)[None]


def mixed_images(n_per_size=8):
    import torch
    from conftest import config3_image
    base = [gray_of(config3_image(i)) for i in range(24)]
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
            ev, wall_ms, last[k] = timed(fn)
            if i >= warmup:
                ms[k]["events"].append(ev)
                ms[k]["wall"].append(wall_ms)
    return ms, last


def pair(ms, one, other):
    return {one: summary(ms[one]["events"]), other: summary(ms[other]["events"]), one + "_wall": summary(ms[one]["wall"]),
            other + "_wall": summary(ms[other]["wall"]),
            one + "_over_" + other: round(statistics.median(ms[one]["events"]) / statistics.median(ms[other]["events"]), 4)}


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


def groups_of(images):
    groups = {}
    for i, im in enumerate(images):
        groups.setdefault(tuple(im.shape), []).append(i)
    return list(groups.values())


def flat_of(images):
    import torch
    offs, off = [], 0
    for im in images:
        offs.append(off)
        off = (off + im.numel() + 15) // 16 * 16
    flat = torch.empty((off,), dtype=torch.uint8, device="cuda")
    for im, o in zip(images, offs):
        flat[o:o + im.numel()].view(im.shape).copy_(im)
    return flat, offs


def case_encode(images, runs, warmup, R=7):
    import torch
    from lrf_amd import _lib
    ctx = _lib.context()
    flat, offs = flat_of(images)
    desc = [(im.shape[1], im.shape[2], R, o) for im, o in zip(images, offs)]
    groups = groups_of(images)
    stacked = [torch.stack([images[i][0] for i in idx]) for idx in groups]

    def by_group():
        return [ctx.encode_gray(batch, R, 10, (-16, 15)) for batch in stacked]

    ms, last = alternate({"ragged": lambda: ctx.encode_gray_ragged(flat, desc, 10, -16, 15), "size_groups": by_group}, runs, warmup)
    U, V, u_off, v_off = last["ragged"]
    for idx, (Ug, Vg) in zip(groups, last["size_groups"]):
        for k, i in enumerate(idx):
            assert torch.equal(U[u_off[i]:u_off[i] + Ug[k].numel()], Ug[k].reshape(-1)) and torch.equal(V[v_off[i]:v_off[i] + 64 * R], Vg[k].reshape(-1)), i
    return dict(images=len(images), sizes=len(groups), rank=R, **pair(ms, "ragged", "size_groups"))


def earlier_route(images, budget_mode, goal):
    """per size group and distinct rank one batch call, every stream decoded, scored and measured, the choice on the host"""
    import torch
    import lrf_amd
    from lrf_amd.codec import gray_target_candidates, select_budget, select_target
    n = len(images)
    streams, quality = [None] * n, [None] * n
    for idx in groups_of(images):
        batch = torch.stack([images[i] for i in idx])
        H, W = batch.shape[-2:]
        _, lowest = gray_target_candidates((H, W), QUALITIES)
        cand = [lrf_amd.qmf_encode_batch(batch, quality=q, color_space="RGB") for q in lowest]
        dec = lrf_amd.qmf_decode_ragged([s for c in cand for s in c])
        sse = torch.stack([((d.long() - batch[k % len(idx)].long()) ** 2).sum() for k, d in enumerate(dec)]).view(len(lowest), len(idx))
        if budget_mode:
            size = torch.tensor([[len(s) for s in c] for c in cand], dtype=torch.int64, device=sse.device)
            index, _ = select_budget(size, sse, torch.full((len(idx),), int(goal * H * W / 8), dtype=torch.int64))
        else:
            _, index, _ = select_target(sse, H * W, torch.full((len(idx),), goal, dtype=torch.float64))
        for k, (i, j) in enumerate(zip(idx, index.cpu().tolist())):
            streams[i], quality[i] = cand[j][k], lowest[j]
    return {"streams": streams, "quality": quality}


def stages(images, chosen):
    """one list call taken apart.  chosen: {"target": [quality per image], "budget": [...]}, what the list calls picked"""
    import numpy as np
    import torch
    import lrf_amd
    from lrf_amd import _lib
    from lrf_amd.codec import _gray_host_streams, gray_streams_from_device_factors, gray_target_candidates, select_budget, select_target
    ctx = _lib.context()
    sizes = [tuple(im.shape[1:]) for im in images]
    n = len(images)
    flat, offs = flat_of(images)
    per = [gray_target_candidates(hw, QUALITIES)[0] for hw in sizes]
    Ms = [_lib.chan_dims(hw[0], hw[1], 1, (8, 8))[2] for hw in sizes]
    counts = np.array([len(t) for t in per], dtype=np.int64)
    first = np.cumsum(counts) - counts
    owner = np.repeat(np.arange(n, dtype=np.int64), counts).tolist()
    ranks = [r for rs in per for r in rs]
    ims = [(H, W, o) for (H, W), o in zip(sizes, offs)]
    cands = list(zip(owner, ranks))
    ctx.encode_gray_ragged_sweep(flat, ims, cands, 10, -16, 15)  # (tables resident, workspaces allocated)
    enc_ms, (U, V, u_off, v_off) = wall(lambda: ctx.encode_gray_ragged_sweep(flat, ims, cands, 10, -16, 15))
    c_hw = [sizes[k] for k in owner]
    items = [(hw[0], hw[1], r, uo, vo, offs[k]) for hw, r, uo, vo, k in zip(c_hw, ranks, u_off, v_off, owner)]
    sse_ms, sse = wall(lambda: ctx.sse_gray_ragged(flat, items, U, V))
    cnt_ms, size = wall(lambda: lrf_amd.qmf_stream_sizes_gray_ragged(U, V, c_hw, ranks, u_off, v_off))
    row = torch.from_numpy(first.reshape(1, n) + np.array([[rs.index(int(_lib.chan_rank(M, 64, None, q))) for q in QUALITIES] for rs, M in zip(per, Ms)]).T).cuda()
    samples = torch.tensor([H * W for H, W in sizes], dtype=torch.int64)
    sel_t_ms, _ = wall(lambda: [x.cpu() for x in select_target(sse[row], samples, torch.full((n,), 32.0, dtype=torch.float64))])
    budget = torch.tensor([int(0.25 * H * W / 8) for H, W in sizes], dtype=torch.int64)
    sel_b_ms, _ = wall(lambda: [x.cpu() for x in select_budget(size[row], sse[row], budget)])
    rec = {"candidates": len(cands), "x_bytes": 4 * 64 * sum(Ms), "factor_bytes": U.numel() + V.numel(),
           "timer": "time.perf_counter, device idle before and after, median of 5", "encode_sweep_ms": enc_ms, "sse_ms": sse_ms, "sizes_ms": cnt_ms,
           "select_target_ms": sel_t_ms, "select_budget_ms": sel_b_ms}
    for name in ("target", "budget"):
        win = [int(first[k]) + per[k].index(int(_lib.chan_rank(Ms[k], 64, None, q))) for k, q in enumerate(chosen[name])]
        w_ranks = [ranks[j] for j in win]
        nus, nvs = [M * r for M, r in zip(Ms, w_ranks)], [64 * r for r in w_ranks]

        def pack_host():
            Uw = torch.cat([U[u_off[j]:u_off[j] + nu] for j, nu in zip(win, nus)])
            Vw = torch.cat([V[v_off[j]:v_off[j] + nv] for j, nv in zip(win, nvs)])
            Uh, Vh = (x.numpy() for x in ctx.to_host(Uw, Vw))
            return _gray_host_streams(Uh, Vh, sizes, w_ranks, np.cumsum([0] + nus[:-1]).tolist(), np.cumsum([0] + nvs[:-1]).tolist(), (-16, 15), None)

        def pack_device():
            return gray_streams_from_device_factors(ctx, U, V, sizes, w_ranks, [u_off[j] for j in win], [v_off[j] for j in win], (-16, 15))
        rec["pack_" + name + "_ms"], streams = wall(pack_host if name == "target" else pack_device, reps=3)
        rec["pack_" + name + "_bytes"] = sum(len(x) for x in streams)
    return rec


def case_rate(images, runs, warmup):
    import lrf_amd
    rec = {"images": len(images), "sizes": len(groups_of(images))}
    chosen = {}
    for name, fn, kw, goal in (("target", lrf_amd.qmf_encode_target, dict(psnr=32.0), 32.0), ("budget", lrf_amd.qmf_encode_budget, dict(bpp=0.25), 0.25)):
        routes = {"list": lambda: fn(images, qualities=QUALITIES, color_space="RGB", **kw), "earlier": lambda: earlier_route(images, name == "budget", goal)}
        ms, last = alternate(routes, runs, warmup)
        if name == "target":
            assert last["list"]["streams"] == last["earlier"]["streams"] and last["list"]["quality"] == last["earlier"]["quality"], name
        rec[name] = dict(pair(ms, "list", "earlier"), chosen_qualities=sorted(set(last["list"]["quality"])), reached=int(last["list"]["reached"].sum()),
                         same_streams=last["list"]["streams"] == last["earlier"]["streams"])
        chosen[name] = last["list"]["quality"]
        print(name, json.dumps(rec[name]), flush=True)
    rec["stages_of_one_list_call"] = stages(images, chosen)
    return rec


def case_uniform(n, runs, warmup):
    import torch
    import lrf_amd
    from conftest import config3_image
    base = [gray_of(config3_image(i)).cuda() for i in range(24)]
    batch = torch.stack([base[i % 24] for i in range(n)])
    images = list(batch)
    ms, last = alternate({"list": lambda: lrf_amd.qmf_encode_ragged(images, rank=7, color_space="RGB"),
                          "tensor": lambda: lrf_amd.qmf_encode_batch(batch, rank=7, color_space="RGB")}, runs, warmup)
    assert last["list"] == last["tensor"]
    return dict(images=n, size=[512, 768], rank=7, **pair(ms, "list", "tensor"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--per-size", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_gray_rate_control.json"))
    args = ap.parse_args()
    import torch
    import lrf_amd
    doc = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "qualities": [QUALITIES[0], QUALITIES[-1]],
           "pack_threads": lrf_amd.codec.default_pack_threads(), "timer": "HIP events around the call, the stream idle before it", "cases": {}}
    cases = args.cases.split(",")
    images = mixed_images(args.per_size) if ("a" in cases or "b" in cases) else None
    ratios = {}
    if "a" in cases:
        doc["cases"]["a_ragged_encode"] = case_encode(images, args.runs, args.warmup)
        ratios["encode"] = doc["cases"]["a_ragged_encode"]["ragged_over_size_groups"]
        print("a", json.dumps(doc["cases"]["a_ragged_encode"]), flush=True)
    if "b" in cases:
        doc["cases"]["b_rate_control"] = case_rate(images, args.runs, args.warmup)
        for k in ("target", "budget"):
            ratios[k] = doc["cases"]["b_rate_control"][k]["list_over_earlier"]
    if ratios:
        doc["bar"] = {"one_call_over_earlier_route": ratios, "below": 1.0, "met": all(v < 1.0 for v in ratios.values())}
    del images
    torch.cuda.empty_cache()
    if "c" in cases:
        doc["cases"]["c_uniform_list"] = case_uniform(32 * args.per_size, args.runs, args.warmup)
        print("c", json.dumps(doc["cases"]["c_uniform_list"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc.get("bar", {})))


if __name__ == "__main__":
    main()
