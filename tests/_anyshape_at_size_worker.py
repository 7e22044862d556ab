"""Child process of tests/test_anyshape_at_size.py: the any-shape kernels (lrf_anyshape_kernels.hip; which variant a call takes:
plan_any_prod / plan_any_gs / plan_any_init_chunk, lrf_plan.cpp) at production batch sizes and at ranks up to LRF_ANY_MAX_RANK,
against the CPU oracle.  `python _anyshape_at_size_worker.py <section>` runs one section on the GPU and prints one
"RESULT {json}" line per case: the kernel timers' counts (LRF_K_INIT and LRF_K_BCD regions), how many images / matrices and
planes were compared, the differing ones, and what ctx.synchronize() / ctx.check() said afterwards.  The parent asserts; this
file only reports.

The case tables are at the top and import nothing heavy: tests/test_any_plan.py reads them on the CPU and states, per case,
which kernel variants and loop counts it reaches."""
import json
import os
import sys
import time

import numpy as np

POOL = 16  # oracle threads: a fixed number, never os.cpu_count() (shared hosts grant a job far fewer cores than they have)
D = (-16, 15)
K_BATCH = 10

# ---- section "batches": qmf_encode_batch's per-plane calls (Context.planes_any + Context.decompose: what _qmf_encode_anyshape
# does, without packing and parsing 256 containers), every image and plane against oracle.qmf_anyshape_decompose.
# (name, (B, H, W), patch size or None, quality, the ranks anyshape_ranks gives (asserted in test_any_plan.py), caller signs)
# B = 256 for all four shipping configurations.  32x32 and patch=False could do with fewer (their kernels, k_any_prod_big and
# k_any_prod with a long contraction, take the batch as a grid dimension only: test_any_plan.py shows the same variants and
# loop counts from B = 1 on), but the oracle pool hides behind nothing else and 256 is where README's timings are taken.
# "6x8" and "4x8 q60" are no shipping configurations: they reach k_any_prod_thin_short<16> / <8>, tpw 2 and 4, and k_any_prod
# with several row tiles per workgroup.  "4x4 ragged": 500x760 images, a partial last 16-row tile and a wave that runs out of
# tiles inside its tpw loop, in luma (1485 tiles, tpw 16) and chroma (375 tiles, tpw 8).
BATCH_CASES = [
    ("4x4", (256, 512, 768), (4, 4), 20, (3, 2, 2), False),
    ("16x16", (256, 512, 768), (16, 16), 20, (51, 26, 26), False),
    ("32x32", (256, 512, 768), (32, 32), 20, (77, 10, 10), False),
    ("none", (256, 512, 768), None, 20, (102, 26, 26), False),
    ("4x8 q60", (256, 512, 768), (4, 8), 60, (19, 10, 10), False),
    # a different sign vector per image: tall matrices take them in the eigen-solver (sign + b0 * R), wide ones in k_any_signfix
    ("4x4 signs", (256, 512, 768), (4, 4), 20, (3, 2, 2), True),
    ("32x32 signs", (32, 512, 768), (32, 32), 20, (77, 10, 10), True),
    ("6x8", (48, 512, 768), (6, 8), 20, (10, 5, 5), False),
    ("4x4 ragged", (256, 500, 760), (4, 4), 20, (3, 2, 2), False),
]
# ---- section "chunked": any_run_init in two chunks.  min side 1024, rank 4: a chunk is floor(2^31 / (8 (1024^2 + 3 * 1024 * 4)))
# = floor(2147483648 / 8486912) = 253 matrices; 254 is the smallest batch with a second, unequal chunk (one matrix).
CHUNK = dict(B=254, chunk=253, R=4, tall=(1100, 1024), wide=(1024, 1100))


def chunk_subset(B, chunk):
    """the matrices compared with the oracle: first and last of each chunk and every 16th in between — both sides of the boundary"""
    idx = set()
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        idx |= {b0, b1 - 1} | set(range(b0, b1, 16))
    return sorted(idx)


# ---- section "ladder": the library's own initialisation, then K = 2, two matrices per call (the second integer-valued)
LADDER_RANKS = [121, 128, 129, 192, 256, 257, 400, 512, 629, 630, 639]
LADDER_SHAPES = [(700, 660), (660, 700)]
LADDER_K = 2
# (name, M, N, R, rank of the matrices' content or None)
LADDER_EXTRA = [("wide", 300, 2048, 200, None), ("rank-deficient", 700, 660, 639, 220)]
# ---- section "general": Context.decompose_ex from given initial factors against oracle.bcd_ex, three distinct matrices per call
GENERAL_B = 3
GENERAL_K = 3
GENERAL_SHAPES = [(24576, 16, 3), (1536, 256, 51), (96, 1024, 10), (5, 16, 3), (130, 100, 101)]
GENERAL_OPTS = [
    ("unbounded", dict(bounds=(None, None), factor=(0, 1))),
    ("bounded", dict(bounds=D, factor=(0, 1))),
    ("l2 l1=0", dict(bounds=D, l2=(1.0, 0.25), l1_ratio=0.0, factor=(0, 1))),
    ("l2 l1=0.3", dict(bounds=D, l2=(1.0, 0.25), l1_ratio=0.3, factor=(0, 1))),
    ("l2 l1=1", dict(bounds=(None, None), l2=(1.0, 0.25), l1_ratio=1.0, factor=(0, 1))),
    ("factor u", dict(bounds=D, factor=(0,))),
    ("factor v", dict(bounds=D, factor=(1,))),
    ("eps", dict(bounds=D, factor=(0, 1), eps=1e-3)),
]
GENERAL_W_SHAPE = (1536, 256, 51)  # factor=(0, 1, 2): w is updated, judged as tests/test_qmf_class.py::test_hip_general_bcd judges it


def general_name(shape, opt):
    return f"{list(shape)} {opt}"


# ---------------------------------------------------------------------------------------------------------------------------
def timed(ctx, fn):
    """fn() with the two kernel timers on: (result, LRF_K_INIT regions, LRF_K_BCD regions)"""
    import torch
    from lrf_amd import _lib
    ctx.profile_kernels([_lib.LRF_K_INIT, _lib.LRF_K_BCD])
    ctx.profile_reset()
    out = fn()
    torch.cuda.synchronize()
    ninit = ctx.kernel_time(_lib.LRF_K_INIT)[1]
    nbcd = ctx.kernel_time(_lib.LRF_K_BCD)[1]
    ctx.profile(False)
    return out, ninit, nbcd


def bits_differ(case, b, kind, plane, name, got, want):
    """fp32 arrays compared as bit patterns: None or the message"""
    from _persist_at_size_worker import diff_message
    g, w = np.ascontiguousarray(got, np.float32).view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32)
    return None if g.shape == w.shape and np.array_equal(g, w) else diff_message(case, b, kind, plane, name, g, w)


def section_batches():
    import torch
    import lrf_amd
    from concurrent.futures import ThreadPoolExecutor
    from _persist_at_size_worker import build_images, ctx_state, diff_message, emit
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    pool = ThreadPoolExecutor(max_workers=POOL)
    sets = {}
    for name, geom, ps, quality, ranks, signs in BATCH_CASES:
        B, H, W = geom
        if geom not in sets:
            sets.clear()  # one image set on the device at a time
            imgs, kinds = build_images(B, H, W, 23 + H + B)
            sets[geom] = (imgs, kinds, imgs.cpu().numpy())
        imgs, kinds, host = sets[geom]
        offs = [sum(ranks[:c]) for c in range(3)]
        sg = None
        if signs:
            sg = (np.random.default_rng(B + sum(ranks)).integers(0, 2, (B, sum(ranks))) * 2 - 1).astype(np.int8)

        def want_of(b):
            s = None if sg is None else [sg[b, offs[c]:offs[c] + ranks[c]] for c in range(3)]
            return [(u.astype(np.int8), v.astype(np.int8)) for u, v in oracle.qmf_anyshape_decompose(host[b], ps, list(ranks), K_BATCH, D, signs=s)]

        t0 = time.perf_counter()
        futures = [pool.submit(want_of, b) for b in range(B)]  # the oracle runs while the GPU does
        got, ninit, nbcd = [], 0, 0
        for c in range(3):
            X = ctx.planes_any(imgs, ps, c)
            sign = None if sg is None else torch.from_numpy(np.ascontiguousarray(sg[:, offs[c]:offs[c] + ranks[c]])).cuda()
            (U, V), ni, nb = timed(ctx, lambda: ctx.decompose(X, ranks[c], K_BATCH, D[0], D[1], sign))
            got.append((U.cpu().numpy(), V.cpu().numpy()))
            ninit, nbcd = ninit + ni, nbcd + nb
        state = ctx_state(ctx)
        t1 = time.perf_counter()
        bad, nplanes = [], 0
        for b in range(B):
            want = futures[b].result()
            for c in range(3):
                nplanes += 1
                for fname, g_, w_ in (("U", got[c][0][b], want[c][0]), ("V", got[c][1][b], want[c][1])):
                    if g_.shape != w_.shape or not np.array_equal(g_, w_):
                        bad.append(diff_message(name, b, kinds[b], "Y Cb Cr".split()[c], fname, g_, w_))
        emit(section="batches", case=name, init=ninit, bcd=nbcd, images=B, planes=nplanes, nbad=len(bad), bad=bad[:8], ctx=state,
             gpu_s=round(t1 - t0, 3), oracle_wait_s=round(time.perf_counter() - t1, 3))
        del got, futures
        ctx.trim()


def section_chunked():
    import torch
    import lrf_amd
    from concurrent.futures import ThreadPoolExecutor
    from _persist_at_size_worker import ctx_state, emit
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    pool = ThreadPoolExecutor(max_workers=POOL)
    B, chunk, R = CHUNK["B"], CHUNK["chunk"], CHUNK["R"]
    subset = chunk_subset(B, chunk)
    for orient in ("tall", "wide"):
        M, N = CHUNK[orient]
        g = torch.Generator(device="cuda").manual_seed(M)
        X = torch.empty((B, M, N), device="cuda")
        for b0 in range(0, B, 32):  # low rank plus noise, a different matrix each; every other one integer-valued
            n = min(32, B - b0)
            X[b0:b0 + n] = torch.randn((n, M, 6), device="cuda", generator=g) @ torch.randn((n, 6, N), device="cuda", generator=g) * 20 \
                + torch.randn((n, M, N), device="cuda", generator=g) * 5 + 100
        X[1::2] = torch.round(X[1::2])
        sign = sg = None
        if orient == "tall":  # per-matrix signs: the eigen-solver reads sign + b0 * R of the chunk
            sg = (np.random.default_rng(5).integers(0, 2, (B, R)) * 2 - 1).astype(np.int8)
            sign = torch.from_numpy(sg).cuda()
        Xh = {b: X[b].cpu().numpy() for b in subset}
        t0 = time.perf_counter()
        futures = {b: pool.submit(oracle.svd_topr_any, Xh[b], R, None if sg is None else sg[b]) for b in subset}
        (U0, V0), ninit, nbcd = timed(ctx, lambda: ctx.svd_init(X, R, sign))
        t1 = time.perf_counter()
        alone_bad = []  # every matrix factorised alone, HIP against HIP
        for b in range(B):
            u1, v1 = ctx.svd_init(X[b:b + 1], R, None if sign is None else sign[b:b + 1])
            if not (torch.equal(u1[0].view(torch.int32), U0[b].view(torch.int32)) and torch.equal(v1[0].view(torch.int32), V0[b].view(torch.int32))):
                alone_bad.append(b)
        state = ctx_state(ctx)
        t2 = time.perf_counter()
        Uh, Vh = U0.cpu().numpy(), V0.cpu().numpy()
        bad = []
        for b in subset:
            uo, vo = futures[b].result()
            for fname, g_, w_ in (("U0", Uh[b], uo), ("V0", Vh[b], vo)):
                m = bits_differ(f"chunked {orient}", b, "integer" if b % 2 else "float", "-", fname, g_, w_)
                if m:
                    bad.append(m)
        emit(section="chunked", case=orient, init=ninit, bcd=nbcd, images=B, subset=subset, planes=len(subset), nbad=len(bad), bad=bad[:8],
             alone=B, alone_bad=alone_bad[:16], ctx=state, gpu_s=round(t1 - t0, 3), alone_s=round(t2 - t1, 3),
             oracle_wait_s=round(time.perf_counter() - t2, 3))
        del X, U0, V0
        ctx.trim()
        torch.cuda.empty_cache()


def section_ladder():
    import torch
    import lrf_amd
    from concurrent.futures import ThreadPoolExecutor
    from _persist_at_size_worker import ctx_state, diff_message, emit
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    pool = ThreadPoolExecutor(max_workers=POOL)

    def want_of(X, R):
        u0, v0 = oracle.svd_topr_any(X, R)
        u, v = oracle.bcd(X, u0, v0, LADDER_K, D)
        return u.astype(np.int8), v.astype(np.int8)

    cases = [(f"[{M}, {N}] R={R}", M, N, R, None) for M, N in LADDER_SHAPES for R in LADDER_RANKS]
    cases += [(f"{name} [{M}, {N}] R={R}", M, N, R, k) for name, M, N, R, k in LADDER_EXTRA]
    pending = []
    for name, M, N, R, k in cases:
        rng = np.random.default_rng(M * 131 + N * 7 + R)
        if k is None:
            X = (rng.normal(size=(2, M, 12)) @ rng.normal(size=(2, 12, N)) * 20 + rng.normal(size=(2, M, N)) * 5 + 100).astype(np.float32)
            X[1] = np.round(X[1])  # integer-valued: exact products, ties in the rounding
        else:  # rank k < R: the eigenvalues of the null space cluster, vectors from the Gram-Schmidt fallbacks
            X = (rng.integers(0, 16, (2, M, k)) @ rng.integers(0, 16, (2, k, N))).astype(np.float32)
        futures = [pool.submit(want_of, X[b], R) for b in range(2)]
        t0 = time.perf_counter()
        (U, V), ninit, nbcd = timed(ctx, lambda: ctx.decompose(torch.from_numpy(X).cuda(), R, LADDER_K, D[0], D[1]))
        pending.append((name, futures, U.cpu().numpy(), V.cpu().numpy(), ninit, nbcd, ctx_state(ctx), round(time.perf_counter() - t0, 3)))
    for name, futures, Uh, Vh, ninit, nbcd, state, gpu_s in pending:
        bad = []
        for b in range(2):
            wu, wv = futures[b].result()
            for fname, g_, w_ in (("U", Uh[b], wu), ("V", Vh[b], wv)):
                if not np.array_equal(g_, w_):
                    bad.append(diff_message(name, b, "integer" if b else "float", "-", fname, g_, w_))
        emit(section="ladder", case=name, init=ninit, bcd=nbcd, images=2, planes=2, nbad=len(bad), bad=bad[:8], ctx=state, gpu_s=gpu_s)


def section_general():
    import torch
    import lrf_amd
    from concurrent.futures import ThreadPoolExecutor
    from _persist_at_size_worker import ctx_state, emit
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    pool = ThreadPoolExecutor(max_workers=POOL)
    B, K = GENERAL_B, GENERAL_K
    pending = []
    for shape in GENERAL_SHAPES:
        M, N, R = shape
        rng = np.random.default_rng(M * 131 + N * 7 + R)
        X = (rng.random((B, M, N)) * 255).astype(np.float32)
        X[1] = np.round(X[1])
        U0 = (rng.normal(size=(B, M, R)) * 3).astype(np.float32)
        V0 = (rng.normal(size=(B, N, R)) * 3).astype(np.float32)
        if R > min(M, N):
            U0[:, :, min(M, N):] = 0
            V0[:, :, min(M, N):] = 0
        Xd, U0d, V0d = torch.from_numpy(X).cuda(), torch.from_numpy(U0).cuda(), torch.from_numpy(V0).cuda()
        opts = GENERAL_OPTS + ([("factor uvw", dict(bounds=D, factor=(0, 1, 2)))] if shape == GENERAL_W_SHAPE else [])
        for oname, kw in opts:
            futures = [pool.submit(oracle.bcd_ex, X[b], U0[b], V0[b], K, **kw) for b in range(B)]
            (U, V, W), ninit, nbcd = timed(ctx, lambda: ctx.decompose_ex(Xd, R, K, init=(U0d, V0d), **kw))
            pending.append((general_name(shape, oname), 2 in kw["factor"], futures, U.cpu().numpy(), V.cpu().numpy(), W.cpu().numpy(), ninit, nbcd,
                            ctx_state(ctx)))
    for name, with_w, futures, Uh, Vh, Wh, ninit, nbcd, state in pending:
        bad, extra = [], {}
        for b in range(B):
            uo, vo, wo = futures[b].result()
            if with_w:  # the two judgements of test_hip_general_bcd that need no fixture
                extra.setdefault("w_close", []).append(bool(np.allclose(Wh[b], wo, rtol=1e-5, atol=1e-4)))
                extra.setdefault("u_same", []).append(float(np.mean(Uh[b] == uo)))
                extra.setdefault("v_same", []).append(float(np.mean(Vh[b] == vo)))
                continue
            for fname, g_, w_ in (("U", Uh[b], uo), ("V", Vh[b], vo), ("W", Wh[b], wo)):
                m = bits_differ(name, b, "integer" if b == 1 else "float", "-", fname, g_, w_)
                if m:
                    bad.append(m)
        emit(section="general", case=name, init=ninit, bcd=nbcd, images=B, planes=B, nbad=len(bad), bad=bad[:8], ctx=state, **extra)


SECTIONS = {"batches": section_batches, "chunked": section_chunked, "ladder": section_ladder, "general": section_general}

if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, ".."))
    sys.path.insert(0, here)
    from oracle import oracle as _o
    _o.build()
    t_start = time.perf_counter()
    SECTIONS[sys.argv[1]]()
    print(f"DONE {sys.argv[1]} {time.perf_counter() - t_start:.1f} s", flush=True)
