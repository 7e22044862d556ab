"""Child process of tests/test_persist_at_size.py: the persistent iteration kernel k_bcd_p on the thresholds a user gets (the
parent removes LRF_PERSIST and the other threshold hooks from the environment; the switch is read once per process), every
image of every batch against the CPU oracle.  `python _persist_at_size_worker.py <section>` runs one section on the GPU and
prints one "RESULT {json}" line per case: the kernel timers' counts (LRF_K_BCD_PERSIST launches, LRF_K_BCD regions), how many
images and planes were compared, the differing ones, and what ctx.synchronize() / ctx.check() said afterwards.  The parent
asserts; this file only reports (so that it can be run by hand with LRF_PERSIST=0 to see which side of a mismatch is wrong).

The case tables are at the top and import nothing heavy: the test module reads them at collection time."""
import json
import os
import sys
import time

import numpy as np

POOL = 16  # oracle threads: a fixed number, never os.cpu_count() (shared hosts grant a job far fewer cores than they have)
D = (-16, 15)

# ---- section 1: 256 x 512x768 -------------------------------------------------------------------------------------------
# (ranks, bounds, K, (persistent launches, LRF_K_BCD regions), the k_bcd_p instantiation <F16, NP32, FIRST> it runs)
# regions: 0 = the first iteration inside the launch (BcdPlan::persist_first: ranks <= 16), 1 = outside (a rank above 16),
# K = no persistent launch (every iteration is a region).  (22,11,11), (28,14,14), (30,15,15): the pair counts 11, 14, 15.
BATCH = (256, 512, 768)
BATCH_CASES = [
    ((4, 2, 2), D, 10, (1, 0), "<false,0,true>"), ((7, 3, 3), D, 10, (1, 0), "<false,0,true>"), ((8, 8, 8), D, 10, (1, 0), "<false,0,true>"),
    ((10, 5, 5), D, 10, (1, 0), "<true,0,true>"), ((16, 8, 8), D, 10, (1, 0), "<true,0,true>"), ((12, 12, 12), D, 10, (1, 0), "<true,0,true>"),
    ((20, 10, 10), D, 10, (1, 1), "<true,10,false>"), ((26, 13, 13), D, 10, (1, 1), "<true,13,false>"),
    ((32, 16, 16), D, 10, (1, 1), "<true,16,false>"), ((24, 12, 6), D, 10, (1, 1), "<true,12,false>"),
    ((17, 8, 8), D, 10, (1, 1), "<true,9,false>"), ((22, 11, 11), D, 10, (1, 1), "<true,11,false>"),
    ((28, 14, 14), D, 10, (1, 1), "<true,14,false>"), ((30, 15, 15), D, 10, (1, 1), "<true,15,false>"),
    ((16, 8, 8), (-8, 7), 10, (1, 0), "<true,0,true>"), ((16, 8, 8), (-22, 22), 10, (1, 0), "<true,0,true>"),
    # (R - 1) 64 mx^3 < 2^24 fails: 15 * 64 * 32^3 and 25 * 64 * 25^3 — the launch-per-iteration kernels take the call
    ((16, 8, 8), (-32, 31), 10, (0, 10), None), ((26, 13, 13), (-25, 25), 10, (0, 10), None),
    # two iterations / a single iteration inside the launch; K < 2: no persistent launch
    ((16, 8, 8), D, 2, (1, 0), "<true,0,true>"), ((26, 13, 13), D, 2, (1, 1), "<true,13,false>"), ((7, 3, 3), D, 1, (0, 1), None),
]
# ---- section 4: the two thresholds of plan_bcd straddled (24 blocks an image): prefixes of section 1's batch
# (ranks, images below, images at the threshold)
THRESHOLD_CASES = [((7, 3, 3), 95, 96), ((12, 12, 12), 95, 96), ((16, 8, 8), 149, 150)]
# ---- section 5: repeat runs next to other GPU work
REPEAT_CASES = [(16, 8, 8), (26, 13, 13)]
REPEATS = 20
# ---- section 2: other geometries ((B, H, W), [(ranks, bounds, K, path, instantiation)])
SHAPE_CASES = [
    ((32, 1365, 2048), [((16, 8, 8), D, 10, (1, 0), "<true,0,true>"), ((26, 13, 13), D, 10, (1, 1), "<true,13,false>")]),
    ((1000, 173, 264), [((3, 2, 1), D, 10, (1, 0), "<false,0,true>"), ((13, 6, 9), D, 10, (1, 0), "<true,0,true>"),
                        ((18, 9, 4), D, 10, (1, 1), "<true,9,false>")]),
]
# ---- section 3: caller-given initial factors (Context.bcd: first_mode 2, never inside the launch) and Context.decompose on
# uniform tables; 160 luma patch matrices of 16 blocks = 2560 blocks, one rank family: above 2304
CALLER_B = 160
CALLER_BCD = [(M, R, K) for M in (6144, 6000) for R in (3, 8, 12, 16, 24) for K in (2, 10)]
CALLER_DECOMPOSE = [(6144, R, 10) for R in (3, 8, 12, 16, 24)] + [(6000, R, 2) for R in (3, 8, 12, 16, 24)]


def caller_path(kind, R):
    return (1, 1) if kind == "bcd" or R > 16 else (1, 0)


def caller_inst(kind, R):
    first = "false" if kind == "bcd" or R > 16 else "true"
    return f"<{'false' if R <= 8 else 'true'},{(R + 1) // 2 if R > 16 else 0},{first}>"


# ---- section 6: the fused sweep on BASELINE config 3's 24 images.  Qualities 1..32 give luma ranks 17, 18, 19 and 20 in one
# run of planes: two pair counts (9 and 10), which plan_bcd declines (one NP32 per launch) — ten launch-per-iteration rounds;
# qualities 1..25 stop at rank 16: one persistent launch with the first iteration inside.
SWEEP_CASES = [(list(range(1, 33)), (0, 10), None), (list(range(1, 26)), (1, 0), "<true,0,true>")]


def case_name(ranks, bounds, K):
    return f"{tuple(ranks)} {tuple(bounds)} K={K}"


# ---------------------------------------------------------------------------------------------------------------------------
def emit(**kw):
    print("RESULT " + json.dumps(kw), flush=True)


def build_images(B, H, W, seed):
    """uint8 CUDA [B,3,H,W] and a label per image.  A mix, so that no case passes because the data is easy: smooth plus noise
    (tests/_persist_worker.py's recipe), uniform noise, shifted crops (tiles, where the image is larger) of the natural
    fixture, and at fixed places, the first and the last of the batch among them, an all-zero image, a constant one and one
    whose left half is zero."""
    import torch
    from conftest import config3_image
    g = torch.Generator(device="cuda").manual_seed(seed)
    imgs = torch.empty((B, 3, H, W), dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 27) // (3 * H * W))
    for b0 in range(0, B, step):  # in chunks: the fp32 temporaries of a whole batch would be four times the batch
        n = min(step, B - b0)
        base = torch.rand((n, 3, max(H // 8, 1), max(W // 8, 1)), device="cuda", generator=g) * 255
        sm = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
        imgs[b0:b0 + n] = (sm + torch.randn(sm.shape, device="cuda", generator=g) * 6).clamp(0, 255).to(torch.uint8)
    kinds = ["smooth"] * B
    nat = [config3_image(i).cuda() for i in range(20, 24)]
    for b in range(2, B, 4):
        imgs[b] = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda", generator=g)
        kinds[b] = "noise"
    for b in range(3, B, 4):
        src = torch.roll(nat[(b // 4) % 4], shifts=((b * 37) % 512, (b * 53) % 768), dims=(1, 2))
        src = src.repeat(1, (H + 511) // 512, (W + 767) // 768)
        imgs[b] = src[:, :H, :W]
        kinds[b] = "natural"
    for b, kind in ((0, "zero"), (1, "half-zero"), (B // 2, "zero"), (B // 2 + 1, "constant"), (B - 2, "half-zero"), (B - 1, "constant")):
        if kind == "zero":
            imgs[b] = 0
        elif kind == "constant":
            imgs[b] = 77 + b % 100
        else:
            imgs[b, :, :, :W // 2] = 0
        kinds[b] = kind
    return imgs, kinds


def diff_message(case, b, kind, plane, name, got, want):
    ne = np.flatnonzero(got.reshape(-1) != want.reshape(-1)) if got.shape == want.shape else None
    if ne is None:
        return f"{case}: image {b} ({kind}) plane {plane} {name}: shape {got.shape} against the oracle's {want.shape}"
    return (f"{case}: image {b} ({kind}) plane {plane} {name}: {ne.size} of {got.size} entries differ, first at "
            f"{tuple(int(i) for i in np.unravel_index(ne[0], got.shape))}")


class Bank:
    """The oracle's int8 factors of the planes of a set of images, computed on a pool and kept: rank triples share chroma
    ranks, the threshold and repeat sections share whole cases with section 1."""

    def __init__(self, oracle, host_imgs):
        from concurrent.futures import ThreadPoolExecutor
        self.oracle, self.imgs = oracle, host_imgs
        self.pool = ThreadPoolExecutor(max_workers=POOL)
        self.X = {}
        self.done = {}
        self.seconds = 0.0

    def _planes(self, b):
        self.X[b] = self.oracle.rgb_to_planes(self.imgs[b])

    def _one(self, key):
        b, c, R, K, bounds = key
        u, v = self.oracle.qmf_decompose(self.X[b][c], R, K, bounds)
        self.done[key] = (u.astype(np.int8), v.astype(np.int8))

    def fill(self, images, ranks, K, bounds):
        t0 = time.perf_counter()
        list(self.pool.map(self._planes, [b for b in images if b not in self.X]))
        keys = [(b, c, ranks[c], K, tuple(bounds)) for b in images for c in range(3)]
        # the most expensive planes first (luma, high rank): the pool ends evenly
        todo = sorted({k for k in keys if k not in self.done}, key=lambda k: (-k[2] * (4 if k[1] == 0 else 1), k[0]))
        list(self.pool.map(self._one, todo))
        self.seconds += time.perf_counter() - t0
        return time.perf_counter() - t0

    def compare(self, case, kinds, images, ranks, K, bounds, Uh, Vh, hw):
        """every image of the call: (planes compared, messages of the differing ones)"""
        from lrf_amd.codec import split_factors
        self.fill(images, ranks, K, bounds)
        bad, n = [], 0
        for row, b in enumerate(images):
            got = split_factors(Uh[row], Vh[row], hw, ranks)
            for c in range(3):
                wu, wv = self.done[(b, c, ranks[c], K, tuple(bounds))]
                n += 1
                for name, g_, w_ in (("U", got[2 * c], wu), ("V", got[2 * c + 1], wv)):
                    if g_.shape != w_.shape or not np.array_equal(g_, w_):
                        bad.append(diff_message(case, b, kinds[b], "Y Cb Cr".split()[c], name, g_, w_))
        return n, bad


def timed_call(ctx, fn):
    """fn() with the two kernel timers on: (result, persistent launches, LRF_K_BCD regions)"""
    import torch
    from lrf_amd import _lib
    ctx.profile_kernels([_lib.LRF_K_BCD, _lib.LRF_K_BCD_PERSIST])
    ctx.profile_reset()
    out = fn()
    torch.cuda.synchronize()
    npersist = ctx.kernel_time(_lib.LRF_K_BCD_PERSIST)[1]
    nbcd = ctx.kernel_time(_lib.LRF_K_BCD)[1]
    ctx.profile(False)
    return out, npersist, nbcd


def ctx_state(ctx):
    """what ctx.synchronize() and ctx.check() raise after a case (the poll-expiry word of k_bcd_p): '' when nothing"""
    try:
        ctx.synchronize()
        ctx.check()
        return ""
    except Exception as e:  # reported, asserted by the parent
        return f"{type(e).__name__}: {e}"


def encode_case(section, ctx, bank, imgs, kinds, images, ranks, bounds, K, hw, keep=False, tag=""):
    import lrf_amd
    case = case_name(ranks, bounds, K) + tag
    sub = imgs if len(images) == imgs.shape[0] else imgs[:len(images)]
    t0 = time.perf_counter()
    (U, V), npersist, nbcd = timed_call(ctx, lambda: lrf_amd.qmf_factorize_batch(sub, ranks, num_iters=K, bounds=bounds))
    Uh, Vh = U.cpu().numpy(), V.cpu().numpy()
    t1 = time.perf_counter()
    n, bad = bank.compare(case, kinds, images, ranks, K, bounds, Uh, Vh, hw)
    emit(section=section, case=case, persist=npersist, bcd=nbcd, images=len(images), planes=n, nbad=len(bad), bad=bad[:8],
         ctx=ctx_state(ctx), gpu_s=round(t1 - t0, 3), oracle_s=round(time.perf_counter() - t1, 3))
    return (U, V, Uh, Vh) if keep else None


def section_batches():
    """sections 1, 4 and 5: they share the 256 images and the oracle's factors of them"""
    import torch
    import lrf_amd
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    B, H, W = BATCH
    imgs, kinds = build_images(B, H, W, 17)
    bank = Bank(oracle, imgs.cpu().numpy())
    everyone = list(range(B))
    kept = {}
    for ranks, bounds, K, _, _ in BATCH_CASES:
        keep = K == 10 and tuple(bounds) == D and ranks in REPEAT_CASES
        r = encode_case("batches", ctx, bank, imgs, kinds, everyone, ranks, bounds, K, (H, W), keep=keep)
        if keep:
            kept[ranks] = r
    # section 4: n images below / at the threshold; the images are section 1's first ones, so are the oracle's factors
    for ranks, below, at in THRESHOLD_CASES:
        got = {}
        for n in (below, at):
            got[n] = encode_case("thresholds", ctx, bank, imgs, kinds, list(range(n)), ranks, D, 10, (H, W), keep=True, tag=f" B={n}")
        same = bool(np.array_equal(got[below][2], got[at][2][:below]) and np.array_equal(got[below][3], got[at][3][:below]))
        emit(section="thresholds", case=case_name(ranks, D, 10) + " flip", same=same)
        del got
    # section 5: 20 further calls into the same output tensors next to unrelated work on the device, each against the first
    # (oracle-checked above); stops at the first difference
    other = torch.empty((64, 1024, 1024), device="cuda")
    for ranks in REPEAT_CASES:
        U0, V0 = kept[ranks][0], kept[ranks][1]
        U, V = torch.empty_like(U0), torch.empty_like(V0)
        differ_at, differ_images = -1, 0
        for i in range(REPEATS):
            if i % 3 == 1:
                other.normal_()  # uneven load next to the launch
            lrf_amd.qmf_factorize_batch(imgs, ranks, out=(U, V))
            if i % 3 == 2:
                other.mul_(1.0001)
            if not (torch.equal(U, U0) and torch.equal(V, V0)):
                differ_at = i
                differ_images = int(((U != U0).any(dim=1) | (V != V0).any(dim=1)).sum())
                break
        emit(section="repeats", case=case_name(ranks, D, 10), runs=REPEATS, differ_at=differ_at, differ_images=differ_images, ctx=ctx_state(ctx))
    print(f"oracle seconds (16 threads) {bank.seconds:.1f}", flush=True)


def section_shapes():
    import torch
    import lrf_amd
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    for (B, H, W), cases in SHAPE_CASES:
        imgs, kinds = build_images(B, H, W, 100 + H)
        bank = Bank(oracle, imgs.cpu().numpy())
        for ranks, bounds, K, _, _ in cases:
            encode_case("shapes", ctx, bank, imgs, kinds, list(range(B)), ranks, bounds, K, (H, W), tag=f" {B}x{H}x{W}")
        print(f"oracle seconds (16 threads) {B}x{H}x{W}: {bank.seconds:.1f}", flush=True)
        bank.pool.shutdown()
        del imgs, bank
        ctx.trim()
        torch.cuda.empty_cache()


def section_caller():
    import torch
    import lrf_amd
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    B = CALLER_B
    imgs, kinds = build_images(B, 512, 768, 31)
    P = ctx.planes_from_rgb(imgs)
    torch.cuda.synchronize()
    X6144 = P[:, :6144 * 64].reshape(B, 6144, 64).contiguous()  # the luma patch matrices (the first plane of an image's row)
    del P, imgs
    Xs = {6144: X6144, 6000: X6144[:, :6000].contiguous()}
    Xh = {M: x.cpu().numpy() for M, x in Xs.items()}
    pool = ThreadPoolExecutor(max_workers=POOL)

    def report(kind, M, R, K, U, V, npersist, nbcd, want_of, t0):
        case = f"{kind} M={M} R={R} K={K}"
        Uh, Vh = U.cpu().numpy(), V.cpu().numpy()
        t1 = time.perf_counter()
        want = list(pool.map(want_of, range(B)))
        bad = []
        for b in range(B):
            for name, g_, w_ in (("U", Uh[b], want[b][0].astype(np.int8)), ("V", Vh[b], want[b][1].astype(np.int8))):
                if not np.array_equal(g_, w_):
                    bad.append(diff_message(case, b, kinds[b], "Y", name, g_, w_))
        emit(section="caller", case=case, persist=npersist, bcd=nbcd, images=B, planes=B, nbad=len(bad), bad=bad[:8], ctx=ctx_state(ctx),
             gpu_s=round(t1 - t0, 3), oracle_s=round(time.perf_counter() - t1, 3))

    inits = {}
    for M, R, K in CALLER_BCD:
        X = Xs[M]
        if (M, R) not in inits:  # the library's initial factors rounded to halves: exact in fp32, and not the library's own
            U0, V0 = ctx.svd_init(X, R)
            U0, V0 = torch.round(U0 * 2) / 2, torch.round(V0 * 2) / 2
            inits = {(M, R): (U0, V0, U0.cpu().numpy(), V0.cpu().numpy())}
        U0, V0, U0h, V0h = inits[(M, R)]
        t0 = time.perf_counter()
        (U, V), npersist, nbcd = timed_call(ctx, lambda: ctx.bcd(X, U0, V0, K, -16, 15))
        report("bcd", M, R, K, U, V, npersist, nbcd, lambda b: oracle.bcd(Xh[M][b], U0h[b], V0h[b], K, D), t0)
    del inits
    for M, R, K in CALLER_DECOMPOSE:
        X = Xs[M]
        t0 = time.perf_counter()
        (U, V), npersist, nbcd = timed_call(ctx, lambda: ctx.decompose(X, R, K, -16, 15))
        report("decompose", M, R, K, U, V, npersist, nbcd, lambda b: oracle.qmf_decompose(Xh[M][b], R, K, D), t0)


def section_sweep():
    import torch
    import lrf_amd
    from concurrent.futures import ThreadPoolExecutor
    from conftest import config3_image
    from lrf_amd.codec import parse_stream
    from oracle import oracle
    ctx = lrf_amd._lib.context(0)
    imgs = torch.stack([config3_image(i) for i in range(24)])
    host = imgs.numpy()
    X = [oracle.rgb_to_planes(host[i]) for i in range(24)]
    pool = ThreadPoolExecutor(max_workers=POOL)
    done = {}

    def one(key):
        i, c, R = key
        u, v = oracle.qmf_decompose(X[i][c], R, 10, D)
        done[key] = (u.astype(np.int8), v.astype(np.int8))

    dev = imgs.cuda()
    for qualities, _, _ in SWEEP_CASES:
        case = f"sweep q={qualities[0]}..{qualities[-1]}"
        t0 = time.perf_counter()
        fused, npersist, nbcd = timed_call(ctx, lambda: lrf_amd.qmf_encode_sweep(dev, qualities=qualities))
        t1 = time.perf_counter()
        parsed = {}  # (image, rank triple) -> factors
        for streams in fused:
            for i, s in enumerate(streams):
                meta, fac = parse_stream(s)
                parsed.setdefault((i, tuple(meta["rank"])), fac)
        keys = sorted({(i, c, t[c]) for (i, t) in parsed for c in range(3)} - set(done), key=lambda k: -k[2] * (4 if k[1] == 0 else 1))
        list(pool.map(one, keys))
        bad = []
        for (i, t), fac in sorted(parsed.items()):
            for c in range(3):
                for name, g_, w_ in (("U", fac[2 * c], done[(i, c, t[c])][0]), ("V", fac[2 * c + 1], done[(i, c, t[c])][1])):
                    if g_.shape != w_.shape or not np.array_equal(g_, w_):
                        bad.append(diff_message(f"{case} ranks {t}", i, "config3", "Y Cb Cr".split()[c], name, np.asarray(g_), w_))
        emit(section="sweep", case=case, persist=npersist, bcd=nbcd, images=24, pairs=len(parsed), triples=len({t for _, t in parsed}),
             planes=3 * len(parsed), nbad=len(bad), bad=bad[:8], ctx=ctx_state(ctx), gpu_s=round(t1 - t0, 3), oracle_s=round(time.perf_counter() - t1, 3))


SECTIONS = {"batches": section_batches, "shapes": section_shapes, "caller": section_caller, "sweep": section_sweep}

if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, ".."))
    sys.path.insert(0, here)
    from oracle import oracle as _o
    _o.build()
    t_start = time.perf_counter()
    SECTIONS[sys.argv[1]]()
    print(f"DONE {sys.argv[1]} {time.perf_counter() - t_start:.1f} s", flush=True)
