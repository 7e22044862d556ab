"""GPU suite (-m gpu): the any-shape kernels (lrf_anyshape_kernels.hip; which variant a call takes: plan_any_prod, plan_any_gs,
plan_any_init_chunk in lrf_plan.cpp) where they ship — 256 x 512x768 at patch sizes 4x4, 16x16, 32x32 and without patches —
and up to the largest rank (LRF_ANY_MAX_RANK = 639), against the CPU oracle, EVERY image and plane of every batch bit for
bit.  A wrong tile offset at several tiles per wave, or a wrong chunk offset in the initialisation, gives plausible but wrong
factors for some images of a large batch and nothing else; only this comparison sees it.  tests/test_any_plan.py (CPU) states
which kernel variants and loop counts each case here reaches, and that together they reach all of them.

The GPU work runs in child processes (tests/_anyshape_at_size_worker.py, one per section, started once per module run) whose
environment has the developer switches of this path and the hooks of the 64-column path REMOVED, so that what runs is what
a user gets.  The parent never initialises HIP.  Every case asserts
  (a) the number of LRF_K_INIT and LRF_K_BCD regions, from the context's kernel timers (one initialisation per call that
      initialises, K iteration regions per call);
  (b) the factors against the oracle's, with the number of compared images and planes (a failure names case, image, plane,
      factor, count and first index of the differing entries);
  (c) ctx.synchronize() / ctx.check() raise nothing afterwards.
After a child that timed out or did not exit cleanly nothing further is started on the GPU by this module.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import _anyshape_at_size_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS = ("LRF_ANY_PROD_SMALL", "LRF_ANY_GS_F32", "LRF_ANY_GRAM_VALU", "LRF_ANY_TRIDIAG_GLOBAL", "LRF_ANY_TRIDIAG_UNBLOCKED",
         "LRF_ANY_TRIDIAG_SQUARE", "LRF_PERSIST", "LRF_BCDW16_MIN_BLOCKS", "LRF_BCDW32_MIN_BLOCKS", "LRF_FAMILY_SPLIT_BLOCKS",
         "LRF_FUSED_GRAM_MIN_CHUNKS")
# seconds.  Bounds from the oracle's cost, which dominates every child (one thread, per image: 0.06 s at 4x4, 0.72 s at 16x16,
# 1.35 s at 32x32, 2.26 s without patches; 3.5 to 7 s per initialisation of side 1024; 8 s per matrix at rank 639), on a pool of
# 16 threads, times three for a shared machine
TIMEOUT = {"batches": 600,  # 256 x (0.06 * 3 + 0.72 + 1.35 + 2.26 + 0.2) + 32 x 1.35 + 48 x 0.1 = 1250 s / 16 = 80 s, plus the image sets
           "chunked": 600,  # 2 x 18 oracle initialisations = 190 s / 16, plus 2 x 254 single-matrix calls of side 1024 on the GPU
           "ladder": 300,   # 48 matrices x 2 .. 8 s = 250 s / 16
           "general": 120}  # 123 oracle runs of three iterations, the largest [1536, 256] at rank 51
_stopped = []  # why nothing more is started on the GPU
_cache = {}


def _child(section):
    """the RESULT lines of one child, by case name; run once per module run"""
    if section in _cache:
        return _cache[section]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_anyshape_at_size_worker.py"), section], env=env, capture_output=True,
                           text=True, timeout=TIMEOUT[section])
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the '{section}' child did not finish in {TIMEOUT[section]} s")
        pytest.fail(f"{_stopped[0]}: {str(e.stdout)[-2000:]}")
    if r.returncode != 0:
        _stopped.append(f"the '{section}' child exited with {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            d = json.loads(ln[7:])
            out[d["case"]] = d
    assert f"DONE {section}" in r.stdout, r.stdout[-2000:]
    print(f"\n'{section}' child: {time.perf_counter() - t0:.1f} s of {TIMEOUT[section]} s; seconds per case (GPU side, waiting for the oracle pool after it): "
          + ", ".join(f"{c} {d.get('gpu_s', '-')} / {d.get('oracle_wait_s', '-')}" for c, d in out.items()))
    _cache[section] = out
    return out


def _check(d, ninit, nbcd, images, planes):
    assert (d["init"], d["bcd"]) == (ninit, nbcd), f"{d['case']}: (LRF_K_INIT, LRF_K_BCD) regions = {(d['init'], d['bcd'])}, expected {(ninit, nbcd)}"
    assert (d["images"], d["planes"]) == (images, planes), (d["case"], d["images"], d["planes"])
    assert d["nbad"] == 0, f"{d['nbad']} factor matrices differ from the oracle's:\n" + "\n".join(d["bad"])
    assert d["ctx"] == "", (d["case"], d["ctx"])


@pytest.mark.parametrize("name, geom", [(c[0], c[1]) for c in W.BATCH_CASES], ids=[c[0] for c in W.BATCH_CASES])
def test_batch_every_image_and_plane_equals_oracle(name, geom):
    """The three per-plane calls of qmf_encode_batch(images, quality=..., patch_size=... / patch=False) at K = 10: int8 U and V
    of every image and plane np.array_equal to oracle.qmf_anyshape_decompose, no image left out; one initialisation and ten
    iteration regions per plane call."""
    _check(_child("batches")[name], 3, 3 * W.K_BATCH, geom[0], 3 * geom[0])


@pytest.mark.parametrize("orient", ["tall", "wide"])
def test_chunked_initialisation(orient):
    """Context.svd_init on 254 matrices of min side 1024 at rank 4 — two chunks of any_run_init, 253 and 1 matrices — with
    per-matrix signs in the tall orientation: bit patterns equal to oracle.svd_topr_any for the first and last matrix of each
    chunk and every 16th in between (the stated subset: the oracle's n = 1024 eigen-solve costs 3.5 to 7 s a matrix on one
    thread), and EVERY matrix equal, bit for bit, to the same matrix factorised alone."""
    d = _child("chunked")[orient]
    B, chunk = W.CHUNK["B"], W.CHUNK["chunk"]
    subset = W.chunk_subset(B, chunk)
    assert {0, chunk - 1, chunk, B - 1} <= set(subset) and len(subset) >= B // 16
    assert d["subset"] == subset
    _check(d, 1, 0, B, len(subset))
    assert d["alone"] == B and d["alone_bad"] == [], f"matrices that differ from the same matrix factorised alone: {d['alone_bad']}"


LADDER = [f"[{M}, {N}] R={R}" for M, N in W.LADDER_SHAPES for R in W.LADDER_RANKS] + [f"{n} [{M}, {N}] R={R}" for n, M, N, R, _ in W.LADDER_EXTRA]


@pytest.mark.parametrize("name", LADDER)
def test_rank_ladder_equals_oracle(name):
    """Context.decompose (the library's own initialisation, then K = 2) at ranks 121 .. 639 on [700, 660] and [660, 700], a wide
    [300, 2048] at rank 200 and matrices of rank 220 at rank 639, two matrices per call: int8 U and V equal to
    oracle.svd_topr_any + oracle.bcd.  629 / 630 straddle k_any_gs<float, true> / <float, false> (test_any_plan.py)."""
    _check(_child("ladder")[name], 1, W.LADDER_K, 2, 2)


@pytest.mark.parametrize("shape, opt", [(s, o[0]) for s in W.GENERAL_SHAPES for o in W.GENERAL_OPTS], ids=lambda v: str(v))
def test_general_solver_equals_oracle(shape, opt):
    """Context.decompose_ex from given initial factors (no initialisation region) against oracle.bcd_ex, three distinct matrices
    per call: U, V and W bit for bit, as test_hip_general_bcd requires wherever w is not updated."""
    _check(_child("general")[W.general_name(shape, opt)], 0, W.GENERAL_K, W.GENERAL_B, W.GENERAL_B)


def test_general_solver_with_w_updated():
    """factor=(0, 1, 2): judged as tests/test_qmf_class.py::test_hip_general_bcd judges it — W within rtol 1e-5 / atol 1e-4 of
    the oracle's, more than 99 % of the entries of U and of V equal."""
    d = _child("general")[W.general_name(W.GENERAL_W_SHAPE, "factor uvw")]
    _check(d, 0, W.GENERAL_K, W.GENERAL_B, W.GENERAL_B)
    assert len(d["w_close"]) == W.GENERAL_B and all(d["w_close"]), d
    assert min(d["u_same"]) > 0.99 and min(d["v_same"]) > 0.99, d
