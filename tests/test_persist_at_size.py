"""GPU suite (-m gpu): the persistent iteration kernel k_bcd_p (lrf_bcdp_kernel.hip; which calls take it: plan_bcd,
lrf_plan.cpp) where it ships — on the default thresholds, at production batch sizes — against the CPU oracle, EVERY
image of every batch bit for bit.  A wrong hand-off inside the launch gives silently stale factors which the poll-expiry
error word does not see; only this comparison does.

The GPU work runs in child processes (tests/_persist_at_size_worker.py, one per group of sections, started once per module
run): the LRF_PERSIST switch and the threshold hooks are read once per process, and the children's environment has them
REMOVED, so that what runs is what a user gets.  The parent never initialises HIP.  Every case asserts
  (a) the path, from the context's kernel timers: the number of LRF_K_BCD_PERSIST launches and of LRF_K_BCD regions (0: the
      first iteration inside the launch; 1: outside; K: no persistent launch) — the tables in the worker give, per case, what
      plan_bcd says on reading and the k_bcd_p instantiation <F16, NP32, FIRST> that makes it; all twelve occur;
  (b) int8 U and V of every image equal the oracle's (np.array_equal; a failure names case, image, plane, count and first
      index of the differing entries);
  (c) ctx.synchronize() / ctx.check() raise nothing afterwards.
After a child that timed out or did not exit cleanly nothing further is started on the GPU by this module.

Measured on an MI355X box (16 usable cores): see profiles/README.md, "tests/test_persist_at_size.py"."""
import json
import os
import subprocess
import sys

import pytest

import _persist_at_size_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS = ("LRF_PERSIST", "LRF_BCDW16_MIN_BLOCKS", "LRF_BCDW32_MIN_BLOCKS", "LRF_FAMILY_SPLIT_BLOCKS", "LRF_FUSED_GRAM_MIN_CHUNKS")
# seconds: about three times a child's measured run (shared machines; the oracle pool competes for the 16 cores)
TIMEOUT = {"batches": 60,  # measured 17.5 s (14 s of them in the oracle pool)
           "shapes": 20,   # measured 5.7 s
           "caller": 20,   # measured 6.7 s
           "sweep": 15}    # measured 3.9 s
_stopped = []  # why nothing more is started on the GPU
_cache = {}


def _child(section):
    """the RESULT lines of one child, by case name; run once per module run"""
    if section in _cache:
        return _cache[section]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_persist_at_size_worker.py"), section], env=env, capture_output=True,
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
            out[(d["section"], d["case"])] = d
    assert f"DONE {section}" in r.stdout, r.stdout[-2000:]
    _cache[section] = out
    return out


def _check(d, path, images, planes=None):
    assert (d["persist"], d["bcd"]) == tuple(path), f"{d['case']}: (persistent launches, LRF_K_BCD regions) = {(d['persist'], d['bcd'])}, expected {tuple(path)}"
    assert d["images"] == images and d["planes"] == (3 * images if planes is None else planes), (d["case"], d["images"], d["planes"])
    assert d["nbad"] == 0, f"{d['nbad']} factor matrices differ from the oracle's:\n" + "\n".join(d["bad"])
    assert d["ctx"] == "", (d["case"], d["ctx"])


@pytest.mark.parametrize("ranks, bounds, K, path", [c[:4] for c in W.BATCH_CASES], ids=[W.case_name(*c[:3]) for c in W.BATCH_CASES])
def test_production_batch_256_images_every_image_equals_oracle(ranks, bounds, K, path):
    """256 x 512x768 (6144 blocks x K iterations: the queue refills all the time, a wave takes items whose inputs another wave
    has just handed off) on the default thresholds: ranks <= 8, 9..16, every pair count 9..16 of ranks 17..32, mixes of three
    families, bounds inside and outside the exact-integer range, K = 10, 2 and 1."""
    _check(_child("batches")[("batches", W.case_name(ranks, bounds, K))], path, W.BATCH[0])


@pytest.mark.parametrize("ranks, below, at", W.THRESHOLD_CASES, ids=[str(c[0]) for c in W.THRESHOLD_CASES])
def test_thresholds_of_bcdp_plan_straddled(ranks, below, at):
    """2304 blocks for one rank family, 3584 for mixed ones (lrf_host.h), 24 blocks an image: one image fewer iterates on the
    launch-per-iteration kernels, the threshold batch in one persistent launch; the common images get the same factors on
    both sides, and all of them the oracle's."""
    res = _child("batches")
    _check(res[("thresholds", W.case_name(ranks, W.D, 10) + f" B={below}")], (0, 10), below)
    _check(res[("thresholds", W.case_name(ranks, W.D, 10) + f" B={at}")], (1, 0), at)
    assert res[("thresholds", W.case_name(ranks, W.D, 10) + " flip")]["same"], "the common images' factors differ across the threshold"


@pytest.mark.parametrize("ranks", W.REPEAT_CASES, ids=[str(c) for c in W.REPEAT_CASES])
def test_repeat_runs_of_the_higher_rank_families(ranks):
    """20 further 256-image calls into the same output tensors with unrelated work on the device between some of them, each
    equal to the first (which the test above compared with the oracle).  A determinism check on code that passes: not to be
    grown or re-run to chase a failure."""
    d = _child("batches")[("repeats", W.case_name(ranks, W.D, 10))]
    assert d["differ_at"] == -1, f"run {d['differ_at']} of {d['runs']} differs from the first in {d['differ_images']} images"
    assert d["runs"] == W.REPEATS and d["ctx"] == "", d


@pytest.mark.parametrize("geom, ranks, bounds, K, path", [(g,) + c[:4] for g, cases in W.SHAPE_CASES for c in cases],
                         ids=[f"{g[0]}x{g[1]}x{g[2]} {c[0]}" for g, cases in W.SHAPE_CASES for c in cases])
def test_other_geometries_every_image_equals_oracle(geom, ranks, bounds, K, path):
    """32 images of 1365x2048 (odd height, reflect padding, 172 blocks an image) and 1000 ragged 173x264 ones (4 blocks each, a
    partial last sub-tile, plane offsets in U that are no multiples of 16), defaults."""
    B, H, W_ = geom
    _check(_child("shapes")[("shapes", W.case_name(ranks, bounds, K) + f" {B}x{H}x{W_}")], path, B)


@pytest.mark.parametrize("kind, M, R, K", [("bcd",) + c for c in W.CALLER_BCD] + [("decompose",) + c for c in W.CALLER_DECOMPOSE])
def test_caller_given_initial_factors_and_uniform_tables(kind, M, R, K):
    """Context.bcd (the old U of the first iteration comes from the caller: the first iteration stays outside the launch —
    k_bcd_p<false,0,false> at ranks <= 8, <true,0,false> at 9..16, <true,12,false> at 24) and Context.decompose (uniform
    tables) on 160 luma patch matrices [M, 64] of real planes, M a multiple of 384 and not: against oracle.bcd from the same
    initial factors / oracle.qmf_decompose, every matrix."""
    _check(_child("caller")[("caller", f"{kind} M={M} R={R} K={K}")], W.caller_path(kind, R), W.CALLER_B, planes=W.CALLER_B)


@pytest.mark.parametrize("qualities, path", [c[:2] for c in W.SWEEP_CASES], ids=[f"q{c[0][0]}..{c[0][-1]}" for c in W.SWEEP_CASES])
def test_fused_sweep_every_image_and_rank_triple_equals_oracle(qualities, path):
    """qmf_encode_sweep on BASELINE config 3's 24 images: every stream parsed, the factors of every (image, distinct rank
    triple) pair against the oracle.  Qualities 1..32 hold luma ranks 17..20 — two pair counts in one run, which plan_bcd
    declines: the launch-per-iteration kernels; qualities 1..25 (ranks <= 16) iterate in one persistent launch."""
    d = _child("sweep")[("sweep", f"sweep q={qualities[0]}..{qualities[-1]}")]
    _check(d, path, 24, planes=3 * d["pairs"])
    assert d["pairs"] == 24 * d["triples"] and d["triples"] >= (18 if qualities[-1] == 32 else 14), d


def test_all_twelve_instantiations_of_the_persistent_kernel_are_covered():
    """the tables above name the k_bcd_p instantiation of every case that expects a persistent launch: all twelve occur"""
    seen = {c[4] for c in W.BATCH_CASES} | {c[4] for _, cases in W.SHAPE_CASES for c in cases} | {c[2] for c in W.SWEEP_CASES}
    seen |= {W.caller_inst("bcd", R) for _, R, _ in W.CALLER_BCD} | {W.caller_inst("decompose", R) for _, R, _ in W.CALLER_DECOMPOSE}
    want = {"<false,0,true>", "<false,0,false>", "<true,0,true>", "<true,0,false>"} | {f"<true,{n},false>" for n in range(9, 17)}
    assert want <= seen, sorted(want - seen)
