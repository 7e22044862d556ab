"""GPU suite (-m gpu): the rank <= 8 body of k_bcd_p<false, 0, true> reads the luma matrices of an eligible call from the caller's
image bytes instead of the fp32 workspace X (lrf_bcdp_kernel.hip: bcdp_w_block<MODE, true>; which calls: plan_luma_bytes,
lrf_plan.h).  The values are k_planes16's bit for bit and everything behind the operand is the fp32 body's, so the int8 factors
must not change by a bit: every image of every case is compared with the same call under LRF_LUMA_BYTES=0 (luma from X), and
every eighth image, the first (all zero) and the last (constant) with the CPU oracle, on three geometries chosen as the smallest
at which the row -> patch mapping can go wrong (tests/_luma_bytes_worker.py).  Every call must say through
lrf_ctx_last_luma_source which path it took: a silent fall-back fails.  The calls that must not take the path — sides that are
no multiples of 16, a tensor one byte off 8-alignment, the pipelined encoder — say "x" and give the same factors.

The GPU work runs in child processes (LRF_PERSIST and LRF_LUMA_BYTES are read once per process), one per (job, setting), started
once per module run, each under its own timeout.  After a child that timed out or did not exit cleanly nothing further is
started on the GPU by this module.  The parent never initialises HIP."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _luma_bytes_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120  # seconds per child (eleven small calls and the start of the process: a few seconds)
POOL = 16      # oracle threads: a fixed number, never os.cpu_count()
_stopped = []  # why nothing more is started on the GPU
_children = {}
_oracle_done = {}
_planes = {}


def _child(job, luma_bytes, tmp_path_factory):
    """the arrays one child saved; run once per module run"""
    key = (job, luma_bytes)
    if key in _children:
        return _children[key]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = dict(os.environ)
    env["LRF_PERSIST"] = "1"
    env["LRF_LUMA_BYTES"] = luma_bytes
    out = str(tmp_path_factory.mktemp("luma_bytes") / f"{job}_{luma_bytes}.npz")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_luma_bytes_worker.py"), job, out], env=env, capture_output=True, text=True,
                           timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the ({job}, LRF_LUMA_BYTES={luma_bytes}) child did not finish in {TIMEOUT} s")
        pytest.fail(f"{_stopped[0]}: {str(e.stdout)[-2000:]}")
    if r.returncode != 0:
        _stopped.append(f"the ({job}, LRF_LUMA_BYTES={luma_bytes}) child exited with {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"DONE {job}" in r.stdout, r.stdout[-2000:]
    with np.load(out) as z:
        _children[key] = {k: z[k] for k in z.files}
    return _children[key]


def _diff(case, ref, b, plane, name, got, want):
    if got.shape != want.shape:
        return f"{case} against {ref}: image {b} plane {plane} {name}: shape {got.shape} against {want.shape}"
    ne = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return (f"{case} against {ref}: image {b} plane {plane} {name}: {ne.size} of {got.size} entries differ, first at "
            f"{tuple(int(i) for i in np.unravel_index(ne[0], got.shape))}")


def _oracle_factors(oracle, geom, images, which, ranks, bounds, K):
    """the oracle's int8 (u, v) per plane of the images `which`; kept per (geometry, image, plane, rank, K, bounds)"""
    if geom not in _planes:
        with ThreadPoolExecutor(max_workers=POOL) as pool:
            _planes[geom] = dict(zip(which, pool.map(oracle.rgb_to_planes, [images[b] for b in which])))
    X = _planes[geom]

    def one(key):
        _, b, c, R, k, bd = key
        u, v = oracle.qmf_decompose(X[b][c], R, k, bd)
        return key, (u.astype(np.int8), v.astype(np.int8))

    keys = [(geom, b, c, ranks[c], K, tuple(bounds)) for b in which for c in range(3)]
    todo = sorted({k for k in keys if k not in _oracle_done})
    with ThreadPoolExecutor(max_workers=POOL) as pool:
        _oracle_done.update(pool.map(one, todo))
    return {b: [_oracle_done[(geom, b, c, ranks[c], K, tuple(bounds))] for c in range(3)] for b in which}


@pytest.mark.parametrize("ranks, bounds, K", W.CASES, ids=[W.case_name(*c) for c in W.CASES])
@pytest.mark.parametrize("geom", list(W.GEOMS))
def test_luma_from_bytes_bit_equal_to_luma_from_x_and_oracle(geom, ranks, bounds, K, tmp_path_factory, oracle):
    from lrf_amd.codec import split_factors
    got = _child(geom, "1", tmp_path_factory)
    ref = _child(geom, "0", tmp_path_factory)
    i = W.CASES.index((ranks, bounds, K))
    case = f"{geom} {W.case_name(ranks, bounds, K)}"
    H, Wd, min_blocks = W.GEOMS[geom]
    B = got["images"].shape[0]
    assert B == W.batch_size(H, Wd, min_blocks) and np.array_equal(got["images"], ref["images"]), case
    # the path: one persistent launch each, luma from the bytes in the one and from X in the other
    assert int(got[f"launches{i}"]) == 1 and int(ref[f"launches{i}"]) == 1, (case, int(got[f"launches{i}"]), int(ref[f"launches{i}"]))
    assert str(got[f"source{i}"]) == "bytes", (case, str(got[f"source{i}"]))
    assert str(ref[f"source{i}"]) == "x", (case, str(ref[f"source{i}"]))
    Ug, Vg, Ur, Vr = got[f"U{i}"], got[f"V{i}"], ref[f"U{i}"], ref[f"V{i}"]
    which = W.oracle_images(B)
    want = _oracle_factors(oracle, geom, got["images"], which, ranks, bounds, K)
    bad = []
    for b in range(B):
        fg = split_factors(Ug[b], Vg[b], (H, Wd), ranks)
        fr = split_factors(Ur[b], Vr[b], (H, Wd), ranks)
        for c in range(3):
            plane = "Y Cb Cr".split()[c]
            for j, name in ((2 * c, "U"), (2 * c + 1, "V")):
                if not np.array_equal(fg[j], fr[j]):
                    bad.append(_diff(case, "LRF_LUMA_BYTES=0", b, plane, name, fg[j], fr[j]))
                if b in want:
                    o_ = want[b][c][j & 1]
                    if fg[j].shape != o_.shape or not np.array_equal(fg[j], o_):
                        bad.append(_diff(case, "the oracle", b, plane, name, fg[j], o_))
    assert not bad, f"{len(bad)} factor matrices differ:\n" + "\n".join(bad[:8])


def test_calls_that_keep_luma_from_x(tmp_path_factory):
    got = _child("fallback", "1", tmp_path_factory)
    ref = _child("fallback", "0", tmp_path_factory)
    # sides that are no multiples of 16: the persistent launch, luma from X
    assert int(got["odd_launches"]) == 1 and str(got["odd_source"]) == "x"
    assert np.array_equal(got["odd_U"], ref["odd_U"]) and np.array_equal(got["odd_V"], ref["odd_V"])
    # the eligible call beside it takes the path (else the three comparisons below say nothing) ...
    assert int(got["al_launches"]) == 1 and str(got["al_source"]) == "bytes" and str(ref["al_source"]) == "x"
    assert np.array_equal(got["al_U"], ref["al_U"]) and np.array_equal(got["al_V"], ref["al_V"])
    # ... the same bytes one byte off 8-alignment do not
    assert int(got["off_launches"]) == 1 and str(got["off_source"]) == "x"
    assert np.array_equal(got["off_U"], got["al_U"]) and np.array_equal(got["off_V"], got["al_V"])
    # the pipelined encoder: the slots that encoded say "x", none says "bytes"
    sources = [str(s) for s in got["pipe_sources"]]
    assert "x" in sources and "bytes" not in sources, sources
    assert np.array_equal(got["pipe_U"], got["al_U"]) and np.array_equal(got["pipe_V"], got["al_V"])
