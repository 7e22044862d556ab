"""GPU suite (-m gpu): k_bcd_p's rank <= 8 block body computes a = x V (first iteration: and X W0) and a' += X^T u on 4x4x1 MFMA
blocks by rank quad (lrf_bcdp_kernel.hip: row_times_quads, xt_u_quads; one quad at R <= 4, two at R = 5..8).  Every element stays
one k-ordered chain of single fmas, so the int8 factors must not change by a bit: every image of every case is compared with
  * the launch-per-iteration kernels (LRF_PERSIST=0: k_bcd_w's VALU chain and 16-wide tiles, the independent on-GPU reference), and
  * the CPU oracle,
on two small geometries (partial sub-tiles, unaligned U spans; a single sub-tile with few live rows), at rank triples on both
sides of the 4 / 5 boundary, with a padded last quad, and mixed so that a wave alternates between one-quad and two-quad items.

The GPU work runs in child processes (tests/_bcdp_quads_worker.py: the LRF_PERSIST switch is read once per process), one per
(geometry, setting), started once per module run, each under its own timeout.  After a child that timed out or did not exit
cleanly nothing further is started on the GPU by this module.  The parent never initialises HIP."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _bcdp_quads_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120  # seconds per child (25 small calls and the start of the process: a few seconds)
POOL = 16      # oracle threads: a fixed number, never os.cpu_count()
_stopped = []  # why nothing more is started on the GPU
_children = {}
_oracle_done = {}
_planes = {}


def _child(geom, persist, tmp_path_factory):
    """the arrays one child saved; run once per module run"""
    key = (geom, persist)
    if key in _children:
        return _children[key]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = dict(os.environ)
    env["LRF_PERSIST"] = persist
    out = str(tmp_path_factory.mktemp("bcdp_quads") / f"{geom}_{persist}.npz")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_bcdp_quads_worker.py"), geom, out], env=env, capture_output=True,
                           text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the ({geom}, LRF_PERSIST={persist}) child did not finish in {TIMEOUT} s")
        pytest.fail(f"{_stopped[0]}: {str(e.stdout)[-2000:]}")
    if r.returncode != 0:
        _stopped.append(f"the ({geom}, LRF_PERSIST={persist}) child exited with {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"DONE {geom}" in r.stdout, r.stdout[-2000:]
    with np.load(out) as z:
        _children[key] = {k: z[k] for k in z.files}
    return _children[key]


def _diff(case, ref, b, plane, name, got, want):
    if got.shape != want.shape:
        return f"{case} against {ref}: image {b} plane {plane} {name}: shape {got.shape} against {want.shape}"
    ne = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return (f"{case} against {ref}: image {b} plane {plane} {name}: {ne.size} of {got.size} entries differ, first at "
            f"{tuple(int(i) for i in np.unravel_index(ne[0], got.shape))}")


def _oracle_factors(oracle, geom, images, ranks, bounds, K):
    """the oracle's int8 (u, v) per (image, plane); kept per (geometry, plane, rank, K, bounds): triples share plane ranks"""
    if geom not in _planes:
        with ThreadPoolExecutor(max_workers=POOL) as pool:
            _planes[geom] = list(pool.map(oracle.rgb_to_planes, list(images)))
    X = _planes[geom]

    def one(key):
        _, b, c, R, k, bd = key
        u, v = oracle.qmf_decompose(X[b][c], R, k, bd)
        return key, (u.astype(np.int8), v.astype(np.int8))

    keys = [(geom, b, c, ranks[c], K, tuple(bounds)) for b in range(len(X)) for c in range(3)]
    todo = sorted({k for k in keys if k not in _oracle_done})
    with ThreadPoolExecutor(max_workers=POOL) as pool:
        _oracle_done.update(pool.map(one, todo))
    return [[_oracle_done[(geom, b, c, ranks[c], K, tuple(bounds))] for c in range(3)] for b in range(len(X))]


@pytest.mark.parametrize("ranks, bounds, K", W.CASES, ids=[W.case_name(*c) for c in W.CASES])
@pytest.mark.parametrize("geom", sorted(W.GEOMS))
def test_quad_body_bit_equal_to_launch_per_iteration_and_oracle(geom, ranks, bounds, K, tmp_path_factory, oracle):
    from lrf_amd.codec import split_factors
    got = _child(geom, "1", tmp_path_factory)
    ref = _child(geom, "0", tmp_path_factory)
    i = W.CASES.index((ranks, bounds, K))
    case = f"{geom} {W.case_name(ranks, bounds, K)}"
    H, Wd, min_blocks = W.GEOMS[geom]
    B = got["images"].shape[0]
    assert B == W.batch_size(H, Wd, min_blocks) and np.array_equal(got["images"], ref["images"]), case
    # the path: one persistent launch where plan_bcd gives one (K >= 2, from 1024 blocks under LRF_PERSIST=1), none in the reference
    assert int(got[f"launches{i}"]) == W.expected_launches(K), (case, int(got[f"launches{i}"]))
    assert int(ref[f"launches{i}"]) == 0, (case, int(ref[f"launches{i}"]))
    Ug, Vg, Ur, Vr = got[f"U{i}"], got[f"V{i}"], ref[f"U{i}"], ref[f"V{i}"]
    want = _oracle_factors(oracle, geom, got["images"], ranks, bounds, K)
    bad = []
    for b in range(B):
        fg = split_factors(Ug[b], Vg[b], (H, Wd), ranks)
        fr = split_factors(Ur[b], Vr[b], (H, Wd), ranks)
        for c in range(3):
            plane = "Y Cb Cr".split()[c]
            for name, g_, r_, o_ in (("U", fg[2 * c], fr[2 * c], want[b][c][0]), ("V", fg[2 * c + 1], fr[2 * c + 1], want[b][c][1])):
                if not np.array_equal(g_, r_):
                    bad.append(_diff(case, "LRF_PERSIST=0", b, plane, name, g_, r_))
                if g_.shape != o_.shape or not np.array_equal(g_, o_):
                    bad.append(_diff(case, "the oracle", b, plane, name, g_, o_))
    assert not bad, f"{len(bad)} factor matrices differ:\n" + "\n".join(bad[:8])
