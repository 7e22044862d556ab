"""CPU suite: the gates and conditions of the exact-integer BCD cases (tests/exact_bcd.py) that tests/test_exact_bcd_gpu.py runs
on the kernels.  The integer reference must equal the oracle and the reference's own recorded factors bit for bit — then a
mismatch on the GPU is the kernel's — and the table must really hold what it is for: dense rounding ties in both halves, zero
denominators, clamped values, and between its cases every U-update kernel a call with the caller's U0 can plan."""
import json
import os

import numpy as np
import pytest

import exact_bcd as E
from conftest import GOLDEN
from test_bcd_plan import FIRST_U0, K_W, K_W16, K_W32, K_W32F, MID, WG8, WG16, lib, plan  # noqa: F401 (lib: the fixture)

ALL = E.CASES + E.ANY_CASES
CUT = 4  # matrices of a large case the CPU gates look at


@pytest.fixture(scope="module")
def results():
    """reference_bcd of the first CUT matrices of every case, computed once: id -> (inputs, U, V, stats)"""
    out = {}
    for c in ALL:
        X, U0, V0 = c.inputs(CUT)
        out[c.id] = ((X, U0, V0),) + E.reference_bcd(X, U0, V0, c.K, c.lo, c.hi)
    return out


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_reference_equals_oracle(case, results, oracle):
    (X, U0, V0), U, V, _ = results[case.id]
    assert U.min() >= case.lo and U.max() <= case.hi and V.min() >= case.lo and V.max() <= case.hi
    for b in range(X.shape[0]):
        u, v = oracle.bcd(X[b], U0[b], V0[b], case.K, (case.lo, case.hi))
        assert np.array_equal(u, U[b].astype(np.float32)) and np.array_equal(v, V[b].astype(np.float32)), (case.id, b)


def test_reference_equals_the_recorded_factors_of_the_reference():
    """tests/golden/exact_bcd.npz (tools/gen_exact_bcd.py): QMF(...).solver on the ten smallest cases, whole"""
    z = np.load(os.path.join(GOLDEN, "exact_bcd.npz"))
    assert int(z["n"]) == len(E.GOLDEN_CASES) == 10
    for i, c in enumerate(E.GOLDEN_CASES):
        a = json.loads(str(z[f"args{i}"]))
        assert a == dict(id=c.id, seed=c.seed, B=c.B, M=c.M, N=c.N, R=c.R, K=c.K, lo=c.lo, hi=c.hi, gen=c.gen), "regenerate the fixture"
        X, U0, V0 = E.generate(a["seed"], a["B"], a["M"], a["N"], a["R"], a["lo"], a["hi"], **a["gen"])
        U, V, _ = E.reference_bcd(X, U0, V0, a["K"], a["lo"], a["hi"])
        assert np.array_equal(U, z[f"u{i}"]) and np.array_equal(V, z[f"v{i}"]), c.id


def test_reference_rounds_ties_to_even_and_divides_zero_by_zero_to_one():
    """by hand: x = [[1, 2]], v0 = [[1, 0], [1, 0]]: column 0 of u = 3 / 2 -> 2 (1.5 to even), then column 1 has b_11 = 0 and
    num = 0 - 2 * 0: (0 + eps) / (0 + eps) = 1; x = [[5, 0]]: 5 / 2 -> 2; x = [[-1, 0]]: -1 / 2 -> -0.  The clamp follows the
    round: 7 / 2 -> 4 -> 3 at hi = 3."""
    v0 = np.array([[[1, 0], [1, 0]]])
    for x, want in (([1, 2], [2, 1]), ([5, 0], [2, 1]), ([-1, 0], [0, 1]), ([7, 0], [3, 1]), ([-7, 0], [-3, 1])):
        u0 = np.zeros((1, 1, 2), np.int64)
        st = E.new_stats()
        u = E._half(np.array([[x]], np.float64), u0.astype(np.float64), v0.astype(np.float64), -3, 3, st["u"], False)
        assert u[0, 0].tolist() == want, (x, u)
        assert st["u"]["ties"] == 1 and st["u"]["zero_den"] == 1 and st["u"]["clamped"] == (abs(x[0]) == 7)


def test_reference_refuses_sums_that_reach_2_to_the_24():
    X = np.full((1, 384, 64), 700, np.int64)
    with pytest.raises(AssertionError, match="2\\^24"):
        E.reference_bcd(X, np.ones((1, 384, 2), np.int64), np.ones((1, 64, 2), np.int64), 1, -128, 127)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_tie_density_is_a_condition(case, results):
    st = results[case.id][3]
    assert case.K >= 3
    if case.R >= 2:
        assert E.share(st["u"]) >= 2.0, st["u"]
        if case.M > 1:  # (one row: after the first sweep the row solves its own least-squares problem, no ties left to meet)
            assert st["u"]["later_ties"] > 0, st["u"]
    if "v" in case.marks:
        assert E.share(st["v"]) >= 1.0, st["v"]
    if "z" in case.marks:
        assert st["u"]["zero_den"] + st["v"]["zero_den"] > 0
    if "c" in case.marks:
        assert st["u"]["clamped"] + st["v"]["clamped"] > 0


def test_marked_cases_cover_the_v_updates_of_every_family():
    """V-update coverage, zero denominators and clamps each occur at ranks <= 8, 9..16 and 17..32, in a persistent call too"""
    fam = lambda c: 0 if c.R <= 8 else 1 if c.R <= 16 else 2
    for mark in "vzc":
        assert {fam(c) for c in E.CASES if mark in c.marks} == {0, 1, 2}, mark
    assert {fam(c) for c in E.CASES if "v" in c.marks and c.blocks() >= 2304} == {0, 1, 2}


def test_table_takes_its_shapes_and_bounds_from_the_lists():
    assert {c.M for c in E.CASES} >= {384, 400, 130, 1, 17, 48}
    assert {(c.lo, c.hi) for c in E.CASES} >= {(-16, 15), (-3, 5), (-128, 127), (-32, 31), (-25, 25)}
    assert {c.gen["nz"] for c in E.CASES} >= {2, 4, 6, 10}
    assert all(c.N == 64 and c.R <= 32 for c in E.CASES)
    assert sorted((c.N, c.R <= 16) for c in E.ANY_CASES) == [(16, True), (64, False), (192, True)]
    assert len({c.id for c in ALL}) == len(ALL)


def planned(lib, c):
    head, runs = plan(lib, [(c.M, c.R)] * c.B, c.K, (c.lo, c.hi), FIRST_U0)
    assert len(runs) == 1 and head["nblocks"] == c.blocks() and not head["first"]
    return head, runs[0]


def test_table_covers_every_kernel_a_callers_u0_can_plan(lib):
    """plan_bcd with first_mode = the caller's U0 and default settings.  The later kernels of the table together are every
    BcdKernel enumerator but one: k_bcd_w32f is the first iteration of ranks 17..32 from old U = X W0 (wave_numbers_ok, mode 1),
    which no call of lrf_qmf_bcd_f32 reaches — asserted here over ranks, sizes and bounds, so that the day it becomes reachable
    this test asks for its case."""
    plans = [planned(lib, c) for c in E.CASES]
    assert {r["later_k"] for _, r in plans} == {WG8, WG16, MID, K_W, K_W16, K_W32}
    assert {r["first_k"] for _, r in plans} == {WG8, WG16, MID, K_W}
    for R in range(17, 33):
        for n in (1, 127, 128, 2304):
            for bounds in ((-16, 15), (-3, 5), (-128, 127)):
                _, runs = plan(lib, [(384, R)] * n, 3, bounds, FIRST_U0)
                assert K_W32F not in (runs[0]["first_k"], runs[0]["later_k"])
    # each wave kernel inside its own numbers and, for ranks above 8, one case outside them that falls back
    by = lambda k: [(c, h, r) for c, (h, r) in zip(E.CASES, plans) if r["later_k"] == k]
    assert any(r["exact_int"] for _, _, r in by(K_W16)) and any(c.blocks() >= 1024 and not r["exact_int"] for c, _, r in by(WG16))
    assert any(c.blocks() >= 128 and 64 * max(-c.lo, c.hi) ** 2 > 32767 for c, _, _ in by(MID))
    assert {r["later_arg"] for _, _, r in by(K_W32)} >= {9, 10, 11}  # an odd rank among them (17: NP = 9)
    # the persistent launch: ranks <= 8 alone, with the body of ranks 9..16, with the body of ranks 17..32
    persistent = [(h["f16"], h["np32"] > 0) for h, _ in plans if h["persist"]]
    assert (0, False) in persistent and (1, False) in persistent and (1, True) in persistent
    for c, (h, r) in zip(E.CASES, plans):
        assert bool(h["persist"]) == (c.blocks() >= 2304 and r["later_k"] in (K_W, K_W16, K_W32)), c.id
    # the thresholds are met by B at default settings
    assert min(c.blocks() for c, _, _ in by(K_W)) == 1024 and min(c.blocks() for c, _, _ in by(K_W16)) == 1024
    assert min(c.blocks() for c, _, _ in by(K_W32)) == 128


def test_docstring_lists_every_case_as_planned_and_measured(lib, results):
    """the table in tests/exact_bcd.py's docstring is the output of `python tests/exact_bcd.py`"""
    for c in ALL:
        st = results[c.id][3] if c.B <= CUT else E.reference_bcd(*c.inputs(E.DOC_CUT), c.K, c.lo, c.hi)[2]
        line = E.describe(c, *planned(lib, c), st) if c in E.CASES else E.describe(c, None, None, st)
        assert line.rstrip() in E.__doc__, line
