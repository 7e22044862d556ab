"""CPU suite: the gates and conditions of the exact-integer cases of the general QMF solver (tests/exact_general.py) that
tests/test_exact_general_gpu.py runs on the kernels.  The integer restatement must equal the oracle and the reference's own
recorded factors bit for bit — then a mismatch on the GPU is the kernel's — and the table must really hold what it is for: rounding
ties, numerators on and inside the l1 threshold, zero denominators, clamps and values past +-127 in U halves and in V halves,
every option of the class, and between its cases every kernel variant the general path can plan (expected by hand, from the
thresholds tests/test_any_plan.py states, never from the plan)."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import exact_general as E
from conftest import GOLDEN
from test_any_plan import BIG, LONG, SHORT4, SHORT8, SHORT16, TILED, gs_kernel_by_hand, lib, update  # noqa: F401 (lib: the fixture)

F32 = np.float32


bits, check_w = E.bits, E.check_w


@pytest.fixture(scope="module")
def results():
    """reference_general of every case, computed once: id -> (inputs, U, V, W, stats)"""
    out = {}
    for c in E.ALL:
        inputs = c.inputs()
        out[c.id] = (inputs,) + E.reference_general(*inputs, c.K, c.opts)
    return out


@pytest.mark.parametrize("case", E.ALL, ids=lambda c: c.id)
def test_reference_equals_oracle(case, results, oracle):
    (X, U0, V0), U, V, W, _ = results[case.id]
    opts = dict(case.opts)
    w = opts.pop("w", (0.0, 1.0))
    for b in range(case.B):
        u, v, wo = oracle.bcd_ex(X[b], U0[b], V0[b], case.K, w=w, **opts)
        assert np.array_equal(bits(u), bits(U[b])) and np.array_equal(bits(v), bits(V[b])), (case.id, b)
        check_w(case, wo, W, b, "oracle")


def test_reference_equals_the_recorded_results_of_the_reference(results):
    """tests/golden/exact_general.npz (tools/gen_exact_general.py): QMF(...).solver on GOLDEN_CASES.  U and V bit for bit; W, where
    recorded, is the initial pair: it is recorded only while bit 2 is clear.  The reference's pair after update_w is another one
    from run to run (its fp32 lstsq), so the tool judges each draw as it runs (line_error, by hand below) and does not keep it."""
    z = np.load(os.path.join(GOLDEN, "exact_general.npz"))
    assert int(z["n"]) == len(E.GOLDEN_CASES) >= 14
    assert {c.name for c in E.GOLDEN_CASES} >= {"safe-div-eps", "eps-above-one", "w-v", "w-uv", "w-z0", "w-zc"}
    for i, c in enumerate(E.GOLDEN_CASES):
        assert json.loads(str(z[f"args{i}"])) == json.loads(json.dumps(c.args())), "regenerate the fixture"
        _, U, V, W, _ = results[c.id]
        assert np.array_equal(bits(U), bits(z[f"u{i}"])) and np.array_equal(bits(V), bits(z[f"v{i}"])), c.id
        assert (f"w{i}" in z.files) == (W is None), c.id
        for b in range(c.B if W is None else 0):
            check_w(c, z[f"w{i}"][b], None, b, "reference")


def test_line_error_by_hand():
    """x = [1, 3, 5, 9] on z = [0, 1, 2, 3]: the exact line is (3/5, 13/5).  w = (3/5, 13/5 + 1/10): A dw = z / 10, |.| = sqrt(14) / 10;
    |A|_F = sqrt(4 + 14), |x| = sqrt(116): bound = 8 * 2^-24 (sqrt(18) |w| + sqrt(116)).  A constant z = 3: every pair with w0 + 3 w1 =
    the mean is the line: (13/6 - 3e6, 1e6) has error 0 up to the fp64 rounding of numbers of that size."""
    x, z = np.array([1.0, 3.0, 5.0, 9.0]), np.array([0.0, 1.0, 2.0, 3.0])
    err, bound = E.line_error(x, z, (0.6, 2.7))
    assert abs(err - 14 ** 0.5 / 10) < 1e-12 and abs(bound - 8 * 2.0 ** -24 * (18 ** 0.5 * (0.36 + 7.29) ** 0.5 + 116 ** 0.5)) < 1e-15
    assert E.line_error(x, z, (0.6, 2.6))[0] < 1e-15
    err, bound = E.line_error(np.array([1.0, 2.0, 3.5]), np.full(3, 3.0), (13 / 6 - 3e6, 1e6))
    assert err < 1e-8 < bound
    assert E.line_error(np.array([1.0, 2.0, 3.5]), np.full(3, 3.0), (13 / 6 - 3e6 + 100.0, 1e6))[0] > bound


def test_reference_by_hand():
    """x = [[1, 2]], v0 = [[1, 0], [1, 0]] (b_00 = 2, b_11 = b_01 = 0), N = 2.  l2 = 1/2, l1_ratio = 1: l1 = 1, l2 = 0.  t = 3: (3 - 1) /
    2 = 1; column 1: (0 + eps) / (0 + eps) = 1.  x = [2, 2]: 3 / 2 -> 2 (to even).  x = [1, 0]: |t| = l1 -> 0.  x = [-4, -1]: -(5 - 1) /
    2 = -2.  x = [0, 0]... l2 = 1, l1_ratio = 0: l2 = 2: 6 / 4 -> 2 and eps / 2 -> 0.  Bounds (-3.5, 5.5): 20 / 2 -> 5, -20 / 2 -> -3."""
    v0 = np.array([[[1.0, 0.0], [1.0, 0.0]]])
    u0 = np.zeros((1, 1, 2))
    on = dict(l2=(0.5, 0.0), l1_ratio=1.0, factor=(0,))
    for x, opts, want, counts in (
            ([1, 2], on, [1, 1], dict(zero_den=1)),
            ([2, 2], on, [2, 1], dict(zero_den=1, ties=1)),
            ([1, 0], on, [0, 1], dict(zero_den=1, thr_eq=1)),
            ([-4, -1], on, [-2, 1], dict(zero_den=1)),
            ([3, 3], dict(l2=(1.0, 0.0), factor=(0,)), [2, 0], dict(ties=1)),
            ([20, 0], dict(bounds=(-3.5, 5.5), factor=(0,)), [5, 1], dict(zero_den=1, clamped=1)),
            ([-20, 0], dict(bounds=(-3.5, 5.5), factor=(0,)), [-3, 1], dict(zero_den=1, clamped=1)),
            ([300, 0], dict(factor=(0,)), [150, 1], dict(zero_den=1, big=1))):
        u, v, W, st = E.reference_general(np.array([[x]], np.float64), u0, v0, 1, opts)
        assert u[0, 0].tolist() == want and np.array_equal(v, v0) and W is None, (x, u)
        assert st["u"] == dict(dict.fromkeys(E.STAT_KEYS, 0), solves=2, **counts), (x, st["u"])
    # inside the threshold: l1 = 2 (l2 = 1), x = [1, 0]: 0 < |t| = 1 < 2 -> 0
    st = E.reference_general(np.array([[[1.0, 0.0]]]), u0, v0, 1, dict(l2=(1.0, 0.0), l1_ratio=1.0, factor=(0,)))[3]
    assert st["u"]["thr_in"] == 1
    # the pair: x = 3 + 0.5 * [2, 4] is x' = [2, 4]; |w1| = 0.25 < eps = 0.5 divides by 0.5; K = 0 returns the initial factors
    u = E.reference_general(np.array([[[4.0, 5.0]]]), u0, v0, 1, dict(w=(3.0, 0.5), factor=(0,)))[0]
    assert u[0, 0, 0] == 3.0
    u = E.reference_general(np.array([[[4.0, 5.0]]]), u0, v0, 1, dict(w=(3.0, 0.25), eps=0.5, factor=(0,)))[0]
    assert u[0, 0, 0] == 3.0  # (6 + 0.5) / (2 + 0.5) = 2.6
    u = E.reference_general(np.array([[[4.0, 6.0]]]), u0, v0, 1, dict(eps=2.0, factor=(0,)))[0]
    assert u[0, 0, 0] == 2.0  # the default pair: |w1| = 1 < eps = 2: x' = [2, 3], (5 + 2) / (2 + 2) = 1.75
    u, v, _, _ = E.reference_general(np.array([[[4.0, 5.0]]]), u0 + 7, v0, 0, dict(factor=(0, 1)))
    assert np.array_equal(u, u0 + 7) and np.array_equal(v, v0)


def test_reference_refuses_bad_cases():
    X = np.full((1, 384, 64), 700.0)
    with pytest.raises(AssertionError, match="2\\^24"):
        E.reference_general(X, np.ones((1, 384, 2)), np.ones((1, 64, 2)), 1, dict(bounds=(-128, 127)))
    with pytest.raises(AssertionError, match="not integers"):
        E.reference_general(np.ones((1, 130, 16)), np.ones((1, 130, 2)), np.ones((1, 16, 2)), 1, dict(l2=1 / 8, l1_ratio=1.0))
    with pytest.raises(AssertionError, match="not an integer"):
        E.reference_general(np.ones((1, 4, 4)), np.ones((1, 4, 2)), np.ones((1, 4, 2)), 1, dict(w=(0.5, 4.0)))
    with pytest.raises(AssertionError, match="ill-conditioned"):  # z = 2^21 +- 1: kappa ~ 2^42
        E.exact_line(np.array([0.0, 1.0, 2.0, 3.0]), np.array([2.0 ** 21 - 1, 2.0 ** 21 + 1] * 2))
    with pytest.raises(AssertionError, match="2\\^53"):
        E.exact_line(np.full(4096, 2.0 ** 20), np.full(4096, 2.0 ** 22))
    with pytest.raises(AssertionError, match="product"):  # the sums fit (sum z^2 = 2^52), n sum z^2 = 2^64 does not
        E.exact_line(np.ones(4096), np.full(4096, 2.0 ** 20))


def test_exact_line_and_loss_by_hand():
    """x = [1, 3, 5, 9] on z = [0, 1, 2, 3]: n = 4, sums 6, 14, 18, 40: det = 20, w1 = (160 - 108) / 20 = 13/5, w0 = 18/4 - 13/5 * 6/4 =
    3/5.  A constant z: (mean, 0).  Loss: x = [[3, 4]], u v^T = [[3, 0]]: 4 / 5; with w = (1, 2): y = [7, 1]: 5 / 5."""
    line = E.exact_line(np.array([1.0, 3.0, 5.0, 9.0]), np.array([0.0, 1.0, 2.0, 3.0]))
    assert (line["w0"], line["w1"]) == (Fraction(3, 5), Fraction(13, 5)) and line["kappa"] == 56 / 20
    line = E.exact_line(np.array([1.0, 2.0, 3.5]), np.array([3.0, 3.0, 3.0]))
    assert (line["w0"], line["w1"], line["kappa"]) == (Fraction(13, 6), 0, None)
    assert E.within_one_ulp(F32(0.6), Fraction(3, 5)) and E.within_one_ulp(np.nextafter(F32(0.6), F32(1)), Fraction(3, 5))
    assert not E.within_one_ulp(F32(0.6) + 2 * np.spacing(F32(0.6)), Fraction(3, 5)) and not E.within_one_ulp(F32(1e-30), Fraction(0))
    x, u, v = np.array([[3.0, 4.0]]), np.array([[3.0]]), np.array([[1.0], [0.0]])
    assert E.exact_loss(x, u, v) == F32(0.8) and E.exact_loss(x, u, v, (1.0, 2.0)) == F32(1.0)
    assert E.exact_loss(np.zeros((1, 2)), u, v) == F32(3e16) and E.exact_loss(np.zeros((1, 2)), 0 * u, v) == 0


def test_update_w_cases_are_exact_and_well_conditioned(results):
    """the 2^53 and kappa asserts of exact_line hold (they ran in `results`); the two lines from a dyadic pair have kappa near 1, the
    two degenerate cases a constant z (0 and 3) in every matrix"""
    for c in E.W_CASES:
        (X, _, _), U, V, W, _ = results[c.id]
        assert c.K == 1 and 2 in c.opts["factor"] and len(W) == c.B
        for b in range(c.B):
            zz = U[b].astype(np.float64) @ V[b].astype(np.float64).T
            if c.name in ("w-z0", "w-zc"):
                assert W[b]["kappa"] is None and (zz == (0 if c.name == "w-z0" else 3)).all()
                assert W[b]["w0"] == Fraction(int(X[b].sum()), X[b].size) and W[b]["w1"] == 0
            else:
                assert 1 <= W[b]["kappa"] <= 2 and W[b]["w1"] != 0
    assert {tuple(c.opts["factor"]) for c in E.W_CASES} == {(1, 2), (0, 1, 2), (2,)}


def test_loss_cases_are_exact(results):
    """exact_loss's asserts (grid, 2^24, 2^53) hold on every loss case, without and with the dyadic pair; rows 1, 64, 65 and B = 3"""
    assert {c.M for c in E.LOSS_CASES} >= {1, 64, 65} and {c.B for c in E.LOSS_CASES} >= {3}
    seen = []
    for c in E.LOSS_CASES:
        (X, _, _), U, V, _, _ = results[c.id]
        for b in range(c.B):
            for w in (None, E.LOSS_W):
                seen.append(float(E.exact_loss(X[b], U[b], V[b], w)))
    assert all(np.isfinite(seen)) and min(seen) == 0.0 and max(seen) > 1e15  # (an all-zero x: 0 / 1e-16 and |y| / 1e-16)
    assert sum(0 < s < 10 for s in seen) > len(seen) // 2


@pytest.mark.parametrize("half", "uv")
def test_data_conditions(half, results):
    """Conditions, not measurements: over the cases that carry each mark, separately for U halves and V halves, rounding ties,
    |t| == l1, 0 < |t| < l1, zero denominators, clamped values and |new| > 127 are each at least 1 % of the solves (and occur in
    every case that carries the mark); rounding ties in U halves over the WHOLE table at least 5 %."""
    for mark, key in E.MARK_KEYS.items():
        marked = [c for c in E.ALL if mark in c.marks[half]]
        assert marked, (half, mark)
        hit = sum(results[c.id][4][half][key] for c in marked)
        solves = sum(results[c.id][4][half]["solves"] for c in marked)
        assert hit >= 0.01 * solves > 0, (half, mark, hit, solves)
        for c in marked:
            assert results[c.id][4][half][key] > 0, (c.id, half, mark)
    if half == "u":
        ties = sum(results[c.id][4]["u"]["ties"] for c in E.ALL)
        assert ties >= 0.05 * sum(results[c.id][4]["u"]["solves"] for c in E.ALL)


def test_cases_hold_every_option():
    get = lambda c, k, d: c.opts.get(k, d)
    pair = lambda c: get(c, "l2", 0.0) if isinstance(get(c, "l2", 0.0), tuple) else (get(c, "l2", 0.0),) * 2
    l1 = {c.id: E.terms(c.opts, c.M, c.N) for c in E.ALL}  # (l1_u, l2_u, l1_v, l2_v), integers (asserted there)
    assert any(t[0] > 0 and t[1] == 0 for t in l1.values()) and any(t[0] == 0 and t[1] > 0 for t in l1.values())
    assert any(t[0] > 0 and t[1] > 0 for t in l1.values()) and any(t[2] > 0 for t in l1.values())
    assert any(pair(c)[0] != pair(c)[1] and min(pair(c)) > 0 for c in E.ALL)
    assert any(get(c, "l1_ratio", 0) == 1.0 for c in E.ALL) and any(get(c, "l1_ratio", 0) == 0.5 for c in E.ALL)
    bounds = {tuple(get(c, "bounds", (None, None))) for c in E.ALL}
    assert bounds >= {(None, None), (-1000, 1000), (-3.5, 5.5), (-16, 15)}
    assert E.clamp_bounds(dict(bounds=(-3.5, 5.5))) == (-3.0, 5.0)
    assert {tuple(c.opts["factor"]) for c in E.CASES} == {(0,), (1,), (0, 1)}
    assert {get(c, "eps", 1e-16) for c in E.ALL} == {1e-16, 0.5, 2.0}
    assert {tuple(get(c, "w", (0.0, 1.0))) for c in E.CASES} == {(0.0, 1.0), (3.0, 0.5), (-7.0, 4.0), (3.0, 0.25)}
    assert {c.K for c in E.CASES} == {0, 1, 2, 3}
    zero_col = {c.name: E.terms(c.opts, c.M, c.N)[1] for c in E.CASES if c.gen["zero_v"] and c.K == 1}
    assert zero_col == {"zero-col": 0, "zero-col-l2": 4}
    assert any(c.B > 2 and c.gen["zero_matrix"] for c in E.ALL) and max(c.B for c in E.ALL) == 4
    assert max(c.B * c.M * c.N for c in E.ALL) <= 100000 and len({c.id for c in E.ALL}) == len(E.ALL)
    assert all(c.B > 1 for c in E.LOSS_CASES if c.M > 1)


def test_zero_columns_and_zero_matrices_give_what_they_are_for(results):
    """an all-zero column of V0: ones with l2 = 0 ((0 + eps) / (0 + eps)), zeros with l2 > 0; an all-zero X: a zero U, then a V
    of ones; K = 0: the initial factors; fractional bounds reach -3 and 5, the wide ones +-1000, unbounded factors go past them"""
    for name, want in (("zero-col", 1.0), ("zero-col-l2", 0.0)):
        c = [c for c in E.CASES if c.name == name][0]
        assert (results[c.id][1][:, :, c.R // 2] == want).all()
    c = [c for c in E.CASES if c.name == "rows63-zero"][0]
    assert (results[c.id][1][1] == 0).all() and (results[c.id][2][1] == 1).all() and (results[c.id][0][0][1] == 0).all()
    c = [c for c in E.CASES if c.name == "k0"][0]
    (X, U0, V0), U, V, W, st = results[c.id]
    assert np.array_equal(U, U0) and np.array_equal(V, V0) and W is None and st["u"]["solves"] == st["v"]["solves"] == 0
    for name, half, lo, hi in (("r2-frac", 1, -3, 5), ("v-frac", 2, -3, 5), ("r4-wide", 1, -1000, 1000), ("v-wide", 2, -1000, 1000)):
        c = [c for c in E.CASES if c.name == name][0]
        assert (results[c.id][half].min(), results[c.id][half].max()) == (lo, hi), name
    c = [c for c in E.CASES if c.name == "v-unb"][0]
    assert np.abs(results[c.id][2]).max() > 1000


# ---- the plan, by hand (the rules of tests/test_any_plan.py's docstring, in the order any_prod applies them) ----
def prod_by_hand(I, D, R):
    """(kernel, folded, native) of C [I, R] = A [I, D] B [D, R]: native below 400 multiply-adds, always on k_any_prod; R <= 16:
    I <= 16 and D > 64 -> THIN_LONG, D <= 64 and I >= 256 -> THIN_SHORT4 / 8 / 16 for D <= 16 / 32 / 64; D > 32, I > 64, R > 16 -> BIG;
    else TILED.  A contraction above 384 is folded."""
    fold = D > 384
    if D * I * R < 400:
        return TILED, fold, True
    if R <= 16 and I <= 16 and D > 64:
        return LONG, fold, False
    if R <= 16 and D <= 64 and I >= 256:
        return (SHORT4 if D <= 16 else SHORT8 if D <= 32 else SHORT16), False, False
    if D > 32 and I > 64 and R > 16:
        return BIG, fold, False
    return TILED, fold, False


def half_by_hand(c, trans):
    """((a), (b), (sweep kernel, native order, rows)) of one half: a = x @ v [rows, R] over depth, b = v.mT @ v [R, R] over depth;
    the sweep in ATen's native order below (R - 1) rows = 400, the diagonal in LDS up to rank 629"""
    rows, depth = (c.N, c.M) if trans else (c.M, c.N)
    return prod_by_hand(rows, depth, c.R), prod_by_hand(c.R, depth, c.R), (gs_kernel_by_hand(c.R, False), (c.R - 1) * rows < 400, rows)


def test_plan_is_the_one_by_hand_and_covers_every_variant(lib):
    prods, sweeps, mkl_ranks, native_ranks = set(), set(), set(), set()
    for c in E.ALL:
        for h, trans in c.halves():
            a, b, g = update(lib, c.B, c.M, c.N, c.R, trans)
            want = half_by_hand(c, trans)
            for got, w in ((a, want[0]), (b, want[1])):
                assert (got["k"], bool(got["fold"]), bool(got["native"]), got["refused"]) == w + (0,), (c.id, h, got, w)
                prods.add(w)
            assert (g["k"], bool(g["native_gs"]), g["gx"], g["gy"]) == want[2][:2] + ((want[2][2] + 63) // 64, c.B), (c.id, h, g)
            sweeps.add(want[2])
            (native_ranks if want[2][1] else mkl_ranks).add(c.R)
    assert prods >= {(LONG, False, False), (LONG, True, False), (SHORT4, False, False), (SHORT8, False, False), (SHORT16, False, False),
                     (BIG, False, False), (BIG, True, False), (TILED, False, False), (TILED, True, False), (TILED, False, True)}
    assert {(k, n) for k, n, _ in sweeps} >= {("GS_F32_LDS", False), ("GS_F32_LDS", True), ("GS_F32_NOLDS", False)}
    assert {c.R for c in E.ALL if c.halves()} >= {1, 2, 3, 4, 5, 9, 10, 17, 18, 64, 65, 129, 629, 630}
    # any_term2 in MKL's order: its early returns (R - 1 = 1, 2), the unrolled eight with tails of both parities, fetch_b's guards
    assert mkl_ranks >= {2, 3, 4, 5, 9, 10, 17, 18, 64, 65, 129, 629, 630} and native_ranks >= {1, 3, 4, 5}
    assert {rows for _, _, rows in sweeps} >= {1, 63, 64, 65, 130}
    assert {gs_kernel_by_hand(629, False), gs_kernel_by_hand(630, False)} == {"GS_F32_LDS", "GS_F32_NOLDS"}


def test_docstring_lists_every_case_as_planned_and_measured(lib, results):
    """the table in tests/exact_general.py's docstring is the output of `python tests/exact_general.py`"""
    for c in E.ALL:
        plans = {h: update(lib, c.B, c.M, c.N, c.R, trans) for h, trans in c.halves()}
        for line in E.describe(c, plans, results[c.id][4]):
            assert "\n" + line.rstrip() + "\n" in E.__doc__, line
