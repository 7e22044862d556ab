"""GPU suite (-m gpu): Context.decompose_ex (lrf_qmf_decompose_ex_f32) on the exact-integer cases of tests/exact_general.py against
reference_general, the whole batch in one call, both factors bit for bit: rounding ties, numerators on and inside the l1
threshold, zero denominators, clamps, values past +-127, every option of the class — on k_any_gs<float, true / false>, the five
product kernels with k_any_fold, and k_any_affine.  The pair W after update_w within 1 fp32 ulp of the exact least-squares line
(k_any_wstats, k_any_wsolve), Context.loss within 1 fp32 ulp of the exact sums (k_any_loss, k_any_loss_finish).
tests/test_exact_general.py holds the CPU gates: the integer restatement equals the oracle and the reference project's recorded
factors, so a mismatch here is the kernel's."""
import numpy as np
import pytest
import torch

import exact_general as E
from test_any_plan import lib, update  # noqa: F401 (lib: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lrf_amd import _lib
    return _lib.context(0)


@pytest.fixture(scope="module")
def expected():
    """reference_general per case, computed when first asked for and shared, unchanged: id -> (inputs, U, V, W)"""
    cache = {}

    def get(case):
        if case.id not in cache:
            inputs = case.inputs()
            cache[case.id] = (inputs,) + E.reference_general(*inputs, case.K, case.opts)[:3]
        return cache[case.id]
    return get


bits = E.bits


def run(ctx, case, X, U0, V0):
    """one call on the matrices given -> fp32 numpy (U, V, W)"""
    opts = dict(case.opts)
    w = opts.pop("w", None)
    w_init = None if w is None else torch.tensor([w] * X.shape[0], dtype=torch.float32)
    Xd, U0d, V0d = (torch.from_numpy(np.ascontiguousarray(t)).float().cuda() for t in (X, U0, V0))
    U, V, W = ctx.decompose_ex(Xd, case.R, case.K, init=(U0d, V0d), w_init=w_init, **opts)
    return tuple(t.numpy() for t in ctx.to_host(U, V, W))


def first_difference(case, inputs, got, want, half, planned):
    ne = np.argwhere(bits(got) != bits(want))
    if not len(ne):
        return None
    b, i, r = (int(t) for t in ne[0])
    return (f"{case.id} ({planned}): {half.upper()} differs in {len(ne)} of {got.size} entries, first at matrix {b}, row {i}, column {r}: "
            f"got {got[b, i, r]!r}; " + E.explain(case, inputs, b, half, i, r))


@pytest.mark.parametrize("case", E.ALL, ids=lambda c: c.id)
def test_general_solver_equals_the_integer_reference(case, ctx, expected, lib):
    inputs, want_u, want_v, W = expected(case)
    planned = "; ".join(f"{h.upper()} {E.kernels(update(lib, case.B, case.M, case.N, case.R, trans))}" for h, trans in case.halves())
    U, V, Wg = run(ctx, case, *inputs)
    bad = [m for m in (first_difference(case, inputs, U, want_u, "u", planned), first_difference(case, inputs, V, want_v, "v", planned)) if m]
    assert not bad, "\n".join(bad)
    for b in range(case.B):
        E.check_w(case, Wg[b], W, b, "lrf_qmf_decompose_ex_f32")
    # a matrix's result does not depend on its neighbours: matrix by matrix equals the batched call
    for b in range(case.B if case.B > 1 else 0):
        u, v, w = run(ctx, case, *(t[b:b + 1] for t in inputs))
        assert np.array_equal(bits(u[0]), bits(U[b])) and np.array_equal(bits(v[0]), bits(V[b])) and np.array_equal(bits(w[0]), bits(Wg[b])), (case.id, b)


@pytest.mark.parametrize("case", E.LOSS_CASES, ids=lambda c: c.id)
def test_loss_equals_the_exact_sums(case, ctx, expected):
    """Context.loss on the case's X and the reference's factors, without a pair and with the dyadic one: within 1 fp32 ulp of
    fp32(sqrt(sum (x - y)^2) / (sqrt(sum x^2) + 1e-16)) from integer sums (two fp64 square roots, a division, the cast); the
    batched call equals the call per matrix bit for bit"""
    (X, _, _), U, V, _ = expected(case)
    Xd, Ud, Vd = (torch.from_numpy(np.ascontiguousarray(t)).float().cuda() for t in (X, U, V))
    for w in (None, E.LOSS_W):
        Wd = None if w is None else torch.tensor([w] * case.B, dtype=torch.float32).cuda()
        got = ctx.to_host(ctx.loss(Xd, Ud, Vd, Wd))[0].numpy()
        for b in range(case.B):
            want = E.exact_loss(X[b], U[b], V[b], w)
            assert abs(float(got[b]) - float(want)) <= float(np.spacing(want)), (case.id, b, w, float(got[b]), float(want))
            one = ctx.to_host(ctx.loss(Xd[b:b + 1], Ud[b:b + 1], Vd[b:b + 1], None if w is None else Wd[b:b + 1]))[0].numpy()
            assert bits(one)[0] == bits(got)[b], (case.id, b, w, float(one[0]), float(got[b]))
