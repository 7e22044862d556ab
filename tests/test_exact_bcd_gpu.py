"""GPU suite (-m gpu): Context.bcd (lrf_qmf_bcd_f32) on the exact-integer cases of tests/exact_bcd.py against reference_bcd, every
matrix, both factors, bit for bit: rounding ties in a few to 45 per cent of the solves, quotients an ulp beside a tie, zero
denominators, clamps — on every U-update kernel a caller's U0 can plan, the three bodies of the persistent launch, the V
updates of the three rank families and the any-shape Gauss-Seidel.  tests/test_exact_bcd.py holds the CPU gates: the reference
equals the oracle and the reference project's recorded factors, so a mismatch here is the kernel's."""
import os

import numpy as np
import pytest
import torch

import exact_bcd as E
from test_bcd_plan import FIRST_U0, lib, plan  # noqa: F401 (lib: the fixture)

pytestmark = pytest.mark.gpu
HOOKS = ("LRF_PERSIST", "LRF_FAMILY_SPLIT_BLOCKS", "LRF_BCDW16_MIN_BLOCKS", "LRF_BCDW32_MIN_BLOCKS")


@pytest.fixture(scope="module")
def ctx():
    from lrf_amd import _lib
    assert not [h for h in HOOKS if h in os.environ], "the table reaches its kernels at default settings: unset the threshold hooks"
    return _lib.context(0)


def first_difference(case, inputs, got, want, half):
    ne = np.argwhere(got != want)
    if not len(ne):
        return None
    b, i, r = (int(t) for t in ne[0])
    X, U0, V0 = (t[b] for t in inputs)
    return (f"{case.id}: {half.upper()} differs in {len(ne)} of {got.size} entries, first at matrix {b}, row {i}, column {r}: got {int(got[b, i, r])}; "
            + E.explain(X, U0, V0, case.K, case.lo, case.hi, half, i, r))


def run_case(ctx, case):
    from lrf_amd import _lib
    inputs = case.inputs()
    want_u, want_v, st = E.reference_bcd(*inputs, case.K, case.lo, case.hi)
    X, U0, V0 = (torch.from_numpy(t).float().cuda() for t in inputs)
    ctx.profile_kernels([_lib.LRF_K_BCD, _lib.LRF_K_BCD_PERSIST])
    ctx.profile_reset()
    U, V = ctx.bcd(X, U0, V0, case.K, case.lo, case.hi)
    torch.cuda.synchronize()
    launches = ctx.kernel_time(_lib.LRF_K_BCD_PERSIST)[1]
    ctx.profile(False)
    Uh, Vh = ctx.to_host(U, V)  # (and ctx.check(): raises if a persistent launch gave up)
    bad = [m for m in (first_difference(case, inputs, Uh.numpy(), want_u, "u"), first_difference(case, inputs, Vh.numpy(), want_v, "v")) if m]
    assert not bad, "\n".join(bad)
    return launches, st


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c.id)
def test_64_column_kernels_equal_the_integer_reference(case, ctx, lib):
    head, _ = plan(lib, [(case.M, case.R)] * case.B, case.K, (case.lo, case.hi), FIRST_U0)
    launches, st = run_case(ctx, case)
    assert launches == (1 if head["persist"] else 0), (case.id, launches, head)
    # the whole case holds what its first matrices promised (tests/test_exact_bcd.py measures those)
    assert case.R < 2 or E.share(st["u"]) >= 2.0
    assert "v" not in case.marks or E.share(st["v"]) >= 1.0


@pytest.mark.parametrize("case", E.ANY_CASES, ids=lambda c: c.id)
def test_any_shape_gauss_seidel_equals_the_integer_reference(case, ctx):
    launches, _ = run_case(ctx, case)
    assert launches == 0
