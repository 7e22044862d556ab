"""The SVD initialisation of the HIP kernels on hard spectra (tests/hard_spectra.py): k_gram64 + k_init for 64 columns,
k_any_eig behind every tridiagonalisation variant for the other shapes, and the [M,192] uint8 route of svd_encode.  Bit for
bit the oracle's, then the properties against numpy's float64 SVD on the GPU's own output."""
import numpy as np
import pytest
import torch

import hard_spectra as hs
from svd_cases import image_of_patch_matrix as _image_of_patch_matrix
from test_init_hard_spectra import END_TO_END

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lrf_amd import _lib
    return _lib.context(0)


def _oracle_init(oracle, X, R):
    return oracle.svd_init(X, R) if X.shape[1] == 64 else oracle.svd_topr_any(X, R)


_NEIGHBOURS = {}


def _neighbours(oracle, shape, R):
    """Two regular matrices of a shape (dominant directions + noise + a mean: simple, well separated eigenvalues) and the
    oracle's initialisation of them, computed once per (shape, rank)"""
    key = (shape, R)
    if key not in _NEIGHBOURS:
        M, N = shape
        rng = np.random.default_rng(M * 1009 + N * 13 + R)
        out = []
        for _ in range(2):
            k = min(12, M, N)
            X = (rng.normal(size=(M, k)) @ rng.normal(size=(k, N)) * 20 + rng.normal(size=(M, N)) * 5 + 100).astype(np.float32)
            out.append((X, _oracle_init(oracle, X, R)))
        _NEIGHBOURS[key] = out
    return _NEIGHBOURS[key]


BATCHED = [(path, cls, name, R) for path in ("init64", "any") for cls, name, R in hs.case_ids(path)]


@pytest.mark.parametrize("path,cls,name,R", BATCHED, ids=[f"{p}-{c}-{n}-R{R}" for p, c, n, R in BATCHED])
def test_hip_init_bits_and_properties(path, cls, name, R, ctx, oracle):
    """Context.svd_init on [regular, hard, regular]: u0 and v0 of all three equal the oracle's bit for bit (signs of zeros
    count) — a hard neighbour changes nothing for the others —, and the GPU's output for the hard one has P1-P4."""
    X = hs.get_case(path, cls, name)
    (Xa, wa), (Xb, wb) = _neighbours(oracle, X.shape, R)
    batch = np.stack([Xa, X, Xb])
    u0, v0 = ctx.svd_init(torch.from_numpy(batch).cuda(), R)
    u0, v0 = u0.cpu().numpy(), v0.cpu().numpy()
    for b, (wu, wv) in enumerate((wa, _oracle_init(oracle, X, R), wb)):
        assert np.array_equal(v0[b].view(np.int32), wv.view(np.int32)), f"v0 of matrix {b} differs from the oracle's"
        assert np.array_equal(u0[b].view(np.int32), wu.view(np.int32)), f"u0 of matrix {b} differs from the oracle's"
    hs.check_init(X, R, u0[1], v0[1], only_p12=name in hs.P12_ONLY)


U8 = [(cls, name, R) for cls, name, R in hs.case_ids("u8")]


@pytest.mark.parametrize("cls,name,R", U8, ids=[f"{c}-{n}-R{R}" for c, n, R in U8])
def test_hip_u8_route_equals_oracle(cls, name, R, ctx, oracle):
    """The [M,192] uint8 route (k_gram192_u8 + k_any_eig), reached as svd_encode reaches it: the quantised factors and their
    quantisation parameters equal the oracle's — whose float factors tests/test_init_hard_spectra.py holds to P1-P4."""
    X = hs.get_case("u8", cls, name)
    img = _image_of_patch_matrix(X, 12, 20)
    assert np.array_equal(oracle.rgb_matrix_any(img, (8, 8)), X)
    U, V, qp = ctx.svd_encode_rgb(torch.from_numpy(img).cuda().unsqueeze(0), R)
    u, v = oracle.svd_topr_u8(X, R)
    hs.check_init(X, R, u, v)
    qu, su, mu = oracle.quantize_u8(u)
    qv, sv, mv = oracle.quantize_u8(v)
    assert np.array_equal(U[0].cpu().numpy(), qu) and np.array_equal(V[0].cpu().numpy(), qv)
    assert np.array_equal(qp[0].cpu().numpy(), np.array([su, mu, sv, mv], np.float32))


@pytest.mark.parametrize("name,R", END_TO_END)
def test_hip_decompose_equals_oracle_64(name, R, ctx, oracle):
    X = hs.get_case("init64", "dup", name)
    U, V = ctx.decompose(torch.from_numpy(X[None].copy()).cuda(), R, 10, -16, 15)
    uo, vo = oracle.qmf_decompose(X, R, 10, (-16, 15))
    assert np.array_equal(U[0].cpu().numpy(), uo.astype(np.int8)) and np.array_equal(V[0].cpu().numpy(), vo.astype(np.int8))


@pytest.mark.parametrize("name", [n for n, _, _ in hs.cases("any", "dup")])
def test_hip_decompose_equals_oracle_any_shape(name, ctx, oracle):
    """one repeated-singular-value matrix per tridiagonalisation variant, rank 7: initialisation + ten BCD iterations"""
    X = hs.get_case("any", "dup", name)
    U, V = ctx.decompose(torch.from_numpy(X[None].copy()).cuda(), 7, 10, -16, 15)
    u0, v0 = oracle.svd_topr_any(X, 7)
    uo, vo = oracle.bcd(X, u0, v0, 10, (-16, 15))
    assert np.array_equal(U[0].cpu().numpy(), uo.astype(np.int8)) and np.array_equal(V[0].cpu().numpy(), vo.astype(np.int8))
