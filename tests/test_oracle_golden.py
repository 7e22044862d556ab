"""CPU suite: the oracle (oracle/lrf_oracle.c) against the golden vectors captured from the reference."""
import hashlib

import numpy as np
import pytest

from conftest import QMF_CASES, Case

# cases whose planes have full column rank, so that even the *initialisation* is determined up to sign (the order of the
# oracle's products is pinned to the reference's up to rank 205: tools/pin_oracle_anyshape.py, lrf_oracle.c header)
EXACT_CASES = ["tiny_q7", "tiny_r7", "tiny_it1", "tiny_it2", "odd_q7", "odd_r7", "smooth_q7", "smooth_r7", "s1_q7",
               "s1_r7", "nat_q7", "nat_r7", "s2odd_q7", "tiny_rank2"]


@pytest.mark.parametrize("name", QMF_CASES)
def test_planes_and_decode_match_reference(name, oracle):
    """L0: decoding the reference's factors reproduces the reference's decoded image bit for bit."""
    case = Case(name)
    H, W = case.image.shape[-2:]
    f = case.ref_factors()
    dec = oracle.planes_to_rgb(f[0::2], f[1::2], H, W)
    assert hashlib.sha256(dec.tobytes()).hexdigest() == case.decoded_sha256
    mse = np.mean((case.image.numpy().astype(np.float32) - dec.astype(np.float32)) ** 2)
    assert abs(20 * np.log10(255 / np.sqrt(mse)) - case.psnr) < 1e-3


@pytest.mark.parametrize("name", ["tiny_q7", "tiny_r7", "tiny_rank2", "tiny_it1", "tiny_it2", "odd_q7", "odd_r7"])
def test_bcd_from_reference_init_is_bit_exact(name, oracle):
    """L1: from the reference's own (u0, v0) the BCD iterations give the reference's int8 factors exactly."""
    case = Case(name)
    X = oracle.rgb_to_planes(case.image.numpy())
    f = case.ref_factors()
    K = case.kwargs.get("num_iters", 10)
    for c in range(3):
        u, v = oracle.bcd(X[c], case.z[f"u0_{c}"], case.z[f"v0_{c}"], K)
        assert np.array_equal(u.astype(np.int8), f[2 * c]), f"U plane {c}"
        assert np.array_equal(v.astype(np.int8), f[2 * c + 1]), f"V plane {c}"


@pytest.mark.parametrize("name", EXACT_CASES)
def test_full_encode_with_reference_signs_is_bit_exact(name, oracle):
    """L3: own initialisation (fp64 Gram + Jacobi) with the reference's LAPACK column signs -> identical factors."""
    case = Case(name)
    X = oracle.rgb_to_planes(case.image.numpy())
    f = case.ref_factors()
    K = case.kwargs.get("num_iters", 10)
    bad = 0
    for c in range(3):
        u, v = oracle.qmf_decompose(X[c], case.ranks[c], K, (-16, 15), sign=case.z[f"sign{c}"])
        bad += int((u.astype(np.int8) != f[2 * c]).sum()) + int((v.astype(np.int8) != f[2 * c + 1]).sum())
    assert bad == 0, f"{bad} factor entries differ from the reference"


@pytest.mark.parametrize("name", ["tiny_q20", "tiny_rank1", "zero_q7", "const_q7"])
def test_unpinned_cases_psnr(name, oracle):
    """R > 7 (MKL order not pinned), R == 1 (gemv order not pinned) and rank-deficient planes (LAPACK's null-space
    vectors are arbitrary): factors may differ from the reference; the decoded quality must not."""
    case = Case(name)
    H, W = case.image.shape[-2:]
    X = oracle.rgb_to_planes(case.image.numpy())
    U, V = [], []
    for c in range(3):
        u, v = oracle.qmf_decompose(X[c], case.ranks[c], case.kwargs.get("num_iters", 10), (-16, 15), sign=case.z[f"sign{c}"])
        U.append(u.astype(np.int8))
        V.append(v.astype(np.int8))
    dec = oracle.planes_to_rgb(U, V, H, W)
    mse = np.mean((case.image.numpy().astype(np.float32) - dec.astype(np.float32)) ** 2)
    psnr = 20 * np.log10(255 / np.sqrt(mse)) if mse > 0 else 99.0
    tol = 0.25 if name in ("zero_q7", "const_q7") else 0.05
    assert psnr > case.psnr - tol, f"PSNR {psnr:.3f} vs reference {case.psnr:.3f}"


def test_default_sign_changes_nothing_but_sign_for_quality(oracle):
    """L2: without the reference's signs the factors differ only through the joint column sign; PSNR stays put."""
    case = Case("smooth_r7")
    H, W = case.image.shape[-2:]
    X = oracle.rgb_to_planes(case.image.numpy())
    U, V = [], []
    for c in range(3):
        u, v = oracle.qmf_decompose(X[c], case.ranks[c], 10, (-16, 15))
        U.append(u.astype(np.int8))
        V.append(v.astype(np.int8))
    dec = oracle.planes_to_rgb(U, V, H, W)
    mse = np.mean((case.image.numpy().astype(np.float32) - dec.astype(np.float32)) ** 2)
    assert abs(20 * np.log10(255 / np.sqrt(mse)) - case.psnr) < 0.05


def test_jacobi_eigen(oracle):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((500, 64))
    G = A.T @ A
    lam, E, sweeps = oracle.jacobi_f64(G)
    assert sweeps < 15
    assert np.allclose(E @ np.diag(lam) @ E.T, G, rtol=0, atol=1e-9 * np.abs(G).max())
    assert np.allclose(E.T @ E, np.eye(64), atol=1e-13)
    assert np.allclose(np.sort(lam), np.linalg.eigvalsh(G), rtol=1e-12, atol=1e-9)


def test_quantize_roundtrip(oracle):
    rng = np.random.default_rng(1)
    t = rng.standard_normal((100, 5)).astype(np.float32) * 10
    q, sc, mn = oracle.quantize_u8(t)
    back = oracle.dequantize_u8(q, sc, mn)
    assert q.min() == 0 and q.max() == 255
    assert np.abs(back - t).max() <= sc * 1.001


@pytest.mark.parametrize("name", ["svd_tiny_q2p5", "svd_smooth_q2p5"])
def test_svd_baseline_oracle(name, oracle):
    """SVD baseline (lrf/compression/svd.py default branch): the oracle decodes the reference's bytes exactly and its
    encoder side agrees with the reference's uint8 codes to within one step (fp32 LAPACK vs fp64 Gram route)."""
    import json
    import os

    from conftest import GOLDEN
    from lrf_amd.container import bytes_to_dict, decode_tensor, separate_bytes
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    img = z["image"]
    meta_b, fac_b = separate_bytes(z["encoded"].tobytes(), 2)
    meta = bytes_to_dict(meta_b)
    qu, qv = [decode_tensor(f) for f in separate_bytes(fac_b, 2)]
    dec = oracle.svd_decode_rgb(qu, qv, meta["quantization"]["u"], meta["quantization"]["v"], img.shape[1], img.shape[2])
    assert hashlib.sha256(dec.tobytes()).hexdigest() == str(z["decoded_sha256"])
    X = oracle.pad_patchify(img.astype(np.float32))
    rvf = oracle.dequantize_u8(qv, *meta["quantization"]["v"])
    _, ov = oracle.svd_topr(X, qu.shape[1])
    sign = np.where((ov.astype(np.float64) * rvf).sum(0) >= 0, -1, 1).astype(np.int8)
    u, v = oracle.svd_topr(X, qu.shape[1], sign)
    for t, q, (sc, mn) in ((u, qu, meta["quantization"]["u"]), (v, qv, meta["quantization"]["v"])):
        got, s2, m2 = oracle.quantize_u8(t)
        assert abs(s2 / sc - 1) < 1e-4 and abs(m2 - mn) < 1e-4 * abs(mn) + 1e-4
        d = np.abs(got.astype(np.int32) - q.astype(np.int32))
        assert (d <= 1).mean() >= 0.995 and d.max() <= 2


def _sturm_grid(d):
    """First-pass shifts of the oracle's multisection for a DIAGONAL matrix diag(d) (oracle/lrf_oracle.c top_eigenvalues,
    restated in numpy doubles): returns the 64 shifts in the matrix's own scale."""
    import math
    lo, hi = float(min(d)), float(max(d))
    tn = max(abs(lo), abs(hi))
    slack = 2.0 * tn * 2.220446049250313e-16 * 64 + 2.0 * 2.2250738585072014e-300
    lo -= slack
    hi += slack
    s = math.frexp(max(abs(lo), abs(hi)))[1]
    a, b = math.ldexp(lo, -s), math.ldexp(hi, -s)
    h = (b - a) / 65.0
    return [math.ldexp(a + h * float(i + 1), s) for i in range(64)]


def test_tridiagonal_eigen_solver(oracle):
    """lrf_oracle_top_eig_f64 (Householder tridiagonalisation + division-free Sturm counts + twisted factorisation; the
    arithmetic k_init mirrors) against LAPACK, on full-rank, rank-deficient, constant and zero Gram matrices."""
    rng = np.random.default_rng(5)
    for trial in range(6):
        X = rng.random((500, 64)) * 255
        if trial == 1: X[:, 10:] = 0
        if trial == 2: X[:] = 7.0
        if trial == 3: X[:] = 0
        if trial == 4: X = np.outer(rng.random(500), rng.random(64)) * 100
        if trial == 5: X = np.diag(np.arange(64.0))
        G = X.T @ X
        lam, E = oracle.top_eig_f64(G, 8)
        w = np.linalg.eigvalsh(G)[::-1][:8]
        scale = max(w[0], 1e-300)
        assert np.abs(lam - w).max() <= 4e-15 * scale
        assert np.abs(E.T @ E - np.eye(8)).max() < 1e-13
        assert np.abs(G @ E - E * lam[None, :]).max() <= 1e-13 * scale


def test_sturm_count_zero_minor_rule(oracle):
    """A shift of the multisection that equals a diagonal entry exactly makes a leading minor exactly zero; the count
    must still be right (the replacement rule of sturm_count).  Diagonal matrices whose entries sit ON the first-pass grid."""
    base = [float(64 - i) for i in range(64)]  # 64, 63, ..., 1
    grid = _sturm_grid(base)
    hits = 0
    for lane in (3, 17, 40, 62):
        d = list(base)
        d[10] = grid[lane]  # strictly inside the hull: the hull, hence the grid, is unchanged
        assert _sturm_grid(d) == grid
        G = np.diag(np.array(d))
        lam, E = oracle.top_eig_f64(G, 8)
        w = np.sort(np.array(d))[::-1][:8]
        assert np.abs(lam - w).max() <= 4e-15 * 64, (lane, lam, w)
        hits += 1
    assert hits == 4
