"""Matrices whose spectra are hard for the SVD initialisation, and the properties its output must have.

Plain numpy, deterministic.  Shared by tests/test_init_hard_spectra.py (the CPU oracle) and
tests/test_init_hard_spectra_gpu.py (the HIP kernels).  Every builder returns (name, X fp32 [M,N], ranks).

Classes
  dup           repeated NON-ZERO singular values that leave the tridiagonal form exactly (or nearly) reducible: block
                diagonal copies A + A, A + A + A, S + flip(S), and a dense Hadamard rotation of A + A.  The twisted
                factorisation returns one vector for all copies of an eigenvalue; the copies after the first go through the
                fallback of the orthonormalisation stage.
  regular-hard  spectra that are hard in other ways (permuted and interleaved copies may or may not split the tridiagonal
                form: see the table): permuted / interleaved copies, distinct blocks, a D4-symmetric image, Hadamard and diagonal Gram matrices, exact and near pairs, seven equal
                values, graded spectra, tiny and huge entries, zero rows and columns, rank deficiency.

check_init(X, R, u0, v0), against numpy.linalg.svd of X in float64, Rc = min(R, M, N):
  P1  everything finite
  P2  excess = (|X - u0 v0^T|_F^2 - sum_{i>=Rc} s_i^2) / |X|_F^2 <= 1e-10
  P3  | |v0_r|^2 - s_r | and | |u0_r|^2 - s_r | <= 2e-6 s_0                     (r < Rc)
  P4  normalised columns of v0 with s_r >= 1e-3 s_0:  max |V^T V - I| <= 1e-5

Largest value per case over its ranks, CPU oracle (oracle.svd_init / svd_topr_any / svd_topr_u8):

  path    class    case                   before the fix: P2 / P3 / P4      after: P2 / P3 / P4
  init64  dup      dup64_noise            4.1e-01 / 9.9e-01 / 4.9e-02   7.4e-15 / 1.3e-08 / 1.4e-08
  init64  dup      dup64_smooth           5.0e-01 / 1.0e+00 / 1.0e-01   8.8e-15 / 1.7e-08 / 1.7e-08
  init64  dup      dup64_three            7.6e-01 / 6.5e+00 / 9.9e-01   5.4e-15 / 2.2e-08 / 1.4e-08
  init64  dup      dup64_flip             4.9e-01 / 9.8e-01 / 1.7e-08   1.0e-14 / 2.0e-08 / 1.7e-08
  init64  dup      dup64_hadamard         4.1e-01 / 9.9e-01 / 3.5e-03   1.5e-14 / 7.8e-08 / 1.7e-08
  init64  regular  perm_dup               3.8e-01 / 9.9e-01 / 1.3e-08   7.6e-15 / 6.3e-09 / 1.2e-08
  init64  regular  kron_I2                4.7e-03 / 8.1e-02 / 1.8e-08   8.3e-15 / 5.3e-08 / 1.5e-08
  init64  regular  distinct_blocks        9.1e-15 / 1.5e-08 / 1.7e-08   9.1e-15 / 1.5e-08 / 1.7e-08
  init64  regular  d4_image               1.2e-14 / 1.7e-08 / 2.7e-08   1.2e-14 / 1.7e-08 / 2.7e-08
  init64  regular  hadamard_x3            1.7e-15 / 7.3e-08 / 0.0e+00   1.7e-15 / 7.3e-08 / 0.0e+00
  init64  regular  hadamard_diag          1.5e-15 / 9.9e-08 / 0.0e+00   1.5e-15 / 9.9e-08 / 0.0e+00
  init64  regular  pair_exact             2.0e-14 / 5.2e-08 / 1.3e-08   2.0e-14 / 5.2e-08 / 1.3e-08
  init64  regular  pair_1e-7              1.9e-14 / 3.6e-08 / 1.6e-08   1.9e-14 / 3.6e-08 / 1.6e-08
  init64  regular  pair_1e-10             1.6e-14 / 2.1e-08 / 1.5e-08   1.6e-14 / 2.1e-08 / 1.5e-08
  init64  regular  pair_1e-12             1.6e-14 / 3.8e-08 / 1.2e-08   1.6e-14 / 3.8e-08 / 1.2e-08
  init64  regular  seven_equal            1.7e-14 / 3.1e-08 / 1.3e-08   1.7e-14 / 3.1e-08 / 1.3e-08
  init64  regular  graded_2               2.0e-14 / 6.8e-08 / 9.4e-09   2.0e-14 / 6.8e-08 / 9.4e-09
  init64  regular  graded_10              2.1e-14 / 1.5e-07 / 2.0e-09   2.1e-14 / 1.5e-07 / 2.0e-09
  init64  regular  tiny_1e-12             9.7e-15 / 7.6e-08 / 1.2e-08   9.7e-15 / 7.6e-08 / 1.2e-08
  init64  regular  huge_1e12              1.0e-14 / 5.5e-08 / 1.6e-08   1.0e-14 / 5.5e-08 / 1.6e-08
  init64  regular  zero_row_col           1.4e-14 / 7.2e-09 / 1.4e-08   1.4e-14 / 7.2e-09 / 1.4e-08
  init64  regular  rank5_R12              2.0e-14 / 1.2e-07 / 6.4e-09   2.0e-14 / 1.2e-07 / 6.4e-09
  any     dup      dupany_36x16           4.3e-01 / 9.8e-01 / 2.5e-08   2.8e-15 / 5.3e-08 / 1.9e-08
  any     dup      dupany_54x34           4.1e-01 / 9.9e-01 / 2.1e-08   5.6e-15 / 3.3e-08 / 1.7e-08
  any     dup      dupany_120x100         4.0e-01 / 9.9e-01 / 1.4e-08   1.5e-14 / 1.8e-08 / 1.3e-08
  any     dup      dupany_210x190         3.8e-01 / 1.0e+00 / 6.8e-09   1.7e-14 / 4.8e-08 / 5.7e-09
  any     dup      dupany_280x260         3.8e-01 / 1.0e+00 / 8.1e-09   2.9e-14 / 4.6e-08 / 6.1e-09
  any     dup      dupany_540x520         3.8e-01 / 1.0e+00 / 3.3e-09   2.7e-14 / 5.0e-08 / 1.6e-09
  any     dup      dupany_64x700          3.8e-01 / 9.9e-01 / 2.8e-01   5.7e-15 / 1.6e-08 / 2.7e-08
  any     regular  any_perm_dup           3.8e-01 / 9.9e-01 / 1.1e-08   1.1e-14 / 4.3e-08 / 4.5e-09
  any     regular  any_kron_I2            6.0e-15 / 6.9e-08 / 1.6e-08   6.0e-15 / 6.9e-08 / 1.6e-08
  any     regular  any_distinct_blocks    6.4e-15 / 1.4e-08 / 1.1e-08   6.4e-15 / 1.4e-08 / 1.1e-08
  any     regular  any_pair_seven         1.8e-14 / 2.4e-08 / 1.1e-08   1.8e-14 / 2.4e-08 / 1.1e-08
  any     regular  any_graded_2           3.6e-14 / 7.1e-08 / 7.2e-09   3.6e-14 / 7.1e-08 / 7.2e-09
  any     regular  any_wide_pair          1.1e-14 / 1.3e-08 / 2.5e-08   1.1e-14 / 1.3e-08 / 2.5e-08
  u8      dup      dupu8_240x192          3.8e-01 / 1.0e+00 / 5.7e-09   2.0e-14 / 7.2e-08 / 5.1e-09
  u8      regular  u8_distinct_blocks     1.9e-14 / 4.0e-08 / 6.0e-09   1.9e-14 / 4.0e-08 / 6.0e-09
  u8      regular  u8_kron_I2             2.0e-14 / 5.4e-09 / 6.5e-09   2.0e-14 / 5.4e-09 / 6.5e-09

Before the fix only matrices with a repeated non-zero singular value exceeded a bar: every dup class, and three of the
regular-hard cases that are built from copies (perm_dup, kron_I2, any_perm_dup — whether a permuted or interleaved copy is
found depends on whether rounding happens to split the tridiagonal form; any_kron_I2 and u8_kron_I2 were found).  After it
no case does.  The repair stops at eigenvalues below 1e-12 lambda_0: null spaces (rank5_R12, the tails of graded_10) keep
the vectors they had before it.
"""
import functools

import numpy as np

P2_MAX = 1e-10
P3_MAX = 2e-6
P4_MAX = 1e-5
P12_ONLY = {"rank5_R12"}  # rank 5 asked for twelve: columns 5..11 span a null space, only P1 and P2 are asserted


def _noise(rng, m, n):
    return rng.integers(0, 256, size=(m, n)).astype(np.float32)


def _smooth(rng, m, n):
    i, j = np.mgrid[0:m, 0:n]
    a = 30 + 150 * i / max(m - 1, 1) + 60 * j / max(n - 1, 1) + rng.normal(size=(m, n)) * 3
    return np.clip(np.round(a), 0, 255).astype(np.float32)


def _blocks(*mats):
    M, N = sum(a.shape[0] for a in mats), sum(a.shape[1] for a in mats)
    X = np.zeros((M, N), np.float32)
    r = c = 0
    for a in mats:
        X[r:r + a.shape[0], c:c + a.shape[1]] = a
        r += a.shape[0]
        c += a.shape[1]
    return X


def hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def _spectrum(rng, M, N, s):
    """Q diag(s) W^T with Haar-like Q [M,k], W [N,k], rounded to fp32 (the reference is the SVD of the rounded matrix)"""
    k = len(s)
    Q, _ = np.linalg.qr(rng.normal(size=(M, k)))
    W, _ = np.linalg.qr(rng.normal(size=(N, k)))
    return ((Q * np.asarray(s, np.float64)) @ W.T).astype(np.float32)


def d4_image(side=128, seed=5):
    """integer image f(|y - c|, |x - c|) symmetrised over transpose and both flips"""
    rng = np.random.default_rng(seed)
    h = side // 2
    q = rng.integers(0, 256, size=(h, h))
    q = np.minimum(255, (q + q.T) // 2)  # f(a, b) = f(b, a), a = |y - c| - 1/2, b = |x - c| - 1/2
    img = np.empty((side, side), np.float32)
    img[h:, h:] = q
    img[h:, :h] = q[:, ::-1]
    img[:h, h:] = q[::-1, :]
    img[:h, :h] = q[::-1, ::-1]
    return img


def _patches(img, p=8):
    H, W = img.shape
    return np.ascontiguousarray(img.reshape(H // p, p, W // p, p).transpose(0, 2, 1, 3).reshape(-1, p * p))


# ---------------------------------------------------------------------------------------------- 64 columns (svd_init)
R64 = (2, 4, 7, 20)


def dup64_cases():
    rng = np.random.default_rng(101)
    A = _noise(rng, 100, 32)
    S = _smooth(rng, 100, 32)
    A3 = _noise(rng, 60, 21)
    X3 = np.zeros((200, 64), np.float32)  # three copies, a zero column, zero rows up to M = 200
    X3[:180, :63] = _blocks(A3, A3, A3)
    AA = _blocks(A, A)
    had = (AA.astype(np.float64) @ hadamard(64) / 8).astype(np.float32)
    assert np.array_equal(had.astype(np.float64), AA.astype(np.float64) @ hadamard(64) / 8)  # exact in fp32
    return [("dup64_noise", AA, R64), ("dup64_smooth", _blocks(S, S), R64), ("dup64_three", X3, R64),
            ("dup64_flip", _blocks(S, np.ascontiguousarray(S[::-1, ::-1])), R64), ("dup64_hadamard", had, R64)]


def regular64_cases():
    rng = np.random.default_rng(202)
    A = _noise(rng, 100, 32)
    B = _noise(rng, 100, 32)
    AA = _blocks(A, A)
    perm = rng.permutation(64)
    out = [("perm_dup", np.ascontiguousarray(AA[:, perm]), R64),
           ("kron_I2", np.kron(A, np.eye(2, dtype=np.float32)).astype(np.float32), R64),
           ("distinct_blocks", _blocks(A, B), R64),
           ("d4_image", _patches(d4_image()), (2, 4, 7, 9, 20)),
           ("hadamard_x3", (3 * hadamard(64)).astype(np.float32), (2, 7, 20)),
           ("hadamard_diag", (hadamard(64) * np.arange(1, 65)).astype(np.float32), (2, 7, 20))]
    base = 200.0 * 0.8 ** np.arange(40)
    for tag, gap in (("pair_exact", 0.0), ("pair_1e-7", 1e-7), ("pair_1e-10", 1e-10), ("pair_1e-12", 1e-12)):
        s = base.copy()
        s[3] = s[2] * (1.0 - gap)
        out.append((tag, _spectrum(rng, 200, 64, s), (2, 3, 4, 7, 20)))
    s = base.copy()
    s[1:8] = 120.0
    out.append(("seven_equal", _spectrum(rng, 200, 64, s), (2, 4, 7, 8, 20)))
    out.append(("graded_2", _spectrum(rng, 200, 64, 200.0 * 2.0 ** -np.arange(64)), (7, 20, 32)))
    out.append(("graded_10", _spectrum(rng, 200, 64, 200.0 * 10.0 ** -np.arange(40)), (7, 20, 32)))
    G = rng.normal(size=(200, 64))
    out.append(("tiny_1e-12", (G * 1e-12).astype(np.float32), (2, 7, 20)))
    out.append(("huge_1e12", (G * 1e12).astype(np.float32), (2, 7, 20)))
    Z = _noise(rng, 200, 64)
    Z[17, :] = 0
    Z[:, 40] = 0
    out.append(("zero_row_col", Z, (2, 7, 20)))
    out.append(("rank5_R12", (_noise(rng, 200, 5) @ rng.integers(-3, 4, size=(5, 64))).astype(np.float32), (12,)))
    return out


# ------------------------------------------------------------------------------ any shape (svd_topr_any / Context.svd_init)
# one size per tridiagonalisation variant of k_any_eig: 16 and 34 plain, 100 in registers with two column chunks, 190 with
# three, 260 symmetric blocked with one chunk, 520 blocked; 64 x 700: the eigen-problem on the row side
ANY_SIDES = ((36, 16), (54, 34), (120, 100), (210, 190), (280, 260), (540, 520), (64, 700))


def dup_any_cases():
    rng = np.random.default_rng(303)
    out = []
    for M, N in ANY_SIDES:
        A = _noise(rng, M // 2, N // 2)
        out.append((f"dupany_{M}x{N}", _blocks(A, A), (2, 7, 40) if N == 100 else (2, 7)))
    return out


def regular_any_cases():
    rng = np.random.default_rng(404)
    A = _noise(rng, 60, 50)
    AA = _blocks(A, A)
    s = 200.0 * 0.8 ** np.arange(40)
    s[3] = s[2]
    s[10:17] = s[10]
    return [("any_perm_dup", np.ascontiguousarray(AA[:, rng.permutation(100)]), (2, 7)),
            ("any_kron_I2", np.kron(_noise(rng, 27, 17), np.eye(2, dtype=np.float32)).astype(np.float32), (2, 7)),
            ("any_distinct_blocks", _blocks(_noise(rng, 40, 30), _noise(rng, 50, 40)), (2, 7)),
            ("any_pair_seven", _spectrum(rng, 130, 90, s), (3, 4, 12, 17)),
            ("any_graded_2", _spectrum(rng, 210, 150, 200.0 * 2.0 ** -np.arange(60)), (7, 20, 32)),
            ("any_wide_pair", _spectrum(rng, 48, 300, s), (3, 4, 7))]


# ------------------------------------------------------------------------------------------ the [M,192] uint8 route
def dup_u8_cases():
    rng = np.random.default_rng(505)
    A = _noise(rng, 120, 96)
    return [("dupu8_240x192", _blocks(A, A), (2, 7))]


def regular_u8_cases():
    rng = np.random.default_rng(606)
    return [("u8_distinct_blocks", _blocks(_noise(rng, 120, 96), _noise(rng, 120, 96)), (2, 7)),
            ("u8_kron_I2", np.kron(_noise(rng, 120, 96), np.eye(2, dtype=np.float32)).astype(np.float32), (2, 7))]


@functools.lru_cache(maxsize=None)
def cases(path, cls):
    """path: "init64" | "any" | "u8";  cls: "dup" | "regular".  Built once; the arrays are read-only."""
    table = {("init64", "dup"): dup64_cases, ("init64", "regular"): regular64_cases, ("any", "dup"): dup_any_cases,
             ("any", "regular"): regular_any_cases, ("u8", "dup"): dup_u8_cases, ("u8", "regular"): regular_u8_cases}
    out = table[(path, cls)]()
    for _, X, _ in out:
        X.setflags(write=False)
    return tuple(out)


def case_ids(path):
    """[(cls, name, R)] for pytest.mark.parametrize"""
    return [(cls, name, R) for cls in ("dup", "regular") for name, _, ranks in cases(path, cls) for R in ranks]


def get_case(path, cls, name):
    return next(X for n, X, _ in cases(path, cls) if n == name)


# ------------------------------------------------------------------------------------------------------- properties
_SVD = {}


def reference_svd(X):
    """numpy.linalg.svd of X in float64 (computed once per matrix)"""
    key = (X.shape, X.tobytes())
    if key not in _SVD:
        _SVD[key] = np.linalg.svd(X.astype(np.float64), full_matrices=False)
    return _SVD[key]


def init_metrics(X, R, u0, v0):
    """(finite, excess, p3, p4) of an initialisation (u0 [M,R], v0 [N,R]) of X: the module docstring's P1-P4"""
    M, N = X.shape
    Rc = min(R, M, N)
    _, s, _ = reference_svd(X)
    u = np.asarray(u0, np.float64)
    v = np.asarray(v0, np.float64)
    finite = bool(np.isfinite(u).all() and np.isfinite(v).all())
    if not finite:
        return False, np.inf, np.inf, np.inf
    X64 = X.astype(np.float64)
    tot = float((s ** 2).sum())
    excess = (float(((X64 - u @ v.T) ** 2).sum()) - float((s[Rc:] ** 2).sum())) / tot if tot > 0 else 0.0
    s0 = s[0] if s[0] > 0 else 1.0
    p3 = max(np.abs((v ** 2).sum(0)[:Rc] - s[:Rc]).max(), np.abs((u ** 2).sum(0)[:Rc] - s[:Rc]).max()) / s0
    keep = [r for r in range(Rc) if s[r] >= 1e-3 * s[0] and s[r] > 0]
    p4 = 0.0
    if keep:
        nrm = np.sqrt((v[:, keep] ** 2).sum(0))
        if (nrm == 0).any():
            p4 = np.inf
        else:
            Vn = v[:, keep] / nrm
            p4 = float(np.abs(Vn.T @ Vn - np.eye(len(keep))).max())
    return finite, float(excess), float(p3), p4


def check_init(X, R, u0, v0, only_p12=False):
    finite, excess, p3, p4 = init_metrics(X, R, u0, v0)
    assert finite, "P1: non-finite entries"
    assert excess <= P2_MAX, f"P2: excess {excess:.3e} above {P2_MAX:g}"
    if only_p12:
        return
    assert p3 <= P3_MAX, f"P3: column norms off by {p3:.3e} s_0 (bar {P3_MAX:g})"
    assert p4 <= P4_MAX, f"P4: |V^T V - I| = {p4:.3e} above {P4_MAX:g}"
