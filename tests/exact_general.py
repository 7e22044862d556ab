"""Exact-integer cases of the general QMF solver (lrf_qmf_decompose_ex_f32, Context.decompose_ex) from caller-given factors:
x' = safe_divide(x - w0, w1), U0 and V0 hold small integers and the elastic-net terms l1 and l2 are integers, so every product and
partial sum of CoordinateDescent.update_u is an exact integer below 2^24, the order of a sum cannot matter, and the expected
factors follow from the integer arithmetic of reference_general below and ONE fp32 division per solve.  The module owns its
arithmetic: it imports neither the oracle nor tests/exact_bcd.py.  tests/test_exact_general.py (CPU) gates it against the oracle
and the reference's own recorded factors and asserts the conditions listed here; tests/test_exact_general_gpu.py compares the
kernels with it, bit for bit.

What the generated data is for.  V0 (or, for a V-only case, U0) has columns of nz entries of +-1, so the first update divides by
nz + l2: odd numerators are rounding ties.  Small data next to l1 = 1, 2 puts numerators on and inside the soft threshold.  An
all-zero column of V0 gives (0 + eps) / (0 + eps) = 1 with l2 = 0 and 0 with l2 > 0; an all-zero matrix X gives a zero U and then
zero denominators in the whole V half.  Unbounded factors and bounds beyond int8 carry values past +-127; fractional bounds
(-3.5, 5.5) must clamp to (-3, 5).  X = w0 + d * integers with d the denominator safe_divide uses for w1 (w1 itself, or
eps * sign(w1) when |w1| < eps: CoordinateDescent hands ITS eps to safe_divide, qmf.py:105).

update_w (factor bit 2, K = 1): the factors of that iteration are exact as above; the expected pair is the least-squares line of x
on z = u v^T in exact rationals (fractions.Fraction) from the integer sums n, sum z, sum z^2, sum x, sum x z.  The kernel's fp64
sums of those integers are exact below 2^53 (asserted), the 2 x 2 solve then errs by about 4 * 2^-53 * kappa with
kappa = max(n sum z^2, (sum z)^2) / |det| (asserted <= 2^20): W is required within 1 fp32 ulp of the correctly rounded exact pair.
A constant z (det = 0 in integers) must give (mean x, 0).  The loss is sqrt(sum (x - y)^2) / (sqrt(sum x^2) + 1e-16) from exact sums.

`python tests/exact_general.py` prints the table below: per case and updated half the planned kernels (plan_any_update: the two
products a and b, then the sweep; f = folded contraction, n = ATen's native order) and the shares in per cent of the solves:
tie = the fp32 quotient ends in exactly .5, =l1 = |t| == l1 > 0, <l1 = 0 < |t| < l1, zero = b_rr + l2 == 0, clamp = the clamp
changed the value, >127 = |new| > 127.  marks (u / v): the halves that count towards the condition of that letter (t e s z c b).

case                          half kernels                        tie   =l1   <l1  zero clamp  >127  marks
rows1          B1-1x64-R8-K3     U TIL,TIL,lds+n                 12.5   8.3   4.2  12.5   0.0   0.0  tesz/ez
                                 V TIL,TILn,lds                   0.0  10.8   0.0  54.2   0.0   0.0
rows63-zero    B3-63x64-R4-K3    U TIL,TIL,lds+n                  5.2   3.5   3.3   0.0   0.0   0.0  tes/z
                                 V TIL,TIL,lds+n                  1.7   0.0   0.0  33.3   0.0   0.0
rows64         B3-64x48-R5-K3    U TIL,TIL,lds+n                 33.6   0.0   0.0  11.1   1.8   0.0  tzc/es
                                 V TIL,TIL,lds+n                  0.2   4.3  15.1   0.0   0.0   0.0
rows65-eps     B2-65x64-R9-K3    U TIL,TIL,lds                    0.0   0.0   0.0   3.7   0.0   0.0  z/
                                 V TIL,LONG,lds                   0.0   0.0   0.0   0.0   0.0   0.0
rows130-w      B2-130x64-R10-K3  U TIL,TIL,lds                   41.7   0.0   0.0   0.0   4.4   0.0  t/
                                 V TIL,LONG,lds                   0.0   0.0   0.0   0.0   0.0   0.0
r1             B2-130x64-R1-K3   U TIL,TILn,lds+n                13.3   0.0   0.0   0.0  47.2   0.0  tc/
                                 V TIL,TILn,lds+n                 0.0   0.0   0.0   0.0   0.0   0.0
issue          B2-130x16-R6-K3   U TIL,TIL,lds                   17.5  10.4  11.2   0.0   1.9   0.0  tesc/
                                 V LONG,LONG,lds+n                0.5   0.0   0.0   0.0   0.0   0.0
r2-frac        B2-400x16-R2-K3   U S4,TILn,lds                   19.1   4.5   5.0   0.0   8.7   0.0  tesc/
                                 V LONGf,LONGf,lds+n              0.0   0.0   0.0   0.0   0.0   0.0
r3-unb         B2-400x16-R3-K2   U S4,TILn,lds                   39.1   0.0   0.0   0.0   0.0   0.0  t/
                                 V LONGf,LONGf,lds+n              0.0   0.0   0.0   0.0   0.0   0.0
r4-wide        B2-140x32-R4-K2   U TIL,TIL,lds                   31.5   0.0   0.0   0.0  35.2  90.0  tcb/
wide-uv        B2-9x16-R2-K2     U TILn,TILn,lds+n               33.3   0.0   0.0   0.0   0.0  34.7  tb/
                                 V TILn,TILn,lds+n                0.0   0.0   0.0   0.0   0.0   0.0
r17-big        B2-130x100-R17-K2 U BIG,TIL,lds                   42.9   0.0   0.0   0.0   0.0   0.0  t/
                                 V BIG,TIL,lds                    0.0   0.0   0.0   0.0   0.0   0.0
r18-w4         B2-130x96-R18-K2  U BIG,TIL,lds                   20.7   9.4  22.5   0.0   0.0   0.0  tes/
                                 V BIG,TIL,lds                    0.1   0.0   0.0   0.0   0.0   0.0
r64            B2-100x40-R64-K2  U BIG,TIL,lds                   46.8   0.0   0.0   0.0  11.5   0.0  tc/
                                 V TIL,TIL,lds                    0.0   0.0   0.0   0.0   0.0   0.0
r65            B2-100x40-R65-K2  U BIG,BIG,lds                   16.7   7.4  35.0   0.0   4.0   0.0  tes/
                                 V TIL,BIG,lds                    0.0   0.0   0.0   0.0   0.0   0.0
r129           B1-90x70-R129-K2  U BIG,BIG,lds                   45.1   0.0   0.0   0.0  15.4   0.0  tc/
                                 V BIG,BIG,lds                    0.0   0.0   0.0   0.0   0.0   0.0
r629           B1-70x66-R629-K1  U BIG,BIG,lds                   43.4   0.0   0.0   0.0  13.2   0.0  tc/
                                 V BIG,BIG,lds                    0.0   0.0   0.0   0.0   0.0   0.0
r630           B1-70x66-R630-K1  U BIG,BIG,nolds                 43.5   0.0   0.0   0.0  13.3   0.0  tc/
                                 V BIG,BIG,nolds                  0.0   0.0   0.0   0.0   0.0   0.0
short8         B2-260x24-R7-K2   U S8,TIL,lds                    20.8   8.4  21.6   0.0   0.0   0.0  tes/
                                 V TIL,LONG,lds+n                 0.0   0.0   0.0   0.0   0.0   0.0
short16        B2-256x64-R12-K2  U S16,TIL,lds                   43.5   0.0   0.0   4.2   0.0   0.0  tz/
                                 V TIL,LONG,lds                   0.0   0.0   0.0   0.0   0.0   0.0
native-u       B2-5x16-R3-K3     U TILn,TILn,lds+n               16.7  16.7  16.7   0.0   4.4   0.0  tesc/
long-nofold    B2-130x192-R12-K2 U TIL,LONG,lds                   9.7   0.0   0.0   0.0   0.0   0.0  t/
                                 V TIL,LONG,lds                   0.0   0.0   0.0   0.0   0.0   0.0
v-unb          B2-17x64-R2-K3    V TIL,TILn,lds+n                48.0   0.0   0.0   0.0   0.0  84.8  /tb
v-frac         B2-16x64-R3-K3    V TIL,TILn,lds+n                17.7   5.2   4.4   0.0  14.3   0.0  /tesc
v-wide         B4-17x64-R6-K3    V TIL,TIL,lds+n                 30.7   0.0   0.0   0.0  35.2  89.3  /tcb
k0             B2-17x16-R3-K0
zero-col       B2-130x64-R5-K1   U TIL,TIL,lds                   38.5   0.0   0.0  20.0   0.0   0.0  tz/
                                 V TIL,LONG,lds+n                 0.2   0.0   0.0   0.0   0.0   0.0
zero-col-l2    B2-130x64-R5-K1   U TIL,TIL,lds                   14.6   0.0   0.0   0.0   0.0   0.0  t/z
                                 V TIL,LONG,lds+n                 0.0   0.0   0.0  20.0   0.0   0.0
big-fold       B2-400x100-R18-K1 U BIG,TIL,lds                   49.5   0.0   0.0   0.0   0.9   0.0  t/
                                 V BIGf,TILf,lds                  0.0   0.0   0.0   0.0   0.0   0.0
tiled-fold     B2-400x40-R18-K1  U BIG,TIL,lds                   48.5   0.0   0.0   0.0   2.5   0.0  t/
                                 V TILf,TILf,lds                  0.0   0.0   0.0   0.0   0.0   0.0
safe-div-eps   B2-48x16-R3-K2    U TIL,TILn,lds+n                 0.0   0.0   0.0   0.0   0.0   0.0  /
                                 V TIL,TIL,lds+n                  0.0   0.0   0.0   0.0   0.0   0.0
eps-above-one  B2-17x16-R3-K2    U TIL,TILn,lds+n                11.8   0.0   0.0   0.0   0.0   0.0  /
                                 V TIL,TILn,lds+n                 0.5   0.0   0.0   0.0   0.0   0.0
w-v            B2-40x32-R3-K1    V TIL,TILn,lds+n                 0.0   0.0   0.0   0.0   0.0   0.0  /
w-uv           B2-40x32-R3-K1    U TIL,TILn,lds+n                51.7   0.0   0.0   0.0   0.0   0.0  t/
                                 V TIL,TILn,lds+n                 0.0   0.0   0.0   0.0   0.0   0.0
w-z0           B2-9x8-R2-K1
w-zc           B2-9x8-R1-K1
"""
import math
import zlib
from fractions import Fraction

import numpy as np

F32 = np.float32
LIMIT = float(1 << 24)
LIMIT53 = 1 << 53
KAPPA_MAX = float(1 << 20)
X_GRID = 4  # every x is a multiple of 1 / X_GRID (asserted): the scale that makes the sums of update_w and of the loss integers
STAT_KEYS = ("solves", "ties", "thr_eq", "thr_in", "zero_den", "clamped", "big")
MARK_KEYS = dict(t="ties", e="thr_eq", s="thr_in", z="zero_den", c="clamped", b="big")


def new_stats():
    return {h: dict.fromkeys(STAT_KEYS, 0) for h in "uv"}


def safe_divide_den(w1, eps):
    """the denominator of safe_divide(x - w0, w1, eps) (factorization/utils.py:18-33) as an fp32 number"""
    w1, e = F32(w1), F32(eps)
    return float(e * np.sign(w1)) if abs(w1) < e else float(w1)


def terms(opts, M, N):
    """(l1_u, l2_u, l1_v, l2_v) of CoordinateDescent.forward (qmf.py:154-157): Python floats, rounded to fp32; asserted integers"""
    l2 = opts.get("l2", 0.0)
    l2 = tuple(l2) if isinstance(l2, (tuple, list)) else (l2, l2)
    ratio = opts.get("l1_ratio", 0.0)
    out = (l2[0] * ratio * N, l2[1] * ratio * M, l2[0] * (1 - ratio) * N, l2[1] * (1 - ratio) * M)
    out = tuple(float(F32(t)) for t in out)
    assert all(t == int(t) and t >= 0 for t in out), ("l1 / l2 are not integers", out)
    return out[0], out[2], out[1], out[3]


def clamp_bounds(opts):
    """QMF._project (qmf.py:191-195): [ceil(lo), floor(hi)] when bounded, None otherwise"""
    b = opts.get("bounds", (None, None))
    if b is None or tuple(b) == (None, None):
        return None
    return float(math.ceil(b[0])), float(math.floor(b[1]))


def _half(x, u, v, l1, l2, eps, bounds, st, trace=None):
    """One update_u (qmf.py:103-126) of every matrix: x [B,I,D], old u [B,I,R], v [B,D,R], float64 holding integers"""
    R = u.shape[-1]
    a, b = x @ v, v.transpose(0, 2, 1) @ v
    assert (np.abs(x) @ np.abs(v)).max(initial=0) < LIMIT, "|x| |v| reaches 2^24"
    assert (np.abs(v).transpose(0, 2, 1) @ np.abs(v)).max(initial=0) + l2 < LIMIT, "b_rr + l2 reaches 2^24"
    u = u.copy()
    e32 = F32(eps)
    for r in range(R):
        bb = b[:, :, r].copy()
        den = bb[:, r] + l2
        bb[:, r] = 0  # the new columns < r and the old columns > r
        assert (np.abs(a[:, :, r]) + (np.abs(u) @ np.abs(bb)[:, :, None])[:, :, 0]).max(initial=0) < LIMIT, "|a_r| + |u_j| |b_jr| reaches 2^24"
        t = a[:, :, r] - (u @ bb[:, :, None])[:, :, 0]
        num = np.sign(t) * np.maximum(np.abs(t) - l1, 0.0)  # soft_thresholding (utils.py:36-40)
        den = np.broadcast_to(den[:, None], num.shape)
        q = (num.astype(F32) + e32) / (den.astype(F32) + e32)  # one IEEE fp32 division
        assert np.isfinite(q).all()
        rq = np.rint(q)
        new = rq if bounds is None else np.clip(rq, F32(bounds[0]), F32(bounds[1]))
        near = np.ones(q.shape, bool) if bounds is None else np.abs(q) < max(abs(bounds[0]), abs(bounds[1])) + 2
        st["solves"] += t.size
        st["ties"] += int(((np.abs(q - np.floor(q)) == F32(0.5)) & near).sum())
        st["thr_eq"] += int(((np.abs(t) == l1) & (l1 > 0)).sum())
        st["thr_in"] += int(((np.abs(t) > 0) & (np.abs(t) < l1)).sum())
        st["zero_den"] += int((den == 0).sum())
        st["clamped"] += int((new != rq).sum())
        st["big"] += int((np.abs(new) > 127).sum())
        u[:, :, r] = new
        if trace is not None:
            trace.append((t.copy(), den.copy(), q.copy()))
    assert np.abs(u).max(initial=0) < LIMIT
    return u


def exact_line(x, z):
    """The least-squares line of x on z over all elements, in exact rationals: dict(w0, w1: Fraction, kappa: float or None for a
    constant z, for which the line is (mean x, 0)).  Asserts that the fp64 sums of the kernel are exact (below 2^53 on the grid of
    x) and kappa <= 2^20."""
    xs = np.rint(np.asarray(x, np.float64).ravel() * X_GRID).astype(np.int64)
    assert np.array_equal(xs / X_GRID, np.asarray(x, np.float64).ravel()), "x is off the 1 / X_GRID grid"
    zs = np.asarray(z, np.float64).ravel().astype(np.int64)
    n = int(xs.size)
    for s in (np.abs(zs).sum(), (zs * zs).sum(), np.abs(xs).sum(), (np.abs(xs) * np.abs(zs)).sum()):
        assert int(s) < LIMIT53, "a sum of update_w reaches 2^53"
    sz, szz, sx, sxz = int(zs.sum()), int((zs * zs).sum()), int(xs.sum()), int((xs * zs).sum())
    # the products of the 2 x 2 solve too: n sum z^2 and (sum z)^2 exact in fp64 make det = 0 exact for a constant z
    for s in (n * szz, sz * sz, n * int((np.abs(xs) * np.abs(zs)).sum()), int(np.abs(zs).sum()) * int(np.abs(xs).sum())):
        assert s < LIMIT53, "a product of update_w's solve reaches 2^53"
    det = n * szz - sz * sz
    if det == 0:
        return dict(w0=Fraction(sx, n * X_GRID), w1=Fraction(0), kappa=None)
    kappa = max(n * szz, sz * sz) / abs(det)
    assert kappa <= KAPPA_MAX, ("update_w is ill-conditioned", kappa)
    w1 = Fraction(n * sxz - sz * sx, det * X_GRID)
    return dict(w0=Fraction(sx, n * X_GRID) - w1 * Fraction(sz, n), w1=w1, kappa=kappa)


def within_one_ulp(got, want):
    """got (fp32) within 1 fp32 ulp of the correctly rounded Fraction `want` (an exact zero is required exactly)"""
    w = F32(float(want))
    if want == 0:
        return float(got) == 0.0
    return abs(float(got) - float(w)) <= float(np.spacing(np.abs(w)))


def line_error(x, z, w):
    """How far the line w = (w0, w1) is from the least-squares line of x on z, in what a least-squares solver controls: (|A dw|_2,
    bound) with A = [1, z], dw = w - the exact line, bound = 2 m u (|A|_F |w|_2 + |x|_2), u = 2^-24, m = the number of elements — the
    first-order error of a backward-stable fp32 solver of an m x 2 problem (Householder QR: a constant of order m n u on the data;
    the conditioning term kappa u |r| is left out, so the bound is on the strict side).  It holds for every draw of the reference's
    fp32 lstsq, and for a constant z too, where the pair is large and only its reconstruction w0 + w1 c is determined."""
    x, z = np.asarray(x, np.float64).ravel(), np.asarray(z, np.float64).ravel()
    line = exact_line(x, z)
    d0, d1 = float(w[0]) - float(line["w0"]), float(w[1]) - float(line["w1"])
    m = x.size
    a_norm = math.sqrt(m + float((z * z).sum()))
    return float(np.linalg.norm(d0 + d1 * z)), 2 * m * 2.0 ** -24 * (a_norm * math.hypot(float(w[0]), float(w[1])) + float(np.linalg.norm(x)))


def bits(a):
    """the bit patterns of an fp32 array: what "bit for bit" compares (-0 is not +0)"""
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def check_w(case, got, W, b, who):
    """The rule for the pair (w0, w1) `who` returned for matrix b: the initial pair, unchanged, while bit 2 is clear; else within
    1 fp32 ulp of the correctly rounded exact line W[b] ((mean x, 0) for a constant z)"""
    if W is None:
        assert [float(t) for t in got] == [float(F32(t)) for t in case.opts.get("w", (0.0, 1.0))], (case.id, b, who, got)
    else:
        assert within_one_ulp(got[0], W[b]["w0"]) and within_one_ulp(got[1], W[b]["w1"]), \
            (case.id, b, who, [float(t) for t in got], float(W[b]["w0"]), float(W[b]["w1"]), W[b]["kappa"])


def exact_loss(x, u, v, w=None):
    """QMF.loss of ONE matrix (qmf.py:225-227, utils.py:12-15) from exact integer sums: fp32(sqrt(sum (x - y)^2) /
    (sqrt(sum x^2) + 1e-16)), y = w0 + w1 u v^T; x and y on the 1 / X_GRID grid, the sums below 2^53"""
    z = np.asarray(u, np.float64) @ np.asarray(v, np.float64).T
    assert (np.abs(np.asarray(u, np.float64)) @ np.abs(np.asarray(v, np.float64)).T).max(initial=0) < LIMIT
    y = z if w is None else float(w[0]) + float(w[1]) * z
    xs, ys = (np.asarray(t, np.float64) * X_GRID for t in (x, y))
    assert np.array_equal(xs, np.rint(xs)) and np.array_equal(ys, np.rint(ys)), "x or y is off the 1 / X_GRID grid"
    assert max(np.abs(xs).max(), np.abs(ys).max()) < LIMIT, "x or y is not an fp32 number"
    num = sum(int(d) ** 2 for d in (xs - ys).ravel())
    den = sum(int(t) ** 2 for t in xs.ravel())
    assert num < LIMIT53 and den < LIMIT53, "a sum of the loss reaches 2^53"
    with np.errstate(over="ignore"):
        return F32((math.sqrt(num) / X_GRID) / (math.sqrt(den) / X_GRID + 1e-16))


def reference_general(X, U0, V0, K, opts, trace=None):
    """K iterations of CoordinateDescent.forward (qmf.py:149-164) behind QMF._project from (U0, V0) and the pair opts["w"]:
    X [B,M,N] float64 (w0 + d * integers), U0 [B,M,R], V0 [B,N,R] float64 holding integers; opts: bounds, l2, l1_ratio, factor,
    eps, w.  Returns fp32 (U, V), W (None while bit 2 is clear: the pair stays; else per matrix the dict of exact_line), and per
    half the counts STAT_KEYS.  Asserts, from sums of absolute values, that every sum stays below 2^24, and that l1, l2 and
    x' = safe_divide(x - w0, w1) are integers: a case that breaks this is a bad case, not a finding.
    trace: a list that receives (half, t, den, q) of every column solved."""
    X, U0, V0 = (np.asarray(t, np.float64) for t in (X, U0, V0))
    for t in (U0, V0):
        assert np.array_equal(t, np.rint(t))
    B, M, N = X.shape
    factor = set(opts.get("factor", (0, 1, 2)))
    eps = opts.get("eps", 1e-16)
    w0, w1 = opts.get("w", (0.0, 1.0))
    l1_u, l2_u, l1_v, l2_v = terms(opts, M, N)
    bounds = clamp_bounds(opts)
    assert 2 not in factor or K == 1, "update_w is exact for the iteration that precedes it only"
    xp = (X - float(F32(w0))) / safe_divide_den(w1, eps)
    assert np.array_equal(xp, np.rint(xp)), "x' = safe_divide(x - w0, w1) is not an integer"
    xt = np.ascontiguousarray(xp.transpose(0, 2, 1))
    st = new_stats()
    u, v = U0.copy(), V0.copy()
    for _ in range(K):
        for half, on in (("u", 0 in factor), ("v", 1 in factor)):
            if on:
                tr = None if trace is None else []
                if half == "u":
                    u = _half(xp, u, v, l1_u, l2_u, eps, bounds, st["u"], tr)
                else:
                    v = _half(xt, v, u, l1_v, l2_v, eps, bounds, st["v"], tr)
                if trace is not None:
                    trace.extend((half,) + c for c in tr)
    W = None
    if 2 in factor and K > 0:
        assert (np.abs(u) @ np.abs(v).transpose(0, 2, 1)).max(initial=0) < LIMIT, "|u| |v|^T reaches 2^24"
        W = [exact_line(X[b], u[b] @ v[b].T) for b in range(B)]
    return u.astype(F32), v.astype(F32), W, st


def explain(case, inputs, b, half, i, r):
    """What the reference solved LAST at entry (i, r) of factor `half` of matrix b: for the message of a failed comparison"""
    X, U0, V0 = (t[b:b + 1] for t in inputs)
    trace = []
    u, v, _, _ = reference_general(X, U0, V0, case.K, case.opts, trace)
    mine = [c for c in trace if c[0] == half]
    if not mine:
        return f"factor {half} is not updated: expected the initial value {(u if half == 'u' else v)[0, i, r]!r}"
    R = U0.shape[-1]
    _, t, den, q = mine[len(mine) - R + r]
    l1 = terms(case.opts, case.M, case.N)[0 if half == "u" else 2]
    kind = [k for k, on in (("zero denominator", den[0, i] == 0), ("tie", abs(q[0, i] - np.floor(q[0, i])) == 0.5),
                            ("on the l1 threshold", l1 > 0 and abs(t[0, i]) == l1), ("inside the l1 threshold", 0 < abs(t[0, i]) < l1)) if on]
    return (f"t = {int(t[0, i])}, l1 = {int(l1)}, b_rr + l2 = {int(den[0, i])}, q = {q[0, i]!r} ({', '.join(kind) or 'plain'}), "
            f"expected {(u if half == 'u' else v)[0, i, r]!r}")


def _factor0(rng, kind, B, rows, R):
    """an initial factor [B, rows, R]: ["uniform", lo, hi] | ["sparse", nz]: columns of nz entries of +-1 | ["const", c]"""
    if kind[0] == "uniform":
        return rng.integers(kind[1], kind[2] + 1, (B, rows, R)).astype(np.float64)
    if kind[0] == "const":
        return np.full((B, rows, R), float(kind[1]))
    nz = kind[1]
    where = np.argsort(rng.random((B, rows, R)), axis=1)[:, :nz]  # nz distinct rows per column
    F = np.zeros((B, rows, R))
    np.put_along_axis(F, where, rng.integers(0, 2, where.shape) * 2.0 - 1.0, axis=1)
    return F


def generate(seed, B, M, N, R, x, u0, v0, w=(0.0, 1.0), eps=1e-16, zero_v=False, zero_matrix=False):
    """Seeded inputs (float64): X = w0 + d * (integers uniform in [x[0], x[1]]), d = the denominator of safe_divide for (w1, eps);
    zero_matrix: X of the batch's second matrix is all zero (w = (0, 1) only); u0, v0: see _factor0; zero_v: column R // 2 of V0
    is all zero"""
    rng = np.random.default_rng(seed)
    Xi = rng.integers(x[0], x[1] + 1, (B, M, N)).astype(np.float64)
    X = float(F32(w[0])) + safe_divide_den(w[1], eps) * Xi
    if zero_matrix:
        assert tuple(w) == (0.0, 1.0) and B > 1
        X[1] = 0.0
    U0, V0 = _factor0(rng, u0, B, M, R), _factor0(rng, v0, B, N, R)
    if zero_v:
        V0[:, :, R // 2] = 0.0
    assert np.array_equal(X.astype(F32), X)
    return X, U0, V0


class Case:
    """name, (B, M, N, R, K), the solver's options (opts: bounds, l2, l1_ratio, factor, eps, w — the keywords of reference_general,
    of oracle.bcd_ex and, with w as w_init, of Context.decompose_ex) and the generator's arguments; marks = (u, v): the letters of
    MARK_KEYS whose condition that half of the case counts towards"""

    def __init__(self, name, B, M, N, R, K, x, marks=("", ""), u0=None, v0=("sparse", 2), zero_v=False, zero_matrix=False, **opts):
        self.name, self.B, self.M, self.N, self.R, self.K = name, B, M, N, R, K
        opts.setdefault("factor", (0, 1))
        self.opts = opts
        if u0 is None:  # uniform in the bounds, at most +-8
            b = clamp_bounds(opts) or (-8.0, 8.0)
            u0 = ("uniform", int(max(b[0], -8)), int(min(b[1], 8)))
        self.gen = dict(x=list(x), u0=list(u0), v0=list(v0), w=list(opts.get("w", (0.0, 1.0))), eps=opts.get("eps", 1e-16),
                        zero_v=zero_v, zero_matrix=zero_matrix)
        self.marks = dict(u=marks[0], v=marks[1])
        self.shape = f"B{B}-{M}x{N}-R{R}-K{K}"
        self.id = f"{name}-{self.shape}"
        self.seed = zlib.crc32(self.id.encode())

    def inputs(self):
        return generate(self.seed, self.B, self.M, self.N, self.R, **self.gen)

    def halves(self):
        """the halves an iteration updates, as (name, trans)"""
        f = set(self.opts["factor"])
        return [h for h, bit in ((("u", False), 0), (("v", True), 1)) if bit in f] if self.K > 0 else []

    def args(self):
        """what tools/gen_exact_general.py records next to the reference's factors"""
        o = {k: (list(v) if isinstance(v, tuple) else v) for k, v in self.opts.items()}
        return dict(id=self.id, seed=self.seed, B=self.B, M=self.M, N=self.N, R=self.R, K=self.K, opts=o, gen=self.gen)


W_HALF, W_FOUR = (3.0, 0.5), (-7.0, 4.0)
CASES = [
    # rows per sweep 1, 63, 64, 65, 130 (U half; 64, 48, 16 in the V half); ranks 8, 4, 5, 9, 10 on ATen's native order and MKL's
    Case("rows1", 1, 1, 64, 8, 3, (0, 6), ("tesz", "ez"), zero_v=True, bounds=(-3, 5), l2=(1 / 32, 1.0), l1_ratio=1.0),
    Case("rows63-zero", 3, 63, 64, 4, 3, (0, 6), ("tes", "z"), zero_matrix=True, bounds=(-16, 15), l2=(1 / 16, 0.0), l1_ratio=0.5),
    Case("rows64", 3, 64, 48, 5, 3, (0, 3), ("tzc", "es"), zero_v=True, bounds=(-2, 2), l2=(0.0, 1 / 16), l1_ratio=1.0),
    Case("rows65-eps", 2, 65, 64, 9, 3, (0, 140), ("z", ""), zero_v=True, eps=0.5),
    Case("rows130-w", 2, 130, 64, 10, 3, (-20, 20), ("t", ""), bounds=(-16, 15), w=W_HALF),
    Case("r1", 2, 130, 64, 1, 3, (0, 40), ("tc", ""), bounds=(-16, 15)),
    # the issue's prototype (l2 on the U half only: 130 / 8 is no integer)
    Case("issue", 2, 130, 16, 6, 3, (0, 6), ("tesc", ""), bounds=(-3, 5), l2=(1 / 8, 0.0), l1_ratio=1.0),
    # 400 x 16: k_any_prod_thin_short<4>, a folded k_any_prod_thin_long in the V half, and any_term2's early returns R - 1 = 1, 2
    Case("r2-frac", 2, 400, 16, 2, 3, (0, 8), ("tesc", ""), bounds=(-3.5, 5.5), l2=(1 / 8, 0.0), l1_ratio=1.0),
    Case("r3-unb", 2, 400, 16, 3, 2, (0, 40), ("t", "")),
    Case("r4-wide", 2, 140, 32, 4, 2, (-2500, 2500), ("tcb", ""), bounds=(-1000, 1000), factor=(0,)),
    Case("wide-uv", 2, 9, 16, 2, 2, (-300, 300), ("tb", ""), bounds=(-1000, 1000)),
    # ranks 17, 18 (the unrolled eight, twice, and a tail of either parity) on k_any_prod_big; 64, 65, 129: fetch_b's guards
    Case("r17-big", 2, 130, 100, 17, 2, (0, 12), ("t", ""), bounds=(-16, 15)),
    Case("r18-w4", 2, 130, 96, 18, 2, (-6, 6), ("tes", ""), bounds=(-16, 15), w=W_FOUR, l2=(1 / 32, 0.0), l1_ratio=1.0),
    Case("r64", 2, 100, 40, 64, 2, (0, 6), ("tc", ""), bounds=(-3, 5)),
    Case("r65", 2, 100, 40, 65, 2, (-10, 10), ("tes", ""), bounds=(-4, 4), l2=(1 / 8, 0.0), l1_ratio=1.0),
    Case("r129", 1, 90, 70, 129, 2, (0, 6), ("tc", ""), bounds=(-3, 3)),
    # the diagonal of b in LDS up to rank 629, from global memory above
    Case("r629", 1, 70, 66, 629, 1, (0, 4), ("tc", ""), bounds=(-2, 2)),
    Case("r630", 1, 70, 66, 630, 1, (0, 4), ("tc", ""), bounds=(-2, 2)),
    # the other thin products
    Case("short8", 2, 260, 24, 7, 2, (-6, 6), ("tes", ""), l2=(1 / 8, 0.0), l1_ratio=1.0),
    Case("short16", 2, 256, 64, 12, 2, (0, 12), ("tz", ""), zero_v=True, bounds=(-16, 15)),
    Case("native-u", 2, 5, 16, 3, 3, (0, 8), ("tesc", ""), bounds=(-3, 5), factor=(0,), l2=(1 / 8, 0.0), l1_ratio=1.0),
    Case("long-nofold", 2, 130, 192, 12, 2, (0, 12), ("t", ""), v0=("sparse", 6), bounds=(-16, 15)),
    # V alone, from U0 columns of two entries of +-1: dense ties, the threshold, clamps and values past +-127 in a V half
    Case("v-unb", 2, 17, 64, 2, 3, (0, 2000), ("", "tb"), u0=("sparse", 2), v0=("uniform", -3, 3), factor=(1,)),
    Case("v-frac", 2, 16, 64, 3, 3, (0, 12), ("", "tesc"), u0=("sparse", 2), v0=("uniform", -3, 3), zero_matrix=True, factor=(1,),
         bounds=(-3.5, 5.5), l2=(0.0, 1 / 8), l1_ratio=1.0),
    Case("v-wide", 4, 17, 64, 6, 3, (-2500, 2500), ("", "tcb"), u0=("sparse", 2), v0=("uniform", -3, 3), factor=(1,), bounds=(-1000, 1000)),
    # K = 0 returns the initial factors; an all-zero column of V0 with l2 = 0 (ones) and with l2 > 0 (zeros)
    Case("k0", 2, 17, 16, 3, 0, (0, 6), bounds=(-3, 5)),
    Case("zero-col", 2, 130, 64, 5, 1, (0, 12), ("tz", ""), zero_v=True, bounds=(-16, 15)),
    Case("zero-col-l2", 2, 130, 64, 5, 1, (0, 12), ("t", "z"), zero_v=True, bounds=(-16, 15), l2=(1 / 16, 0.0)),
    # contractions over 400 = two blocks of 384 on k_any_prod_big and k_any_prod
    Case("big-fold", 2, 400, 100, 18, 1, (0, 6), ("t", ""), bounds=(-8, 7)),
    Case("tiled-fold", 2, 400, 40, 18, 1, (0, 6), ("t", ""), bounds=(-8, 7)),
    # |w1| = 0.25 < eps = 0.5: safe_divide divides by eps, CoordinateDescent's own (qmf.py:105)
    Case("safe-div-eps", 2, 48, 16, 3, 2, (-12, 12), ("", ""), bounds=(-16, 15), w=(3.0, 0.25), eps=0.5),
    # the same for the default pair (0, 1) and eps = 2: x' = x / 2
    Case("eps-above-one", 2, 17, 16, 3, 2, (-12, 12), ("", ""), bounds=(-16, 15), eps=2.0),
]
# update_w, K = 1: from a dyadic pair, and the two degenerate lines z == 0 and z == 3
W_CASES = [
    Case("w-v", 2, 40, 32, 3, 1, (-20, 20), u0=("uniform", -3, 3), v0=("uniform", -3, 3), factor=(1, 2), w=W_HALF),
    Case("w-uv", 2, 40, 32, 3, 1, (-6, 6), ("t", ""), bounds=(-16, 15), factor=(0, 1, 2), w=W_FOUR),
    Case("w-z0", 2, 9, 8, 2, 1, (0, 40), u0=("const", 0), v0=("uniform", -3, 3), factor=(2,)),
    Case("w-zc", 2, 9, 8, 1, 1, (0, 40), u0=("const", 1), v0=("const", 3), factor=(2,)),
]
ALL = CASES + W_CASES
# tools/gen_exact_general.py records the reference's own results of these in tests/golden/exact_general.npz: the ten cases of
# the fewest elements that run an update (and the two that prove safe_divide's eps), and the update_w cases.  Of the update_w
# cases U and V only: the reference's fp32 torch.linalg.lstsq gives another pair from run to run, also at one thread (seen: 1 to
# 242 fp32 ulps from the exact line; for z == 3 pairs of either sign), so its W is judged when the tool runs (line_error) and not kept
GOLDEN_CASES = sorted([c for c in CASES if c.K > 0], key=lambda c: c.B * (c.M * c.N + (c.M + c.N) * c.R))[:10]
GOLDEN_CASES += [c for c in CASES if c.name in ("safe-div-eps", "eps-above-one") and c not in GOLDEN_CASES] + W_CASES
# the loss: rows 1, 64, 65 and a batch of three among them
LOSS_CASES = [c for c in ALL if c.name in ("rows1", "rows64", "rows65-eps", "rows63-zero", "issue", "w-uv")]
LOSS_W = (3.0, 0.5)


def share(st, key="ties"):
    return 100.0 * st[key] / max(st["solves"], 1)


PROD_SHORT = dict(THIN_LONG="LONG", THIN_SHORT4="S4", THIN_SHORT8="S8", THIN_SHORT16="S16", BIG="BIG", TILED="TIL")
GS_SHORT = dict(GS_I8="i8", GS_F32_LDS="lds", GS_F32_NOLDS="nolds")


def kernels(plan):
    """(a, b, sweep) of plan_any_update as dicts (tests/test_any_plan.py) -> 'S4,TILn,lds+n'"""
    a, b, g = plan
    p = lambda d: PROD_SHORT[d["k"]] + ("f" if d["fold"] else "") + ("n" if d["native"] else "")
    return f"{p(a)},{p(b)},{GS_SHORT[g['k']]}" + ("+n" if g["native_gs"] else "")


def describe(case, plans, st):
    """the case's lines of the docstring's table; plans: {half: plan_any_update of it}"""
    lines = []
    head = f"{case.name:14s} {case.shape:17s}"
    marks = f"{case.marks['u']}/{case.marks['v']}"
    for h, _ in case.halves():
        s = st[h]
        f = " ".join(f"{share(s, k):5.1f}" for k in STAT_KEYS[1:])
        lines.append(f"{head} {h.upper()} {kernels(plans[h]):28s} {f}" + (f"  {marks}" if head.strip() else ""))
        head = " " * 32
    return lines or [head.rstrip()]


if __name__ == "__main__":
    import ctypes
    import os
    import subprocess
    import tempfile
    import test_any_plan as P
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libany_plan_test.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", so, os.path.join(P.CSRC, "lrf_plan.cpp"),
                               os.path.join(here, "any_plan_shim.cpp")])
        lib = ctypes.CDLL(so)
        print(f"{'case':29s} half {'kernels':28s}   tie   =l1   <l1  zero clamp  >127  marks")
        for c in ALL:
            st = reference_general(*c.inputs(), c.K, c.opts)[3]
            plans = {h: P.update(lib, c.B, c.M, c.N, c.R, trans) for h, trans in c.halves()}
            print("\n".join(line.rstrip() for line in describe(c, plans, st)))
