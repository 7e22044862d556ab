"""Exact-integer cases of the BCD from caller-given factors (lrf_qmf_bcd_f32, Context.bcd): X, U0 and V0 hold small integers, so
every product and partial sum of CoordinateDescent.update_u is an exact integer below 2^24, the order of a sum cannot matter, and
the expected factors follow from the integer arithmetic of reference_bcd below, which shares no code with the oracle.
tests/test_exact_bcd.py (CPU) gates it against the oracle and the reference's own recorded factors and checks the conditions
listed here; tests/test_exact_bcd_gpu.py compares every kernel the table plans with it, bit for bit.

What the generated data is for: with V0 columns of nz entries of +-1 the first U update divides by nz — every odd numerator is a
rounding tie when nz = 2, and num = nz (k + 1/2) is one for nz = 4, 6, 10; the reciprocal 1 / nz is exact for 2 and 4 (q~ is the
tie itself) and rounded for 6 and 10 (q~ lands an ulp or two beside it: the case the kernels' threshold fthr exists for).  Later
iterations and the V halves divide by the column sums of squares of small integer factors; narrow bounds and small M keep those
small and the ties dense.  An all-zero column of V0 gives (0 + eps) / (0 + eps) = 1; bounds narrower than the data give clamps.

`python tests/exact_bcd.py` prints the table below from the cases (plan_bcd with first_mode = the caller's U0 and default
settings: first / later = the U-update kernel of iteration 1 / of iterations >= 2; p = one persistent launch k_bcd_p<f16, np32>
takes iterations 2..K) and the measured shares per half in per cent of the solves: exact ties with |q| < mx + 2, solves with a
zero denominator, values the clamp changed.  u>=2: the ties of the U halves of iterations 2..K alone, the ones the int8-U kernels see.

case                                           first / later kernel                     tie  zero clamp                  tie  zero clamp  marks
B1-M1-R8-K3-(-3,5)-nz2                1 blocks k_bcd<8> / k_bcd<8>                  U  12.5   4.2   8.3 (u>=2   0.0)  V   5.3   0.0   0.0  vzc
B2-M17-R12-K3-(-4,4)-nz2              2 blocks k_bcd<16> / k_bcd<16>                U  23.9   0.0   0.2 (u>=2  14.5)  V   5.1   0.0   0.0  v
B3-M17-R20-K3-(-3,5)-nz2              3 blocks k_bcd_mid / k_bcd_mid                U  26.8   0.6   0.5 (u>=2  17.5)  V   4.1   0.0   0.0  vc
B2-M48-R20-K3-(-4,4)-nz6              2 blocks k_bcd_mid / k_bcd_mid                U   9.3   0.0   0.4 (u>=2   5.8)  V   0.2   0.0   0.0  c
B3-M130-R1-K3-(-16,15)-nz2            3 blocks k_bcd<8> / k_bcd<8>                  U  43.8   0.0   7.8 (u>=2  38.6)  V   0.0   0.0   0.0  c
B3-M130-R5-K4-(-16,15)-nz4            3 blocks k_bcd<8> / k_bcd<8>                  U  13.6   5.0   0.0 (u>=2  11.2)  V   0.2   0.0   0.0  z
B4-M400-R8-K3-(-16,15)-nz2            8 blocks k_bcd<8> / k_bcd<8>                  U  23.5   0.0   0.0 (u>=2  10.0)  V   1.8  22.9   0.0  vz
B2-M400-R8-K3-(-128,127)-nz6          4 blocks k_bcd<8> / k_bcd<8>                  U   9.7   2.1   0.0 (u>=2   6.1)  V   0.0   0.0   0.0
B2-M384-R12-K3-(-16,15)-nz10          2 blocks k_bcd<16> / k_bcd<16>                U   6.6   2.8   0.0 (u>=2   5.2)  V   0.0   0.0   0.0  z
B2-M400-R16-K3-(-32,31)-nz4           4 blocks k_bcd<16> / k_bcd<16>                U  13.2   5.2   0.0 (u>=2   7.1)  V   0.0   0.0   0.0
B2-M130-R20-K3-(-16,15)-nz6           2 blocks k_bcd_mid / k_bcd_mid                U   9.5   1.7   0.1 (u>=2   6.8)  V   0.1   0.0   0.0  z
B2-M384-R32-K3-(-16,15)-nz4           2 blocks k_bcd_mid / k_bcd_mid                U  16.9   0.5   0.2 (u>=2  12.7)  V   0.0   0.0   0.0
B1024-M130-R8-K3-(-16,15)-nz2      1024 blocks k_bcd_w / k_bcd_w                    U  23.3   1.0   0.0 (u>=2   9.9)  V   2.1  24.0   0.0  vz
B1024-M17-R8-K3-(-128,127)-nz4     1024 blocks k_bcd_w / k_bcd_w                    U  12.9   1.0   0.0 (u>=2   7.4)  V   0.0   0.0   0.0
B1024-M48-R12-K3-(-16,15)-nz2      1024 blocks k_bcd<16> / k_bcd_w16                U  21.7   2.4   0.1 (u>=2   8.5)  V   1.8  21.2   0.0  vz
B1024-M130-R16-K3-(-32,31)-nz10    1024 blocks k_bcd<16> / k_bcd<16>                U   7.5   0.3   0.0 (u>=2   6.2)  V   0.0   0.0   0.0
B64-M400-R20-K3-(-16,15)-nz4        128 blocks k_bcd_mid / k_bcd_w32<10>            U  16.2   2.1   0.1 (u>=2  12.5)  V   0.0   0.0   0.0  z
B128-M130-R17-K3-(-4,4)-nz10        128 blocks k_bcd_mid / k_bcd_w32<9>             U   5.7   0.0   0.1 (u>=2   3.4)  V   0.1   0.0   0.0  c
B128-M17-R20-K3-(-4,4)-nz2          128 blocks k_bcd_mid / k_bcd_w32<10>            U  25.0   2.5   0.0 (u>=2  12.8)  V   3.0  13.5   0.0  vz
B128-M384-R20-K3-(-25,25)-nz6       128 blocks k_bcd_mid / k_bcd_mid                U  11.2   0.2   0.0 (u>=2   8.4)  V   0.0   0.0   0.0
B2304-M384-R7-K3-(-16,15)-nz4      2304 blocks k_bcd_w / k_bcd_w p<-,0>             U  14.8   4.8   0.0 (u>=2  11.4)  V   0.0   0.0   0.0  z
B2304-M48-R8-K3-(-3,5)-nz6         2304 blocks k_bcd_w / k_bcd_w p<-,0>             U   9.6   2.1   0.0 (u>=2   7.3)  V   3.1   1.6   0.0  v
B2304-M130-R12-K3-(-8,7)-nz6       2304 blocks k_bcd<16> / k_bcd_w16 p<f16,0>       U   9.4   0.3   1.4 (u>=2   5.8)  V   0.0   0.0   0.0  c
B2304-M48-R12-K3-(-3,5)-nz4        2304 blocks k_bcd<16> / k_bcd_w16 p<f16,0>       U  15.6   5.9   0.1 (u>=2  11.3)  V   1.7   0.3   0.0  vz
B1152-M400-R22-K3-(-16,15)-nz4     2304 blocks k_bcd_mid / k_bcd_w32<11> p<f16,11>  U  16.8   0.4   0.1 (u>=2  12.8)  V   0.0   0.0   0.0
B2304-M24-R20-K3-(-16,15)-nz2      2304 blocks k_bcd_mid / k_bcd_w32<10> p<f16,10>  U  24.2   2.5   0.1 (u>=2  10.4)  V   2.9  10.0   0.0  vz
B2-M130-R40-K3-(-16,15)-nz4                    any-shape kernels                    U  19.7   0.4   0.4 (u>=2  17.4)  V   0.0   0.0   0.0  c
B2-M400-N16-R6-K3-(-3,5)-nz2                   any-shape kernels                    U  44.7   0.0  16.5 (u>=2  42.7)  V   0.0   0.0   0.0  c
B2-M130-N192-R12-K3-(-16,15)-nz6               any-shape kernels                    U   7.7   2.8   0.0 (u>=2   4.2)  V   0.1   0.0   0.0  z
"""
import numpy as np

F32 = np.float32
EPS = F32(1e-16)
LIMIT = float(1 << 24)
GEN_CHUNK = 8
KERNEL_NAMES = ("k_bcd<8>", "k_bcd<16>", "k_bcd_mid", "k_bcd_w", "k_bcd_w16", "k_bcd_w32", "k_bcd_w32f")  # enum BcdKernel


def _half(x, u, v, lo, hi, st, later, trace=None):
    """One update_u (qmf.py:103-126) of every matrix: x [B,I,D], old u [B,I,R], v [B,D,R], all float64 holding integers."""
    R = u.shape[-1]
    a, b = x @ v, v.transpose(0, 2, 1) @ v
    assert (np.abs(x) @ np.abs(v)).max(initial=0) < LIMIT, "|x| |v| reaches 2^24"
    u = u.copy()
    mx = max(abs(lo), abs(hi))
    err = np.seterr(invalid="ignore")  # (np.mod by a zero denominator below; masked by den > 0)
    for r in range(R):
        bb = b[:, :, r].copy()
        den = bb[:, r].copy()
        bb[:, r] = 0  # the new columns < r and the old columns > r
        num = a[:, :, r] - (u @ bb[:, :, None])[:, :, 0]
        assert (np.abs(u) @ np.abs(bb)[:, :, None]).max(initial=0) < LIMIT, "|u_j| |b_jr| reaches 2^24"
        assert np.abs(num).max(initial=0) < LIMIT and den.max(initial=0) < LIMIT, "num or b_rr reaches 2^24"
        den = np.broadcast_to(den[:, None], num.shape)
        q = (num.astype(F32) + EPS) / (den.astype(F32) + EPS)  # one IEEE fp32 division
        rq = np.rint(q)
        new = np.clip(rq, lo, hi)
        tie = (den > 0) & (np.mod(2 * num, 2 * den) == den) & (np.abs(num) < (mx + 2) * den)
        st["solves"] += num.size
        st["ties"] += int(tie.sum())
        st["zero_den"] += int((den == 0).sum())
        st["clamped"] += int((new != rq).sum())
        if later:
            st["later_solves"] += num.size
            st["later_ties"] += int(tie.sum())
        u[:, :, r] = new
        if trace is not None:
            trace.append((num.copy(), den.copy()))
    np.seterr(**err)
    return u


def new_stats():
    return {h: dict(solves=0, ties=0, zero_den=0, clamped=0, later_solves=0, later_ties=0) for h in "uv"}


def reference_bcd(X, U0, V0, K, lo, hi, chunk=32, threads=8):
    """K iterations of QMF's solver from (U0, V0) on integer arrays X [B,M,N], U0 [B,M,R], V0 [B,N,R] -> int64 (U, V) and, per
    half ("u", "v"), the counts of solves, exact ties with |q| < mx + 2, zero denominators and clamped values.  Asserts, from sums
    of absolute values, that every sum stays below 2^24: a case that breaks this is a bad case, not a finding.  The matrices are
    independent: chunks of them run on a few threads (numpy releases the lock)."""
    from concurrent.futures import ThreadPoolExecutor
    for t in (X, U0, V0):
        assert np.issubdtype(np.asarray(t).dtype, np.integer)
    U, V = np.empty(U0.shape, np.int64), np.empty(V0.shape, np.int64)

    def run(b0):
        s = slice(b0, b0 + chunk)
        st = new_stats()
        x, u, v = X[s].astype(np.float64), U0[s].astype(np.float64), V0[s].astype(np.float64)
        xt = np.ascontiguousarray(x.transpose(0, 2, 1))
        for it in range(K):
            u = _half(x, u, v, lo, hi, st["u"], it > 0)  # U half first,
            v = _half(xt, v, u, lo, hi, st["v"], it > 0)  # then the V half on X.T (qmf.py:128-139)
        U[s], V[s] = u, v
        return st

    starts = range(0, X.shape[0], chunk)
    if len(starts) > 1:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            parts = list(pool.map(run, starts))
    else:
        parts = [run(0)]
    total = new_stats()
    for st in parts:
        for h in "uv":
            for k in total[h]:
                total[h][k] += st[h][k]
    return U, V, total


def explain(X, U0, V0, K, lo, hi, half, i, r):
    """What the reference solved at entry (i, r) of factor `half` ("u" or "v") of ONE matrix in the last iteration: the exact
    num and den there and what kind of entry it is — for the message of a failed comparison."""
    x, u, v = (np.asarray(t, np.float64)[None] for t in (X, U0, V0))
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))
    st = new_stats()
    for it in range(K):
        tu, tv = [], []
        u = _half(x, u, v, lo, hi, st["u"], it > 0, tu)
        v = _half(xt, v, u, lo, hi, st["v"], it > 0, tv)
    num, den = (int(t[0, i]) for t in (tu if half == "u" else tv)[r])
    kind = []
    if den == 0:
        kind.append("zero denominator")
    elif (2 * num) % (2 * den) == den:
        kind.append("exact tie")
    elif abs((2 * num) % (2 * den) - den) * 64 <= den:
        kind.append("near-tie")
    q = (F32(num) + EPS) / (F32(den) + EPS)
    if not lo <= np.rint(q) <= hi:
        kind.append("clamped")
    return f"num = {num}, den = {den}, q = {q!r} ({', '.join(kind) or 'plain'}), expected {int((v if half == 'v' else u)[0, i, r])}"


def generate(seed, B, M, N, R, lo, hi, xmax, nz, zero_x=False, zero_v=False):
    """Seeded integer inputs: X uniform in [0, xmax] (zero_x: half of its columns, picked per matrix, are zero), U0 uniform in
    [lo, hi], V0 columns with nz entries of +-1 (zero_v: column R // 2 is all zero)."""
    out = []
    for b0 in range(0, B, GEN_CHUNK):  # a generator per GEN_CHUNK matrices: a prefix of a large case costs only its own chunks
        n = min(GEN_CHUNK, B - b0)
        rng = np.random.default_rng([seed, b0])
        X = rng.integers(0, xmax + 1, (n, M, N), dtype=np.int32)
        if zero_x:
            X *= (rng.random((n, 1, N)) < 0.5)
        U0 = rng.integers(lo, hi + 1, (n, M, R), dtype=np.int32)
        where = np.argsort(rng.random((n, N, R)), axis=1)[:, :nz]  # nz distinct rows per column
        V0 = np.zeros((n, N, R), np.int32)
        np.put_along_axis(V0, where, rng.integers(0, 2, where.shape, dtype=np.int32) * 2 - 1, axis=1)
        if zero_v:
            V0[:, :, R // 2] = 0
        out.append((X, U0, V0))
    return tuple(np.concatenate(t) for t in zip(*out))


class Case:
    """(B, M, N, R, K, lo, hi) and the generator's arguments; marks: "v" = counts as V-update coverage (>= 1 % ties in the V
    half), "z" = holds zero denominators, "c" = holds clamped values"""

    def __init__(self, B, M, R, K, lo, hi, xmax, nz, marks="", N=64, **gen):
        self.B, self.M, self.N, self.R, self.K, self.lo, self.hi = B, M, N, R, K, lo, hi
        self.gen = dict(xmax=xmax, nz=nz, **gen)
        self.marks = marks
        self.seed = 1000 * R + M + 7 * nz + abs(lo)
        self.id = f"B{B}-M{M}" + (f"-N{N}" if N != 64 else "") + f"-R{R}-K{K}-({lo},{hi})-nz{nz}"

    def inputs(self, B=None):
        """the case's (X, U0, V0); B: only its first B matrices"""
        return generate(self.seed, min(B or self.B, self.B), self.M, self.N, self.R, self.lo, self.hi, **self.gen)

    def blocks(self):
        return self.B * ((self.M + 383) // 384)


# ---- the 64-column table.  Block counts are B * ceil(M / 384) against LRF_BCDW_MIN_BLOCKS = LRF_BCDW16_MIN_BLOCKS = 1024,
# LRF_BCDW32_MIN_BLOCKS = 128 and LRF_PERSIST_MIN_BLOCKS_ONE_FAMILY = 2304 (a call of one rank has one family), at default settings.
CASES = [
    # the workgroup kernels k_bcd<8>, k_bcd<16>, k_bcd_mid: small calls, small M (the ATen-native order at (R - 1) M < 400)
    Case(1, 1, 8, 3, -3, 5, 6, 2, "vzc", zero_v=True),
    Case(2, 17, 12, 3, -4, 4, 2, 2, "v"),
    Case(3, 17, 20, 3, -3, 5, 2, 2, "vc"),
    Case(2, 48, 20, 3, -4, 4, 6, 6, "c"),
    Case(3, 130, 1, 3, -16, 15, 40, 2, "c"),
    Case(3, 130, 5, 4, -16, 15, 12, 4, "z", zero_v=True),
    Case(4, 400, 8, 3, -16, 15, 1, 2, "vz"),
    Case(2, 400, 8, 3, -128, 127, 40, 6, "", zero_x=True),
    Case(2, 384, 12, 3, -16, 15, 12, 10, "z", zero_v=True),
    Case(2, 400, 16, 3, -32, 31, 12, 4, ""),
    Case(2, 130, 20, 3, -16, 15, 12, 6, "z", zero_v=True),
    Case(2, 384, 32, 3, -16, 15, 8, 4, ""),
    # k_bcd_w from 1024 blocks on, any bounds
    Case(1024, 130, 8, 3, -16, 15, 1, 2, "vz"),
    Case(1024, 17, 8, 3, -128, 127, 40, 4, ""),
    # k_bcd_w16 from 1024 blocks on; (-32, 31): 15 * 64 * 32^3 >= 2^24, the run stays on k_bcd<16>
    Case(1024, 48, 12, 3, -16, 15, 1, 2, "vz"),
    Case(1024, 130, 16, 3, -32, 31, 12, 10, ""),
    # k_bcd_w32 from 128 blocks on; (-25, 25): 64 * 25^2 > 32767, the run stays on k_bcd_mid
    Case(64, 400, 20, 3, -16, 15, 12, 4, "z", zero_v=True),
    Case(128, 130, 17, 3, -4, 4, 6, 10, "c"),
    Case(128, 17, 20, 3, -4, 4, 1, 2, "vz"),
    Case(128, 384, 20, 3, -25, 25, 12, 6, ""),
    # one persistent launch k_bcd_p from 2304 blocks on: ranks <= 8, 9..16 (f16), 17..32 (np32)
    Case(2304, 384, 7, 3, -16, 15, 12, 4, "z", zero_v=True),
    Case(2304, 48, 8, 3, -3, 5, 1, 6, "v"),
    Case(2304, 130, 12, 3, -8, 7, 12, 6, "c"),
    Case(2304, 48, 12, 3, -3, 5, 1, 4, "vz"),
    Case(1152, 400, 22, 3, -16, 15, 10, 4, ""),
    Case(2304, 24, 20, 3, -16, 15, 1, 2, "vz"),
]
# ---- the any-shape Gauss-Seidel behind the same entry point: R = 40 at N = 64, N = 16, N = 192 at a rank <= 16
ANY_CASES = [
    Case(2, 130, 40, 3, -16, 15, 8, 4, "c"),
    Case(2, 400, 6, 3, -3, 5, 6, 2, "c", N=16),
    Case(2, 130, 12, 3, -16, 15, 12, 6, "z", N=192, zero_v=True),
]
# the ten smallest cases: tools/gen_exact_bcd.py records the reference's own factors of them in tests/golden/exact_bcd.npz
GOLDEN_CASES = sorted(CASES + ANY_CASES, key=lambda c: c.B * (c.M + c.N) * c.R)[:10]


def share(st, key="ties"):
    return 100.0 * st[key] / max(st["solves"], 1)


def later_share(st):
    return 100.0 * st["later_ties"] / max(st["later_solves"], 1)


def describe(case, head, run, st):
    """one line of the docstring's table; head, run: the case's plan (None for the any-shape cases)"""
    if head is None:
        k, blocks = "any-shape kernels", ""
    else:
        k = f"{KERNEL_NAMES[run['first_k']]} / {KERNEL_NAMES[run['later_k']]}" + (f"<{run['later_arg']}>" if run["later_arg"] else "")
        k += f" p<{'f16' if head['f16'] else '-'},{head['np32']}>" if head["persist"] else ""
        blocks = f"{case.blocks():5d} blocks"
    f = lambda h: f"{share(st[h]):5.1f} {share(st[h], 'zero_den'):5.1f} {share(st[h], 'clamped'):5.1f}"
    return f"{case.id:33s} {blocks:12s} {k:36s} U {f('u')} (u>=2 {later_share(st['u']):5.1f})  V {f('v')}  {case.marks}"


DOC_CUT = 8  # the shares in the docstring are those of a case's first DOC_CUT matrices

if __name__ == "__main__":
    import ctypes
    import os
    import subprocess
    import tempfile
    import test_bcd_plan as P
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libbcd_plan_test.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", so, os.path.join(P.CSRC, "lrf_plan.cpp"),
                               os.path.join(here, "bcd_plan_shim.cpp")])
        lib = ctypes.CDLL(so)
        print(f"{'case':33s} {'':12s} {'first / later kernel':36s}     tie  zero clamp {'':13s}    tie  zero clamp  marks")
        for c in CASES + ANY_CASES:
            st = reference_bcd(*c.inputs(DOC_CUT), c.K, c.lo, c.hi)[2]
            head, runs = P.plan(lib, [(c.M, c.R)] * c.B, c.K, (c.lo, c.hi), P.FIRST_U0) if c in CASES else (None, [None])
            print(describe(c, head, runs[0], st).rstrip())
