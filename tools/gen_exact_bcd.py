"""Generates tests/golden/exact_bcd.npz by running the REFERENCE's own solver (QMF(...).solver, lrf/factorization/qmf.py:149-164,
factor=(0, 1) as qmf_encode builds it) on the ten smallest exact-integer cases of tests/exact_bcd.py, from their generated
(U0, V0) and the affine pair w = (0, 1).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_exact_bcd.py
The fixture holds data only: per case the generator's arguments (JSON) and the reference's int8 factors; the test regenerates
the inputs (tests/test_exact_bcd.py) and never imports the reference.  One torch thread, as tools/gen_golden.py."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import ref_loader  # noqa: E402
import exact_bcd  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "exact_bcd.npz")


def main():
    torch.set_num_threads(1)
    QMF = ref_loader.load().fqmf.QMF
    arrays = {}
    for i, c in enumerate(exact_bcd.GOLDEN_CASES):
        X, U0, V0 = c.inputs()
        x, u, v = (torch.from_numpy(t).float() for t in (X, U0, V0))
        w = torch.tensor([[0.0], [1.0]]).expand(c.B, 2, 1)
        qmf = QMF(rank=c.R, num_iters=c.K, bounds=(c.lo, c.hi), factor=(0, 1))
        for _ in range(c.K):
            u, v, w = qmf.solver(x, [u, v, w])
        for t in (u, v):
            assert torch.equal(t, t.round()) and t.min() >= c.lo and t.max() <= c.hi
        arrays[f"args{i}"] = json.dumps(dict(id=c.id, seed=c.seed, B=c.B, M=c.M, N=c.N, R=c.R, K=c.K, lo=c.lo, hi=c.hi, gen=c.gen))
        arrays[f"u{i}"] = u.numpy().astype(np.int8)
        arrays[f"v{i}"] = v.numpy().astype(np.int8)
        print(c.id, flush=True)
    np.savez_compressed(OUT, n=np.int64(len(exact_bcd.GOLDEN_CASES)), **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
