"""Generates tests/golden/exact_general.npz by running the REFERENCE's own solver (QMF(...).solver = CoordinateDescent behind
QMF._project, lrf/factorization/qmf.py:149-164, 191-195) on GOLDEN_CASES of tests/exact_general.py: the smallest exact-integer
cases of the general solver, the two whose |w1| is below CoordinateDescent's eps, and the update_w cases (both degenerate lines
among them), each from its generated (U0, V0) and its initial pair w.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_exact_general.py
The fixture holds data only: per case the case's arguments (JSON), the reference's fp32 U and V and, while bit 2 of `factor` is
clear, its W (the initial pair, unchanged); the test regenerates the inputs (tests/test_exact_general.py) and never imports the
reference.  One torch thread, as tools/gen_golden.py; the archive is written with fixed time stamps, and everything in it is
the same on every run, so a second run reproduces it byte for byte.
NOT recorded: the W of the update_w cases.  The reference's fp32 torch.linalg.lstsq (qmf.py:146) returns another pair from run to
run, also at one thread (1 to 242 fp32 ulps from the exact line on w-uv; for the constant z = 3 ill-conditioned pairs such as
(-6.4e6, 2.1e6) and (4.7e6, -1.6e6)).  Each run judges the pair it drew by a criterion that holds for every draw
(exact_general.line_error: |A dw| against the first-order error of a backward-stable fp32 solver, which for a constant z is a
statement on the reconstruction w0 + w1 c alone), requires w1 = 0 for z = 0, prints the figures and fails if one is missed."""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import ref_loader  # noqa: E402
import exact_general  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "exact_general.npz")


def save(path, arrays):
    """np.savez_compressed with the time stamp of every member fixed"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    torch.set_num_threads(1)
    QMF = ref_loader.load().fqmf.QMF
    arrays = {}
    for i, c in enumerate(exact_general.GOLDEN_CASES):
        X, U0, V0 = c.inputs()
        x, u, v = (torch.from_numpy(t).float() for t in (X, U0, V0))
        w = torch.tensor(c.opts.get("w", (0.0, 1.0)), dtype=torch.float32).reshape(1, 2, 1).expand(c.B, 2, 1)
        kw = {k: c.opts[k] for k in ("l2", "l1_ratio", "eps") if k in c.opts}
        qmf = QMF(rank=c.R, num_iters=c.K, bounds=tuple(c.opts.get("bounds", (None, None))), factor=tuple(c.opts["factor"]), **kw)
        for _ in range(c.K):
            u, v, w = qmf.solver(x, [u, v, w])
        arrays[f"args{i}"] = json.dumps(c.args())
        arrays[f"u{i}"] = u.numpy().astype(np.float32)
        arrays[f"v{i}"] = v.numpy().astype(np.float32)
        wr = w.reshape(c.B, 2).numpy().astype(np.float32)
        if 2 not in c.opts["factor"]:
            arrays[f"w{i}"] = wr
            print(c.id, flush=True)
            continue
        for b in range(c.B):  # this draw of the reference's lstsq against the exact line; not recorded
            zz = u[b].double().numpy() @ v[b].double().numpy().T
            err, bound = exact_general.line_error(X[b], zz, wr[b])
            print(f"{c.id} matrix {b}: reference w = ({wr[b][0]!r}, {wr[b][1]!r}), |A dw| = {err:.3g} <= {bound:.3g}", flush=True)
            assert err <= bound, (c.id, b, wr[b], err, bound)
            assert zz.any() or wr[b][1] == 0, (c.id, b, wr[b])
    arrays = dict(n=np.int64(len(exact_general.GOLDEN_CASES)), **arrays)
    save(OUT, arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
