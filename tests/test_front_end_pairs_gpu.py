"""GPU suite (-m gpu): both instantiations of k_planes16_gram (lrf_amd/csrc/lrf_planes_gram_kernel.hip) at the smallest sizes
where its unit walk can go wrong — one unit, segments whose last has 2 live patch columns of 32, chunks of 3 and 4 units, an odd
number of chunks — forced on (LRF_FUSED_GRAM_MIN_CHUNKS=1) against the two-kernel form k_planes16 + k_gram64: identical int8
factors, for batches of 1, 2 and 3 images and for a batch that LRF_PERSIST=1 puts on k_bcd_p, whose rank <= 8 body reads luma
from the image bytes, so that the planes kernel runs without its "luma rows out" phase (<false>); with LRF_LUMA_BYTES=0 the same
batch runs <true>.  One batch is compared with the oracle.

The GPU work runs in child processes (tests/_front_end_pairs_worker.py: the hooks are read once per process), each under a
time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import _front_end_pairs_worker as W

pytestmark = pytest.mark.gpu

NCALLS = len(W.GEOMETRIES) * (len(W.SMALL_BATCHES) + 1)
NSMALL = len(W.GEOMETRIES) * len(W.SMALL_BATCHES)


def _run(tmp_path, tag, min_chunks, luma_bytes):
    env = dict(os.environ, LRF_PERSIST="1", LRF_FUSED_GRAM_MIN_CHUNKS=str(min_chunks))
    for k in ("LRF_LUMA_BYTES", "LRF_X_KEEP_MB", "LRF_FAMILY_SPLIT_BLOCKS"):
        env.pop(k, None)
    if luma_bytes is not None:
        env["LRF_LUMA_BYTES"] = luma_bytes
    out = os.path.join(str(tmp_path), tag + ".npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_front_end_pairs_worker.py"), out], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    which = [l for l in r.stderr.splitlines() if l.startswith("launches:")]
    assert len(which) == 1, r.stderr
    return r.stdout.splitlines(), which[0], out


@pytest.mark.parametrize("luma_bytes", [None, "0"], ids=["luma_from_bytes", "luma_from_x"])
def test_fused_form_gives_the_factors_of_the_two_kernel_form(luma_bytes, tmp_path, oracle):
    fused, which_f, out_f = _run(tmp_path, "fused", 1, luma_bytes)
    plain, which_p, _ = _run(tmp_path, "plain", 1 << 40, luma_bytes)
    print(which_f)
    print(which_p)
    src = "x" if luma_bytes == "0" else "bytes"
    n = len(W.GEOMETRIES)
    assert which_f == f"launches: small k_planes16_gram {NSMALL} k_planes16 0 k_bcd_p 0; persist k_planes16_gram {n} k_planes16 0 k_bcd_p {n} luma from {src}", which_f
    assert which_p == f"launches: small k_planes16_gram 0 k_planes16 {NSMALL} k_bcd_p 0; persist k_planes16_gram 0 k_planes16 {n} k_bcd_p {n} luma from {src}", which_p
    assert len(fused) == NCALLS and fused == plain, "\n".join(a + "   |   " + b for a, b in zip(fused, plain))
    # the fused form's factors of one batch against the oracle
    from lrf_amd.codec import split_factors
    (H, Wd), B = W.ORACLE_CALL
    ranks = dict(W.GEOMETRIES)[(H, Wd)]
    imgs = W.build_images(B, H, Wd, W.seed_of(H, Wd, B)).numpy()
    got = np.load(out_f)
    for b in range(B):
        f = split_factors(got["U"][b], got["V"][b], (H, Wd), ranks)
        X = oracle.rgb_to_planes(imgs[b])
        for c in range(3):
            u, v = oracle.qmf_decompose(X[c], ranks[c], 10, (-16, 15))
            assert np.array_equal(f[2 * c], u.astype(np.int8)) and np.array_equal(f[2 * c + 1], v.astype(np.int8)), (b, c)
