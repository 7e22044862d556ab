"""(build container) tests/golden/svd_product.json: SHA-256 of torch's CPU fp32 product `u @ v.mT`, one thread as the reference
is pinned (tools/pin_oracle.py), on the float factors of tests/svd_cases.py — every residue case and decoder rank whose shape
svd_cases.product_is_pinned names, every wide case, every case without patches (batched), and a single 8x8 patch at rank 2.
BLAS picks its routine by the CPU it runs on, so the order is recorded where the reference is pinned and not asked of the
torch of whatever machine runs the suite.  tests/test_svd_cases.py holds the oracle's product to these."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svd_cases as sc  # noqa: E402


def main():
    torch.set_num_threads(1)
    out = {}
    for key, (u, v) in sc.product_cases().items():
        x = (torch.from_numpy(u) @ torch.from_numpy(v).mT).numpy()
        out[key] = hashlib.sha256(np.ascontiguousarray(x, dtype=np.float32).tobytes()).hexdigest()
    with open(os.path.join(ROOT, "tests", "golden", "svd_product.json"), "w") as f:
        json.dump({"torch": torch.__version__.split("+")[0], "threads": 1, "sha256": out}, f, indent=0, sort_keys=True)
    print(len(out), "products recorded")


if __name__ == "__main__":
    main()
