"""GPU suite (-m gpu): k_bcd_p's rank <= 8 block body hands its partials over as dense slots and its int8 U rows as whole 16-B
aligned spans.  The factors must stay bit-equal to the launch-per-iteration path (LRF_PERSIST=0), at the benchmark's batch and at
a batch whose U spans start unaligned, at ranks below 4.  Each setting runs in a child process of its own (the switch is read
once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run(geom, persist, tmp_path):
    env = dict(os.environ)
    env.pop("LRF_PERSIST", None)
    if persist is not None:
        env["LRF_PERSIST"] = persist
    out = str(tmp_path / f"{geom}_{persist}.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_bcdp_dense_worker.py"), geom, out], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("geom, persist", [("bench", None), ("odd", "1")])
def test_bcdp_dense_handoffs_bit_equal(geom, persist, tmp_path):
    got = _run(geom, persist, tmp_path)
    ref = _run(geom, "0", tmp_path)
    for i in range(2):
        assert int(got[f"launches{i}"]) == 1, (geom, i, int(got[f"launches{i}"]))
        assert int(ref[f"launches{i}"]) == 0, (geom, i, int(ref[f"launches{i}"]))
        assert np.array_equal(got[f"U{i}"], ref[f"U{i}"]), (geom, i, "U")
        assert np.array_equal(got[f"V{i}"], ref[f"V{i}"]), (geom, i, "V")
