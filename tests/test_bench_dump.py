"""CPU suite: bench.py --dump-outputs stays inside its byte budget by one fixed, seeded sample of images, the same rows of every
array.  The helper runs in a child process: importing bench.py sets the HIP runtime's queue count in the importer's environment."""
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT

CHILD = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
import bench


class Ctx:  # bench.dump_outputs copies through the context, as lrf_amd's wrappers do
    def to_host(self, *tensors):
        return tuple(t.cpu() for t in tensors)


g = torch.Generator().manual_seed(5)
U = torch.randint(-16, 16, (64, 5000), dtype=torch.int8, generator=g)
V = torch.randint(-16, 16, (64, 100), dtype=torch.int8, generator=g)
bench.dump_outputs(Ctx(), sys.argv[2], {"U": U, "V": V}, int(sys.argv[3]))
"""


def _dump(directory, budget):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(directory), str(budget)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return {f[:-4]: np.load(os.path.join(directory, f)) for f in sorted(os.listdir(directory))}


def test_dump_outputs_samples_images_to_fit_its_budget(tmp_path):
    g = torch.Generator().manual_seed(5)
    U = torch.randint(-16, 16, (64, 5000), dtype=torch.int8, generator=g).numpy()
    V = torch.randint(-16, 16, (64, 100), dtype=torch.int8, generator=g).numpy()
    whole = _dump(tmp_path / "whole", 64 * 5100 * 4)
    assert sorted(whole) == ["U", "V"] and whole["U"].dtype == whole["V"].dtype == np.float32
    assert np.array_equal(whole["U"], U) and np.array_equal(whole["V"], V)
    budget = 20 * 5100 * 4
    a, b = _dump(tmp_path / "a", budget), _dump(tmp_path / "b", budget)
    assert sorted(a) == ["U", "V", "sample_images"]
    rows = a["sample_images"].astype(np.int64)
    assert a["sample_images"].dtype == np.float64 and len(rows) == 19 and np.all(np.diff(rows) > 0) and rows[-1] < 64
    assert np.array_equal(a["U"], U[rows]) and np.array_equal(a["V"], V[rows])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget
    assert all(np.array_equal(a[n], b[n]) for n in a), "the sample is fixed: the same rows in every run"
