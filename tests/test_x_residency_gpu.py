"""GPU suite (-m gpu): the cache policy of the X loads in the rank <= 8 body of k_bcd_p (lrf_bcdp_kernel.hip: bcdp_w_block; which
blocks: plan_x_residency, lrf_plan.h).  Kept chroma planes load plain, everything else — luma from the image bytes or from
fp32 X, the chroma planes past the budget — loads non-temporal.  A cache-policy bit cannot change a result: U and V must be
byte-identical with LRF_X_KEEP_MB = 0 (no policy), a budget that splits the chroma planes of one image, a budget that keeps
all of them, a budget the whole call fits (the policy leaves such a call alone), and on the per-iteration kernels
(LRF_PERSIST=0).  Every call must say through lrf_ctx_last_x_residency what it kept — the numbers are counted by hand from
the plane sizes, as in tests/test_x_residency_plan.py — so a call that silently ran without the policy fails.

The GPU work runs in child processes (the settings are read once per process), one per (case, setting), started once per module
run, each under its own timeout.  After a child that timed out or did not exit cleanly nothing further is started on the GPU
by this module.  The parent never initialises HIP."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _x_residency_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120  # seconds per child (two small calls and the start of the process: a few seconds)
_stopped = []  # why nothing more is started on the GPU
_children = {}

# (LRF_PERSIST, LRF_X_KEEP_MB): no policy; 18 x 10^6 bytes; 40 x 10^6: room for every chroma plane, not for the call; room for
# the call; the per-iteration kernels
SETTINGS = [("1", "0"), ("1", "18"), ("1", "40"), ("1", "1000"), ("0", None)]
# what lrf_ctx_last_x_residency must report, (planes, bytes), per case in the order of SETTINGS.  A chroma plane of M rows is
# 256 M bytes of X.
#   small: M = 143, 36608 bytes; 18e6 / 36608 = 491.7: the 256 Cb planes and the Cr planes of images 0..234 (image 235 keeps
#          its Cb plane and streams its Cr plane); all: 512 planes, 18.7 MB; a pass reads 28.1 MB of image bytes + 18.7 = 46.9 MB
#   fp32:  M = 1536, 393216 bytes; 18e6 / 393216 = 45.8: the 44 Cb planes and the Cr plane of image 0 (image 1 keeps its Cb
#          plane and streams its Cr plane); all: 88 planes, 34.6 MB; a pass reads 69.2 MB of fp32 luma + 34.6 = 103.8 MB
KEPT = {"small": [(0, 0), (491, 491 * 36608), (512, 512 * 36608), (0, 0), (0, 0)],
        "fp32": [(0, 0), (45, 45 * 393216), (88, 88 * 393216), (0, 0), (0, 0)]}


def _child(case, persist, keep, tmp_path_factory):
    """the arrays one child saved; run once per module run"""
    key = (case, persist, keep)
    if key in _children:
        return _children[key]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = dict(os.environ)
    env["LRF_PERSIST"] = persist
    env["LRF_LUMA_BYTES"] = W.CASES[case][5]
    env.pop("LRF_X_KEEP_MB", None)
    if keep is not None:
        env["LRF_X_KEEP_MB"] = keep
    out = str(tmp_path_factory.mktemp("x_residency") / f"{case}_{persist}_{keep}.npz")
    what = f"the ({case}, LRF_PERSIST={persist}, LRF_X_KEEP_MB={keep}) child"
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "_x_residency_worker.py"), case, out], env=env, capture_output=True, text=True,
                           timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"{what} did not finish in {TIMEOUT} s")
        pytest.fail(f"{_stopped[0]}: {str(e.stdout)[-2000:]}")
    if r.returncode != 0:
        _stopped.append(f"{what} exited with {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"DONE {case}" in r.stdout, r.stdout[-2000:]
    with np.load(out) as z:
        _children[key] = {k: z[k] for k in z.files}
    return _children[key]


@pytest.mark.parametrize("case", list(W.CASES))
def test_factors_do_not_depend_on_the_cache_policy(case, tmp_path_factory):
    B, H, Wd, ranks, K, luma_bytes = W.CASES[case]
    runs = [_child(case, persist, keep, tmp_path_factory) for persist, keep in SETTINGS]
    ref = runs[-1]  # LRF_PERSIST=0
    for (persist, keep), got, kept in zip(SETTINGS, runs, KEPT[case]):
        what = f"{case} LRF_PERSIST={persist} LRF_X_KEEP_MB={keep}"
        assert int(got["images_sum"]) == int(ref["images_sum"]), what
        # the path: one persistent launch with the luma source the case is about, or none
        assert int(got["launches"]) == (1 if persist == "1" else 0), (what, int(got["launches"]))
        assert str(got["source"]) == ("bytes" if persist == "1" and luma_bytes == "1" else "x"), (what, str(got["source"]))
        assert tuple(int(v) for v in got["kept"]) == kept, (what, got["kept"], kept)
        assert got["U"].shape == ref["U"].shape and got["V"].shape == ref["V"].shape and got["U"].shape[0] == B, what
        for name in ("U", "V"):
            ne = np.flatnonzero(got[name].reshape(-1) != ref[name].reshape(-1))
            assert ne.size == 0, f"{what}: {ne.size} of {got[name].size} entries of {name} differ from LRF_PERSIST=0, first at {int(ne[0])}"
            assert np.array_equal(got[name + "2"], got[name]), f"{what}: the second call's {name} differs from the first's"
    assert np.any(ref["U"] != 0) and np.any(ref["V"] != 0), case
