"""Batched PSNR / SSIM on the device (lrf_image_metrics_u8, lrf_amd.image_metrics_batch): what can be checked without a GPU.
  1. the arithmetic contract of the kernel — exact integer window sums, then the float64 formula (tests/metrics_cases.py) — is
     the definition lrf_amd.metrics.ssim / psnr already state (bars: SSIM 1e-9, PSNR 1e-4 dB; measured here 6.9e-13 / 3.8e-6 dB);
  2. the entry point and its kernel id exist in the header, the built library and the binding;
  3. image_metrics_batch refuses bad arguments before it asks for a GPU;
  4. the shipped metrics kernels hold no flat_ memory instruction and use no scratch."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from metrics_cases import PSNR_BAR, SSIM_BAR, cases, psnr_contract, ssim_contract
from test_bcdp_codegen import LLVM, _code_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_contract_is_the_definition_of_metrics_ssim_and_psnr():
    from lrf_amd import metrics
    worst_s = worst_p = 0.0
    n = 0
    for name, a, b in cases():
        ref_s = metrics.ssim(torch.from_numpy(a), torch.from_numpy(b)).item()
        ref_p = metrics.psnr(torch.from_numpy(a), torch.from_numpy(b)).item()
        got_s, got_p = ssim_contract(a, b), psnr_contract(a, b)
        n += 1
        assert not math.isnan(ref_s), name
        worst_s = max(worst_s, abs(ref_s - got_s))
        if math.isinf(ref_p):
            assert got_p == ref_p, name
        else:
            worst_p = max(worst_p, abs(ref_p - got_p))
        assert abs(ref_s - got_s) <= SSIM_BAR, (name, ref_s, got_s)
        assert math.isinf(ref_p) or abs(ref_p - got_p) <= PSNR_BAR, (name, ref_p, got_p)
    print(f"{n} cases: worst |SSIM difference| {worst_s:.3g}, worst |PSNR difference| {worst_p:.3g} dB")
    assert n == 40
    # a constant first image: data_range 0, c1 = c2 = 0, 0/0 in every window on both sides
    a = np.full((3, 9, 12), 77, np.uint8)
    with np.errstate(invalid="ignore"):
        assert math.isnan(metrics.ssim(torch.from_numpy(a), torch.from_numpy(a)).item()) and math.isnan(ssim_contract(a, a))


def test_entry_point_and_kernel_id_are_in_header_library_and_binding():
    import ctypes
    from lrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    assert re.search(r"\bint\s+lrf_image_metrics_u8\s*\(", header)
    assert "lrf_image_metrics_u8" in _lib.EXPORTS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "lrf_image_metrics_u8")
    assert _lib.load().lrf_image_metrics_u8.argtypes is not None
    m = re.search(r"#define\s+LRF_K_METRICS\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.LRF_K_METRICS == 8
    assert int(re.search(r"#define\s+LRF_K_COUNT\s+(\d+)", header).group(1)) == 9
    assert _lib.LRF_K_METRICS in _lib.KERNEL_NAMES
    ctx_src = open(os.path.join(ROOT, "lrf_amd", "csrc", "lrf_metrics.hip")).read()
    assert "Prof p(c, LRF_K_METRICS)" in ctx_src  # the timers of lrf_ctx_kernel_time are arrays of LRF_K_COUNT


def test_bad_arguments_are_refused_before_a_gpu_is_asked_for(monkeypatch):
    import lrf_amd
    from lrf_amd import _lib

    def no_context(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_lib, "context", no_context)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    with pytest.raises(TypeError):
        lrf_amd.image_metrics_batch(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16))
    with pytest.raises(TypeError):
        lrf_amd.image_metrics_batch(u8(2, 3, 16, 16), torch.zeros(2, 3, 16, 16, dtype=torch.int16))
    with pytest.raises(ValueError):
        lrf_amd.image_metrics_batch(u8(2, 3, 16, 16), u8(2, 3, 16, 17))
    with pytest.raises(ValueError):
        lrf_amd.image_metrics_batch(u8(2, 3, 16, 16), u8(1, 3, 16, 16))
    with pytest.raises(ValueError):
        lrf_amd.image_metrics_batch(u8(16, 16), u8(16, 16))
    with pytest.raises(ValueError):
        lrf_amd.image_metrics_batch(u8(1, 3, 6, 16), u8(1, 3, 6, 16))
    with pytest.raises(ValueError):
        lrf_amd.ssim_batch(u8(3, 16, 6), u8(3, 16, 6))
    with pytest.raises(AssertionError, match="a context was asked for"):  # H < 7 is fine without the SSIM
        lrf_amd.psnr_batch(u8(1, 3, 6, 16), u8(1, 3, 6, 16))
    with pytest.raises(ValueError):
        lrf_amd.rd_sweep_batched(u8(1, 3, 16, 16), (5,), metrics="gpu")


@pytest.fixture(scope="module")
def metrics_kernels(tmp_path_factory):
    """name -> (instructions, kernel descriptor metadata text) of the k_metrics_* / k_ssim_* kernels of the shipped library"""
    tmp = tmp_path_factory.mktemp("metrics_codegen")
    found = {}
    for i, co in enumerate(_code_objects(tmp)):
        path = tmp / f"co{i}.o"
        path.write_bytes(co)
        txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", str(path)], text=True)
        if "k_ssim_tiles" not in txt:
            continue
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(path)], text=True)
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1) if re.match(r"_Z\d+k_(ssim|metrics)_", m.group(1)) else None
                if cur:
                    found[cur] = ([], notes)
            elif cur and line.startswith("\t"):
                found[cur][0].append(line.strip().split("//")[0].strip())
    return found


def test_metrics_kernels_use_no_flat_access_and_no_scratch(metrics_kernels):
    names = sorted(metrics_kernels)
    assert sum("k_ssim_tiles" in n for n in names) == 3 and sum("k_metrics_pre" in n for n in names) == 6 and \
        sum("k_ssim_final" in n for n in names) == 1, names
    for name, (ins, notes) in metrics_kernels.items():
        assert len(ins) > 20, name
        bad = [i for i in ins if i.startswith("flat_") or i.startswith("scratch_")]
        assert not bad, (name, bad[:5])
        m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", notes)
        assert m, name
        assert int(m.group(1)) == 0, (name, m.group(1))
    tiles = [ins for n, (ins, _) in metrics_kernels.items() if "k_ssim_tiles" in n]
    for ins in tiles:  # ONE float64 division per window: six windows per thread
        assert sum(i.startswith("v_div_fixup_f64") for i in ins) == 6
