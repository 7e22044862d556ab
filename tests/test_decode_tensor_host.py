"""CPU suite: the tensor format of the model-ready decode entries.  _lib.check_tensor_format (no GPU is touched), the definition
restated in tests/tensor_format.py against float64 and against torchvision's own chain, and the gate of the GPU tests: the bytes
their inputs decode to cover the byte values on which a fused multiply-add would differ, so a contracted kernel cannot pass."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tensor_format as tf
from tensor_format import IMAGENET_MEAN, IMAGENET_STD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fmt(*a, **k):
    from lrf_amd import _lib
    return _lib.check_tensor_format(*a, **k)


def test_abi_is_declared():
    from lrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    for name in ("lrf_qmf_decode_crops_tensor", "lrf_qmf_decode_scaled_crops_tensor", "lrf_qmf_decode_resized_crops_tensor"):
        assert name in _lib.EXPORTS and name + "(" in header and hasattr(_lib.load(), name)
    assert "} lrf_tensor_format;" in header and ctypes.sizeof(_lib.TensorFormat) == 32
    for k, v in dict(LRF_T_F32=_lib.T_F32, LRF_T_F16=_lib.T_F16, LRF_T_BF16=_lib.T_BF16, LRF_T_NCHW=_lib.T_NCHW, LRF_T_NHWC=_lib.T_NHWC).items():
        assert f"#define {k} {v}\n" in header


@pytest.mark.parametrize("bad,exc", [
    (dict(dtype="float16"), TypeError), (dict(dtype=np.float32), TypeError), (dict(dtype=None), TypeError),
    (dict(dtype=torch.uint8), ValueError), (dict(dtype=torch.float64), ValueError), (dict(dtype=torch.int8), ValueError),
    (dict(mean="0.5"), TypeError), (dict(mean=[0.5, "a", 0.5]), TypeError), (dict(std=True), TypeError), (dict(mean=[0.1, True, 0.2]), TypeError),
    (dict(std={0.2, 0.3, 0.4}), TypeError), (dict(mean=torch.float32), TypeError),
    (dict(mean=[0.5, 0.5]), ValueError), (dict(std=[0.2] * 4), ValueError), (dict(mean=[]), ValueError),
    (dict(std=0), ValueError), (dict(std=0.0), ValueError), (dict(std=[0.2, 0.0, 0.2]), ValueError), (dict(std=[0.2, -0.0, 0.2]), ValueError),
    (dict(mean=float("nan")), ValueError), (dict(mean=[0.1, float("inf"), 0.1]), ValueError), (dict(std=float("inf")), ValueError),
    (dict(std=[0.2, float("nan"), 0.2]), ValueError), (dict(std=1e-45), ValueError), (dict(mean=1e30, std=1e-30), ValueError),
    (dict(channels_last=1), TypeError), (dict(channels_last="yes"), TypeError), (dict(channels_last=None), TypeError),
])
def test_check_tensor_format_refuses(bad, exc):
    kw = dict(dtype=torch.float16, mean=None, std=None, channels_last=False)
    kw.update(bad)
    with pytest.raises(exc):
        _fmt(**kw)


def test_uint8_takes_no_format_arguments():
    from lrf_amd import _lib
    assert _lib._tensor_request("entry", torch.uint8, None, None, False, None) is None
    for kw in (dict(mean=0.5), dict(std=0.2), dict(channels_last=True), dict(out=torch.empty(1))):
        args = dict(mean=None, std=None, channels_last=False, out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            _lib._tensor_request("entry", torch.uint8, **args)


@pytest.mark.parametrize("mean,std", [(None, None), (0.5, 0.25), (None, 0.5), (0.5, None), (IMAGENET_MEAN, IMAGENET_STD),
                                      (np.array(IMAGENET_MEAN), torch.tensor(IMAGENET_STD).tolist()), (1, 1), ([0, 0, 0], [1, 2, 4])])
def test_constants_against_python_doubles(mean, std):
    from lrf_amd import _lib
    for dtype, code in ((torch.float32, 0), (torch.float16, 1), (torch.bfloat16, 2)):
        for cl in (False, True):
            f = _fmt(dtype, mean, std, cl)
            assert isinstance(f, _lib.TensorFormat) and (f.dtype, f.layout) == (code, int(cl))
            three = lambda v, d: [d] * 3 if v is None else ([float(v)] * 3 if np.isscalar(v) else [float(x) for x in v])
            m, s = three(mean, 0.0), three(std, 1.0)
            for k in range(3):
                assert np.float32(f.scale[k]).tobytes() == np.float32(1.0 / (255.0 * s[k])).tobytes()
                assert np.float32(f.bias[k]) == np.float32(-m[k] / s[k])
            sc, bi = tf.constants(mean, std)
            assert np.array_equal(sc, np.array(list(f.scale), np.float32)) and np.array_equal(bi, np.array(list(f.bias), np.float32))
    f = _fmt(torch.float32)
    assert list(f.scale) == [float(np.float32(1.0 / 255.0))] * 3 and list(f.bias) == [0.0] * 3


def test_the_definition_exhaustively():
    """256 bytes x 3 channels x 3 dtypes.  fp32: against float64 (b / 255 - mean) / std the largest error is recorded and is no
    larger than the one torchvision's own fp32 chain ((b.float() / 255) - mean) / std makes plus one fp32 ulp of the largest value
    (measured: 3.4e-7 against 3.7e-7).  float16 and bfloat16 with the ImageNet constants: all 768 values equal that chain cast
    to the dtype (measured: zero differences)."""
    scale, bias = tf.constants(IMAGENET_MEAN, IMAGENET_STD)
    b = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1).contiguous()  # [3, h = 256, w = 1]
    mean, std = torch.tensor(IMAGENET_MEAN).view(3, 1, 1), torch.tensor(IMAGENET_STD).view(3, 1, 1)
    exact = (b.double() / 255.0 - torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(3, 1, 1)) / torch.tensor(IMAGENET_STD, dtype=torch.float64).view(3, 1, 1)
    tv = ((b.float() / 255) - mean) / std
    ours = tf.apply_format(b, scale, bias, torch.float32)
    err_ours, err_tv = float((ours.double() - exact).abs().max()), float((tv.double() - exact).abs().max())
    ulp = float(np.spacing(np.float32(exact.abs().max())))
    print(f"\nfp32 error against float64: ours {err_ours:.3g}, torchvision's chain {err_tv:.3g}, ulp of the largest value {ulp:.3g}")
    assert err_ours <= err_tv + ulp
    for dtype in (torch.float16, torch.bfloat16):
        n = int((tf.bits(tf.apply_format(b, scale, bias, dtype)) != tf.bits(tv.to(dtype))).sum())
        print(f"{dtype}: {n} of 768 values differ from torchvision's chain cast to the dtype")
        assert n == 0
    # the restatement is the chain of separate roundings: numpy's float32 arithmetic, element by element
    want = (np.arange(256, dtype=np.float32)[None, :] * scale[:, None] + bias[:, None]).astype(np.float32)
    assert np.array_equal(ours.reshape(3, 256).numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(tf.unfused(scale, bias).view(np.int32), want.view(np.int32))
    # float16 overflow is +-inf, as torch's conversion gives
    big = tf.apply_format(b, np.float32([300.0, -300.0, 1.0]), np.float32([0.0, 0.0, 0.0]), torch.float16)
    assert bool(torch.isinf(big[0, 255, 0])) and float(big[0, 255, 0]) > 0 and bool(torch.isinf(big[1, 255, 0])) and float(big[1, 255, 0]) < 0


def test_a_contraction_is_visible():
    """for the ImageNet constants the fused and the unfused form differ on 133, 132 and 124 of the 256 byte values of the three
    channels (exact arithmetic in float64, one rounding, against the two roundings of the definition)"""
    d = tf.fma_differs(*tf.constants(IMAGENET_MEAN, IMAGENET_STD))
    print("\nbyte values on which an fma differs, per channel:", d.sum(axis=1).tolist())
    assert d.sum(axis=1).tolist() == [133, 132, 124]
    assert not tf.fma_differs(*tf.constants()).any()  # without a bias there is nothing to contract


@pytest.mark.parametrize("H,W,ranks", tf.GATE_CASES, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gate_the_gpu_inputs_expose_a_contraction(oracle, H, W, ranks):
    """per channel at least GATE_MIN of the byte values on which the two forms differ occur in the oracle's decode of the case"""
    d = tf.fma_differs(*tf.constants(IMAGENET_MEAN, IMAGENET_STD))
    u, v = tf.case_factors(H, W, ranks)
    img = tf.oracle_image(oracle, u, v, H, W, ranks)
    met = [int(d[k][np.unique(img[k])].sum()) for k in range(3)]
    print(f"\n{H}x{W} {ranks}: differing byte values met per channel {met} of {d.sum(axis=1).tolist()}")
    assert min(met) >= tf.GATE_MIN, met
