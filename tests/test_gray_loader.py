"""The gray loader (gray streams through qmf_decode_ragged / qmf_load_factors / qmf_decode_crops / qmf_decode_scaled /
qmf_decode_resized_crops), CPU part: the numpy definitions of tests/gray_loader.py against the reference's gray fixtures, the
consequences the resized crops promise, the gate on the GPU tests' inputs, and the Python argument refusals, which all come
before a GPU is asked for."""
import os

import numpy as np
import pytest
import torch

import gray_loader as gl
from conftest import GOLDEN
from scaled_decode import block_sum, int_plane
from tensor_format import fma_differs
from test_channels import GRAY8_CASES, ChanCase


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def no_gpu(monkeypatch_module):
    """every refusal below must come before a context is asked for: asking for one fails the test"""
    from lrf_amd import _lib

    def refuse(device=None):
        raise AssertionError("a GPU context was asked for")
    monkeypatch_module.setattr(_lib, "context", refuse)


def _fixture_factors(name):
    c = ChanCase(name)
    u, v = (np.asarray(f, dtype=np.int8) for f in c.ref_factors())
    _, H, W = c.image.shape
    return c, u, v, int(H), int(W)


@pytest.mark.parametrize("name", GRAY8_CASES)
def test_level_1_is_the_fixture_s_decode(name):
    c, u, v, H, W = _fixture_factors(name)
    assert gl.patches(H, W) == u.shape[0] and v.shape[0] == 64
    assert np.array_equal(gl.level(u, v, H, W, 1), c.decoded.reshape(H, W))


@pytest.mark.parametrize("name", GRAY8_CASES)
def test_pooled_levels_lie_within_one_level_of_the_block_average_where_nothing_clamps(name):
    c, u, v, H, W = _fixture_factors(name)
    P = int_plane(u, v, H, W)
    clamps = ((P < 0) | (P > 255)).astype(np.int64)
    for f in (2, 4, 8):
        L = gl.level(u, v, H, W, f)
        assert L.shape == gl.scaled_dims(H, W, f)
        n = block_sum(np.ones((H, W), np.int64), f)
        avg = block_sum(c.decoded.reshape(H, W).astype(np.int64), f) / n
        clean = block_sum(clamps, f) == 0
        assert clean.any()
        assert np.abs(L.astype(np.float64) - avg)[clean].max() <= 1.0
        # and the definition itself: the floor of the exact mean wherever the sum needs no clamp
        s = block_sum(P, f)
        inside = (s >= 0) & (s <= 255 * n)
        assert np.array_equal(L[inside], (s // n)[inside])


def test_partial_blocks_hold_the_pixels_that_exist():
    u, v = gl.case_factors(37, 53, 7, "mid")
    P = int_plane(u, v, 37, 53)
    L = gl.level(u, v, 37, 53, 8)
    assert L.shape == (5, 7)
    s = int(P[32:37, 48:53].sum())
    assert L[4, 6] == min(max(s, 0), 255 * 25) // 25


@pytest.mark.parametrize("size", [(5, 7), (17, 33)])
def test_the_three_consequences_of_the_resized_definition(size):
    H, W, R = 173, 264, 7
    u, v = gl.case_factors(H, W, R, "mid")
    oh, ow = size
    plain = (H - oh, (W - ow) // 3, oh, ow)
    assert np.array_equal(gl.resized(u, v, H, W, plain, size), gl.level(u, v, H, W, 1)[plain[0]:plain[0] + oh, plain[1]:plain[1] + ow])
    for f in (2, 4, 8):
        y0, x0 = (H - f * oh) // f * f, (W - f * ow) // f * f
        box = (y0, x0, f * oh, f * ow)
        assert np.array_equal(gl.resized(u, v, H, W, box, size), gl.level(u, v, H, W, f)[y0 // f:y0 // f + oh, x0 // f:x0 // f + ow])
    box = (3, 5, 101, 77)
    assert np.array_equal(gl.resized(u, v, H, W, box, size, flip=True), gl.resized(u, v, H, W, box, size)[:, ::-1])


def test_the_inputs_of_the_gpu_tests_reach_both_clamps_and_a_hundred_byte_values():
    for f in gl.LEVELS:
        seen = np.zeros(256, bool)
        for H, W, R, tone in gl.ALL_CASES:
            u, v = gl.case_factors(H, W, R, tone)
            seen[np.unique(gl.level(u, v, H, W, f))] = True
        assert seen[0] and seen[255] and int(seen.sum()) >= 100, (f, int(seen.sum()))
    assert sorted(gl.patches(H, W) for H, W in gl.SIZES) == [1, 6, 35, 96, 385, 726]


def test_a_contracted_multiply_add_would_differ_on_the_tensor_tests_constants():
    scale, bias = gl.constants(gl.MEAN, gl.STD)
    assert int(fma_differs([scale] * 3, [bias] * 3)[0].sum()) == 124
    b = np.arange(256, dtype=np.uint8)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        want = torch.from_numpy(b).float().mul(float(scale)).add(float(bias)).to(dtype)
        assert torch.equal(gl.tensor_of(b, scale, bias, dtype), want)


# ---- the Python entry points: routing and refusals, no GPU ---------------------------------------------------------------------
def _gray_streams():
    return [ChanCase("chan_g_odd_q10").encoded, ChanCase("chan_g_tiny_r7").encoded]


def test_a_list_of_gray_streams_is_described_on_the_host(no_gpu):
    from lrf_amd.codec import _gray_factors_ragged
    from lrf_amd import _lib
    streams = _gray_streams()
    images, U, V = _gray_factors_ragged(streams)
    uo = vo = 0
    for (H, W, R, u_off, v_off), name in zip(images, ("chan_g_odd_q10", "chan_g_tiny_r7")):
        c, u, v, Hc, Wc = _fixture_factors(name)
        assert (H, W, R, u_off, v_off) == (Hc, Wc, c.R, uo, vo)
        assert np.array_equal(U[uo:uo + u.size].reshape(u.shape), u) and np.array_equal(V[vo:vo + v.size].reshape(v.shape), v)
        uo, vo = uo + u.size, vo + v.size
    assert _lib.check_gray_images(torch.from_numpy(U), torch.from_numpy(V), images) == images
    colour = np.load(os.path.join(GOLDEN, "rgbsp_tiny_q4.npz"))["encoded"].tobytes()
    ycc = np.load(os.path.join(GOLDEN, "tiny_q7.npz"))["encoded"].tobytes()
    for other in ([streams[0], colour], [ycc, streams[0]], [ycc], [], b"bytes", [streams[0], "text"], [ChanCase("chan_g_p4_q10").encoded],
                  [ChanCase("chan_c2_q5").encoded], [streams[0][:40]]):
        assert _gray_factors_ragged(other) is None
    with pytest.raises(AssertionError, match="a GPU context was asked for"):
        import lrf_amd
        lrf_amd.qmf_load_factors(streams)  # and a good list does reach the GPU


def test_mixed_lists_keep_their_present_errors(no_gpu):
    import lrf_amd
    gray = _gray_streams()[0]
    ycc = np.load(os.path.join(GOLDEN, "tiny_q7.npz"))["encoded"].tobytes()
    colour = np.load(os.path.join(GOLDEN, "rgbsp_tiny_q4.npz"))["encoded"].tobytes()
    for streams in ([ycc, gray], [gray, ycc], [gray, colour]):
        for call in (lambda s: lrf_amd.qmf_decode_ragged(s), lambda s: lrf_amd.qmf_load_factors(s), lambda s: lrf_amd.qmf_decode_scaled(s, 2),
                     lambda s: lrf_amd.qmf_decode_crops(s, [(0, 0, 0)], (4, 4)), lambda s: lrf_amd.qmf_decode_resized_crops(s, [(0, 0, 0, 5, 5)], (5, 7))):
            with pytest.raises(NotImplementedError, match="RGB"):
                call(streams)


def test_inflate_on_the_device_is_refused_for_gray_lists(no_gpu):
    import lrf_amd
    streams = _gray_streams()
    for call in (lambda: lrf_amd.qmf_decode_ragged(streams, inflate="device"), lambda: lrf_amd.qmf_load_factors(streams, inflate="device"),
                 lambda: lrf_amd.qmf_decode_scaled(streams, 2, inflate="device"),
                 lambda: lrf_amd.qmf_decode_crops(streams, [(0, 0, 0)], (4, 4), inflate="device"),
                 lambda: lrf_amd.qmf_decode_resized_crops(streams, [(0, 0, 0, 5, 5)], (5, 7), inflate="device")):
        with pytest.raises(NotImplementedError, match="inflate"):
            call()
    with pytest.raises(ValueError):
        lrf_amd.qmf_decode_ragged(streams, inflate="gpu")


def test_crops_are_refused_before_a_gpu_is_asked_for(no_gpu):
    from lrf_amd import qmf_decode_crops
    streams = _gray_streams()  # 37x53 and the tiny one
    H, W = 37, 53
    for crops, size, scale in (([(0, H - 3, 0)], (4, 4), 1), ([(0, 0, W - 3)], (4, 4), 1), ([(0, -1, 0)], (4, 4), 1), ([(2, 0, 0)], (4, 4), 1),
                               ([(0, 0, 0)], (H + 1, 4), 1), ([(0, 17, 0)], (3, 3), 2), ([(0, 0, 5)], (3, 3), 8), ([(0, 0, 0)], (4, 4), 3),
                               ([(0, 0, 0), (0, 0, 0)], (4, 4), [1, 16]), ([(0, 0, 0)], (0, 4), 1), ([(0, 0)], (4, 4), 1), ([], (4, 4), 1)):
        with pytest.raises(ValueError):
            qmf_decode_crops(streams, crops, size, scale=scale)
    with pytest.raises(TypeError):
        qmf_decode_crops(streams, [(0, 0.5, 0)], (4, 4))
    with pytest.raises(TypeError):
        qmf_decode_crops(streams, [(0, 0, 0)], (4, 4), scale=2.0)
    with pytest.raises(AssertionError, match="a GPU context was asked for"):
        qmf_decode_crops(streams, [(0, 16, 24), (0, 0, 0)], (3, 3), scale=[2, 8])  # the last windows of their levels: good


def test_resized_boxes_and_scales_are_refused_before_a_gpu_is_asked_for(no_gpu):
    from lrf_amd import qmf_decode_resized_crops, qmf_decode_scaled
    streams = _gray_streams()
    for boxes, size in (([(0, 0, 0, 38, 5)], (5, 7)), ([(0, 30, 0, 8, 5)], (5, 7)), ([(0, 0, 50, 5, 4)], (5, 7)), ([(0, 0, 0, 0, 5)], (5, 7)),
                        ([(5, 0, 0, 5, 5)], (5, 7)), ([(0, 0, 0, 5, 5)], (0, 7)), ([(0, 0, 0, 5, 5)], (5, 16385)), ([(0, 0, 0, 5)], (5, 7))):
        with pytest.raises(ValueError):
            qmf_decode_resized_crops(streams, boxes, size)
    with pytest.raises(TypeError):
        qmf_decode_resized_crops(streams, [(0, 0, 0, 5, 5)], (5, 7), flip=1)
    for scale in (1, 3, 16):
        with pytest.raises(ValueError):
            qmf_decode_scaled(streams, scale)
    with pytest.raises(TypeError):
        qmf_decode_scaled(streams, 2.0)


def test_the_tensor_arguments_of_a_gray_source(no_gpu):
    from lrf_amd import _lib, qmf_decode_crops, qmf_decode_resized_crops
    streams = _gray_streams()
    for bad in (dict(mean=(0.485, 0.456, 0.406)), dict(std=[0.229, 0.224, 0.225]), dict(mean=(0.4, 0.5)), dict(std=0.0), dict(std=[0.0]),
                dict(mean=float("nan"))):
        with pytest.raises(ValueError):
            qmf_decode_crops(streams, [(0, 0, 0)], (4, 4), dtype=torch.float16, **bad)
        with pytest.raises(ValueError):
            qmf_decode_resized_crops(streams, [(0, 0, 0, 5, 5)], (5, 7), dtype=torch.float32, **bad)
    with pytest.raises(ValueError):
        qmf_decode_crops(streams, [(0, 0, 0)], (4, 4), mean=0.5)  # the byte entry takes no mean
    with pytest.raises(ValueError):
        qmf_decode_crops(streams, [(0, 0, 0)], (4, 4), dtype=torch.float64)
    with pytest.raises(TypeError):
        qmf_decode_crops(streams, [(0, 0, 0)], (4, 4), dtype=torch.float16, mean="0.5")
    # one number and a sequence of one are the same format; only element 0 is the gray entries'
    a = _lib.check_gray_tensor_request("t", torch.float16, gl.MEAN, gl.STD, False, None)
    b = _lib.check_gray_tensor_request("t", torch.float16, [gl.MEAN], (gl.STD,), True, None)
    scale, bias = gl.constants(gl.MEAN, gl.STD)
    assert (a.scale[0], a.bias[0]) == (b.scale[0], b.bias[0]) == (float(scale), float(bias)) and (a.layout, b.layout) == (_lib.T_NCHW, _lib.T_NHWC)
    # out= is checked for [n, 1, h, w]
    for out in (torch.empty((2, 3, 4, 4), dtype=torch.float16), torch.empty((2, 1, 4, 4), dtype=torch.float32), torch.empty((2, 1, 4, 8), dtype=torch.float16)[..., ::2]):
        with pytest.raises(ValueError):
            _lib._gray_tensor_output("t", out, 2, 4, 4, torch.float16, out.device)
    big = torch.empty((5, 1, 4, 4), dtype=torch.float16)
    assert _lib._gray_tensor_output("t", big[1:3], 2, 4, 4, torch.float16, big.device).data_ptr() == big[1:3].data_ptr()


def test_the_header_declares_the_entries_the_binding_exports():
    from lrf_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "lrf_hip.h")).read()
    for name in ("lrf_qmf_decode_gray_ragged_u8", "lrf_qmf_decode_gray_crops_u8", "lrf_qmf_decode_gray_crops_tensor",
                 "lrf_qmf_decode_gray_resized_crops_u8", "lrf_qmf_decode_gray_resized_crops_tensor"):
        assert name in _lib.EXPORTS and name + "(" in header and hasattr(_lib.load(), name)
    assert "} lrf_gray_image;" in header
