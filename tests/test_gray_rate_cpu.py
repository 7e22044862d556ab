"""CPU suite: the gray forms of qmf_encode_ragged / qmf_encode_target / qmf_encode_budget (color_space="RGB") without a GPU — the
two-factor container arithmetic against folds by the container code, every argument refusal before a context is asked for, the
argument checks of the three Context wrappers, and the default-keyword calls, which refuse gray input as they always did."""
import zlib

import numpy as np
import pytest
import torch

from lrf_amd.container import combine_bytes, dict_to_bytes, separate_bytes


@pytest.fixture
def no_gpu(monkeypatch):
    """every refusal below must come before a context is asked for: asking for one fails the test"""
    from lrf_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(_lib, "context", refuse)


def gray(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_exported_declared_and_bound():
    import os

    import lrf_amd
    from lrf_amd import _lib
    for name in ("container_bytes_two_factor", "qmf_stream_sizes_gray_ragged"):
        assert name in lrf_amd.__all__ and callable(getattr(lrf_amd, name))
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lrf_hip.h")).read()
    for name in ("lrf_qmf_encode_gray_ragged_u8", "lrf_qmf_encode_gray_ragged_sweep_u8", "lrf_qmf_sse_gray_ragged_u8"):
        assert f"int {name}(lrf_ctx* ctx, int64_t n, " in text and name in _lib.EXPORTS
    assert all(hasattr(_lib.Context, m) for m in ("encode_gray_ragged", "encode_gray_ragged_sweep", "sse_gray_ragged"))


@pytest.mark.parametrize("R", [1, 2, 9, 10, 32])
def test_container_bytes_two_factor_equals_the_fold(R):
    """len() of a fold in _two_factor_stream's layout, the columns arbitrary byte strings (R = 9 -> 10: the JSON headers gain a digit)"""
    from lrf_amd import container_bytes_two_factor
    from lrf_amd.codec import _two_factor_metadata
    rng = np.random.default_rng(R)
    meta = _two_factor_metadata("uint8", (-16, 15), (8, 8), (37, 53), (40, 56), R)
    lens = rng.integers(1, 700, 2 * R)
    cols = [bytes(rng.integers(0, 256, int(n), dtype=np.uint8)) for n in lens]
    header = dict_to_bytes({"num_fibers": R, "mode": "col", "dtype": "int8"})
    fold = combine_bytes([meta, combine_bytes([combine_bytes([header, combine_bytes(cols[:R])]), combine_bytes([header, combine_bytes(cols[R:])])])])
    assert int(container_bytes_two_factor(len(meta), R, lens)) == len(fold)
    assert int(container_bytes_two_factor(len(meta), R, torch.from_numpy(lens[::-1].copy()))) == len(fold)  # (any order, a tensor)
    many = container_bytes_two_factor(len(meta), R, np.stack([lens, lens + 1]))
    assert many.tolist() == [len(fold), len(fold) + 2 * R]
    # and the fold parses as the container does: metadata, then two factors of R columns
    m, body = separate_bytes(fold, 2)
    assert m == meta and all(len(separate_bytes(separate_bytes(f, 2)[1], R)) == R for f in separate_bytes(body, 2))


@pytest.mark.parametrize("R", [1, 10])
def test_container_bytes_two_factor_equals_two_factor_stream(R):
    """the host container itself: _two_factor_stream of int8 factors, its columns' zlib-9 lengths"""
    from lrf_amd import container_bytes_two_factor
    from lrf_amd.codec import _two_factor_metadata, _two_factor_stream
    rng = np.random.default_rng(10 + R)
    u, v = rng.integers(-16, 16, (35, R), dtype=np.int8), rng.integers(-16, 16, (64, R), dtype=np.int8)
    stream = _two_factor_stream("uint8", (-16, 15), (8, 8), (37, 53), (40, 56), R, [u, v])
    lens = [len(zlib.compress(np.ascontiguousarray(f[:, j]).tobytes(), 9)) for f in (u, v) for j in range(R)]
    assert int(container_bytes_two_factor(len(_two_factor_metadata("uint8", (-16, 15), (8, 8), (37, 53), (40, 56), R)), R, lens)) == len(stream)


def test_container_bytes_two_factor_refuses():
    from lrf_amd import container_bytes_two_factor
    for R, lens in [(0, []), (3, [1, 2, 3]), (2, [1, 2, 3, 4, 5])]:
        with pytest.raises(ValueError, match="2 R column lengths"):
            container_bytes_two_factor(10, R, lens)


def test_encode_ragged_gray_refusals_need_no_gpu(no_gpu):
    import lrf_amd
    ims = [gray(1, 16, 24), gray(1, 37, 53)]
    enc = lambda images=ims, **kw: lrf_amd.qmf_encode_ragged(images, color_space="RGB", **kw)
    with pytest.raises(ValueError, match="'ranks' is refused"):
        enc(ranks=(4, 2, 2))
    with pytest.raises(ValueError, match="exactly one of 'rank' and 'quality'"):
        enc()
    with pytest.raises(ValueError, match="exactly one of 'rank' and 'quality'"):
        enc(rank=2, quality=5)
    with pytest.raises(ValueError, match="one value or one per image"):
        enc(rank=[1, 2, 3])
    with pytest.raises(ValueError, match="scalar rank"):
        enc(rank=[(4, 2, 2), (4, 2, 2)])
    with pytest.raises(ValueError, match=">= 1"):
        enc(rank=[2, 0])
    with pytest.raises(NotImplementedError, match="gray images"):
        enc(images=[gray(1, 16, 24), gray(3, 16, 24)], rank=2)
    with pytest.raises(NotImplementedError, match="gray images"):
        enc(images=gray(2, 3, 16, 24), rank=2)
    with pytest.raises(ValueError, match=r"must be \[1,H,W\]"):
        enc(images=[gray(2, 16, 24)], rank=2)
    with pytest.raises(ValueError, match="tensor of shape"):
        enc(images=gray(16, 24), rank=2)
    with pytest.raises(ValueError, match="non-empty"):
        enc(images=[], rank=2)
    with pytest.raises(TypeError, match="not a tensor"):
        enc(images=[np.zeros((1, 16, 24), np.uint8)], rank=2)
    with pytest.raises(NotImplementedError, match="uint8"):
        enc(images=[gray(1, 16, 24).float()], rank=2)
    with pytest.raises(NotImplementedError, match="num_iters"):
        enc(rank=2, num_iters=0)
    with pytest.raises(ValueError, match="init_sign holds 3 signs"):
        enc(rank=2, init_sign=[1, -1, 1])
    with pytest.raises(ValueError, match="deflate"):
        enc(rank=2, deflate="gpu")
    with pytest.raises(ValueError, match="reflect padding"):
        enc(images=[gray(1, 9, 2)], rank=1)
    with pytest.raises(AssertionError, match="color_space"):
        lrf_amd.qmf_encode_ragged(ims, rank=2, color_space="gray")


@pytest.mark.parametrize("call, goal", [("qmf_encode_target", dict(psnr=30.0)), ("qmf_encode_budget", dict(bpp=0.5))])
def test_rate_control_gray_refusals_need_no_gpu(no_gpu, call, goal):
    import lrf_amd
    fn = getattr(lrf_amd, call)
    ims = [gray(1, 16, 24), gray(1, 37, 53)]
    with pytest.raises(NotImplementedError, match="gray images"):
        fn([gray(3, 16, 24)], color_space="RGB", **goal)
    with pytest.raises(NotImplementedError, match="gray images"):
        fn(gray(2, 3, 16, 24), color_space="RGB", **goal)
    with pytest.raises(ValueError, match=r"must be \[1,H,W\]"):
        fn([gray(16, 24)], color_space="RGB", **goal)
    with pytest.raises(ValueError, match="non-empty"):
        fn([], color_space="RGB", **goal)
    with pytest.raises(NotImplementedError, match="num_iters"):
        fn(ims, color_space="RGB", num_iters=0, **goal)
    with pytest.raises(ValueError, match="qualities"):
        fn(ims, color_space="RGB", qualities=[], **goal)
    with pytest.raises(ValueError, match="qualities"):
        fn(ims, color_space="RGB", qualities=[5, 101], **goal)
    with pytest.raises(ValueError, match="one number or one per image"):
        fn(ims, color_space="RGB", **{k: [v, v, v] for k, v in goal.items()})
    with pytest.raises(ValueError, match="x_workspace_bytes"):
        fn(ims, color_space="RGB", x_workspace_bytes=0, **goal)
    # a quality whose rank passes 32: 64x96 has M = 96, min(M, 64) = 64, quality 51 -> rank 33; the image and the quality are named
    with pytest.raises(NotImplementedError, match=r"image 1 \(64x96\) at quality 51 has rank 33"):
        fn([gray(1, 16, 24), gray(1, 64, 96)], color_space="RGB", qualities=[10, 51, 50], **goal)


def test_budget_gray_goal_refusals_need_no_gpu(no_gpu):
    import lrf_amd
    ims = [gray(1, 16, 24)]
    with pytest.raises(ValueError, match="exactly one of 'bpp' and 'nbytes'"):
        lrf_amd.qmf_encode_budget(ims, color_space="RGB")
    with pytest.raises(ValueError, match="exactly one of 'bpp' and 'nbytes'"):
        lrf_amd.qmf_encode_budget(ims, bpp=1, nbytes=100, color_space="RGB")
    with pytest.raises(ValueError, match=">= 0"):
        lrf_amd.qmf_encode_budget(ims, nbytes=-1, color_space="RGB")


def test_gray_candidates_are_the_distinct_ranks_with_their_lowest_quality():
    from lrf_amd.codec import gray_target_candidates
    # 16x24: M = 6, R = max(round(6 q / 100), 1), Python's round (half to even, as the reference): 25 -> round(1.5) = 2, but 75 -> round(4.5) = 4
    ranks, lowest = gray_target_candidates((16, 24), range(1, 101))
    assert ranks == [1, 2, 3, 4, 5, 6] and lowest == [1, 25, 42, 59, 76, 92]
    assert all(max(round(6 * q / 100), 1) == r and max(round(6 * (q - 1) / 100), 1) < r for r, q in zip(ranks[1:], lowest[1:]))
    assert gray_target_candidates((64, 96), [50, 3, 2, 1]) == ([1, 2, 32], [1, 3, 50])


def test_default_keyword_calls_refuse_gray_as_before(no_gpu):
    """color_space defaults to "YCbCr": [1,H,W] input raises exactly what it raised before the keyword existed"""
    import lrf_amd
    ims = [gray(1, 16, 24)]
    with pytest.raises(ValueError) as e:
        lrf_amd.qmf_encode_ragged(ims, rank=2)
    assert str(e.value) == "qmf_encode_ragged: image 0 must be [3,H,W], got (1, 16, 24)"
    with pytest.raises(ValueError) as e:
        lrf_amd.qmf_encode_target(ims, 30.0)
    assert str(e.value) == "qmf_encode_target: image 0 must be [3,H,W], got (1, 16, 24)"
    with pytest.raises(ValueError) as e:
        lrf_amd.qmf_encode_budget(ims, bpp=0.5)
    assert str(e.value) == "qmf_encode_budget: image 0 must be [3,H,W], got (1, 16, 24)"
    with pytest.raises(ValueError) as e:
        lrf_amd.qmf_encode_target(gray(2, 1, 16, 24), 30.0)
    assert str(e.value) == "qmf_encode_target takes a batch [B,3,H,W], got (2, 1, 16, 24)"
    with pytest.raises(ValueError) as e:
        lrf_amd.qmf_encode_budget(gray(2, 1, 16, 24), nbytes=100)
    assert str(e.value) == "qmf_encode_budget takes a batch [B,3,H,W], got (2, 1, 16, 24)"
    with pytest.raises(ValueError) as e:
        lrf_amd.qmf_encode_ragged(gray(2, 1, 16, 24), rank=2)
    assert str(e.value) == "qmf_encode_ragged: image 0 must be [3,H,W], got (1, 16, 24)"
    # and the batch call keeps its refusal of the device coder for gray images
    with pytest.raises(NotImplementedError, match="deflate"):
        lrf_amd.qmf_encode_batch(gray(2, 1, 16, 16), rank=1, color_space="RGB", deflate="device")


def test_context_wrappers_check_their_arguments_without_a_device():
    from lrf_amd._lib import check_encode_gray_ragged_args, check_encode_gray_ragged_sweep_args, check_sse_gray_ragged_args
    g = torch.zeros(64 * 96 + 16 + 37 * 53, dtype=torch.uint8)
    sign = torch.ones(40, dtype=torch.int8)
    assert check_encode_gray_ragged_args(g, [(64, 96, 7, 0), (37, 53, 32, 64 * 96 + 16, 8)], sign) == [(64, 96, 7, 0, -1), (37, 53, 32, 6160, 8)]
    for bad, err in [([(64, 96, 33, 0)], "rank 33"), ([(64, 96, 0, 0)], "rank 0"), ([(64, 96, (7, 3, 3), 0)], "scalar rank"), ([(64, 96, 7, -1)], "leave the buffer"),
                     ([(64, 96, 7, 16 + 37 * 53 + 1)], "leave the buffer"), ([(64, 96, 7, 0, 34)], "signs"), ([(9, 2, 1, 0)], "reflect padding"),
                     ([(64, 96, 7)], "expected"), ([], "1 to 65535")]:
        with pytest.raises(ValueError, match=err):
            check_encode_gray_ragged_args(g, bad, sign)
    with pytest.raises(ValueError, match="signs"):
        check_encode_gray_ragged_args(g, [(64, 96, 7, 0, 0)], None)
    with pytest.raises(TypeError, match="uint8"):
        check_encode_gray_ragged_args(g.float(), [(64, 96, 7, 0)])
    with pytest.raises(TypeError, match="int8"):
        check_encode_gray_ragged_args(g, [(64, 96, 7, 0)], sign.float())
    ims, cds = check_encode_gray_ragged_sweep_args(g, [(64, 96, 0, 0), (37, 53, 6160)], [(1, 3), (0, 32), (1, 9), (0, 1)], sign)
    assert ims == [(64, 96, 0, 0), (37, 53, 6160, -1)] and cds == [(1, 3), (0, 32), (1, 9), (0, 1)]
    for bad_ims, bad_cds, err in [([(64, 96, 0)], [(1, 3)], "out of range"), ([(64, 96, 0), (37, 53, 6160)], [(0, 3), (0, 4)], "image 1 has no candidate"),
                                  ([(64, 96, 0)], [(0, 33)], "rank 33"), ([(64, 96, 0)], [], "a candidate per image"), ([(64, 96, 0, 9)], [(0, 32)], "signs"),
                                  ([(64, 96, 0)], [(0, 3, 1)], "expected")]:
        with pytest.raises(ValueError, match=err):
            check_encode_gray_ragged_sweep_args(g, bad_ims, bad_cds, sign)
    U, V = torch.zeros(96 * 64 + 35 * 5, dtype=torch.int8), torch.zeros(64 * 64 + 64 * 5, dtype=torch.int8)
    items = [(64, 96, 64, 0, 0, 0), (37, 53, 5, 96 * 64, 64 * 64, 6160), (37, 53, 5, 96 * 64, 64 * 64, 6160)]
    assert check_sse_gray_ragged_args(g, items, U, V) == items
    for bad, err in [([(64, 96, 65, 0, 0, 0)], "rank"), ([(64, 96, 64, 176, 0, 0)], "leave the buffers"), ([(37, 53, 5, 0, 0, 6161)], "its source"),
                     ([(37, 53, 5, 0, 0, -1)], "its source"), ([(37, 53, 5, 0, 0)], "expected")]:
        with pytest.raises(ValueError, match=err):
            check_sse_gray_ragged_args(g, bad, U, V)
    with pytest.raises(TypeError, match="uint8"):
        check_sse_gray_ragged_args(g.float(), items, U, V)
