"""No GPU: the selection rule of qmf_encode_target on hand-made squared-error tables, its argument refusals (raised before a
context exists), and the declaration of the new export."""
import math
import os

import pytest
import torch

from conftest import ROOT

N = 3 * 8 * 8  # samples per "image" of the hand-made tables


def _sse_for(psnr_db):
    """an integer squared error whose PSNR over N samples is close to psnr_db (the tests read the table back, not this)"""
    return int(round(N * (255.0 / 10 ** (psnr_db / 20)) ** 2))


def _select(rows, target):
    from lrf_amd.codec import select_target
    sse = torch.tensor(rows, dtype=torch.int64)
    t = torch.as_tensor(target, dtype=torch.float64).reshape(-1).expand(sse.shape[1])
    return select_target(sse, N, t)


def test_table_is_the_psnr_expression_of_image_metrics_batch():
    from lrf_amd.metrics import psnr_from_sse
    sse = torch.tensor([[5, 0], [123456, 7]], dtype=torch.int64)
    table, _, _ = _select(sse.tolist(), 30.0)
    m, p = psnr_from_sse(sse, N)
    assert table.dtype == torch.float64 and torch.equal(table, p) and torch.equal(m, sse.double() / N)
    assert abs(table[0, 0].item() - 20 * math.log10(255 / math.sqrt(5 / N))) < 1e-12
    assert math.isinf(table[0, 1].item()) and table[0, 1].item() > 0


def test_first_candidate_that_reaches_the_target_wins():
    # image 0 grows 25, 31, 33, 36 dB; image 1 is flat at 40 dB
    rows = [[_sse_for(25), _sse_for(40)], [_sse_for(31), _sse_for(40)], [_sse_for(33), _sse_for(40)], [_sse_for(36), _sse_for(40)]]
    table, index, reached = _select(rows, 32.0)
    assert index.tolist() == [2, 0] and reached.tolist() == [True, True]
    # a tie on the target itself counts as reached: target = the table's own value
    _, index, reached = _select(rows, table[1, 0].item())
    assert index.tolist() == [1, 0] and reached.tolist() == [True, True]


def test_non_monotone_rows_are_searched_whole():
    # 25, 34, 29, 35 dB: the first candidate >= 32 is number 1 although number 2 falls below again;
    # and for a target of 34.5 the answer is number 3, past the dip
    rows = [[_sse_for(25)], [_sse_for(34)], [_sse_for(29)], [_sse_for(35)]]
    assert _select(rows, 32.0)[1].tolist() == [1]
    assert _select(rows, 34.5)[1].tolist() == [3]
    # none reached, and the best is not the last: 25, 34, 29, 33 against 50 dB
    rows[3] = [_sse_for(33)]
    _, index, reached = _select(rows, 50.0)
    assert index.tolist() == [1] and reached.tolist() == [False]


def test_none_reached_takes_the_first_of_equal_best():
    rows = [[900], [400], [400], [700]]
    _, index, reached = _select(rows, 99.0)
    assert index.tolist() == [1] and reached.tolist() == [False]


def test_zero_error_is_infinite_psnr_and_reaches_everything():
    rows = [[50, 0], [0, 0], [10, 3]]
    table, index, reached = _select(rows, 1e9)
    assert index.tolist() == [1, 0] and reached.tolist() == [True, True]
    assert math.isinf(table[1, 0].item())


def test_per_image_targets():
    rows = [[_sse_for(25), _sse_for(25)], [_sse_for(31), _sse_for(31)], [_sse_for(36), _sse_for(36)]]
    _, index, reached = _select(rows, [30.0, 40.0])
    assert index.tolist() == [1, 2] and reached.tolist() == [True, False]


def test_candidates_are_distinct_triples_with_their_lowest_quality():
    from lrf_amd.codec import qmf_ranks, target_candidates
    triples, lowest = target_candidates((512, 768), [5, 1, 3, 2, 4, 2])
    assert len(set(triples)) == len(triples) and lowest == sorted(lowest)
    for t, q in zip(triples, lowest):
        assert t == tuple(qmf_ranks((512, 768), None, q))
        assert all(tuple(qmf_ranks((512, 768), None, p)) != t for p in [1, 2, 3, 4, 5] if p < q)
    assert {tuple(qmf_ranks((512, 768), None, p)) for p in [1, 2, 3, 4, 5]} == set(triples)


def test_argument_refusals_need_no_gpu(monkeypatch):
    import lrf_amd
    from lrf_amd import _lib

    def no_context(*a, **k):
        raise AssertionError("a context was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "context", no_context)
    img = torch.zeros((2, 3, 16, 16), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="uint8"):
        lrf_amd.qmf_encode_target(img.float(), 30.0)
    with pytest.raises(NotImplementedError, match="num_iters"):
        lrf_amd.qmf_encode_target(img, 30.0, num_iters=0)
    for bad in (img[0], img[:, :2], img[:0]):
        with pytest.raises(ValueError):
            lrf_amd.qmf_encode_target(bad, 30.0)
    with pytest.raises(ValueError, match="psnr"):
        lrf_amd.qmf_encode_target(img, [30.0, 31.0, 32.0])
    with pytest.raises(ValueError, match="psnr"):
        lrf_amd.qmf_encode_target(img, float("nan"))
    with pytest.raises(ValueError, match="qualities"):
        lrf_amd.qmf_encode_target(img, 30.0, qualities=[])
    with pytest.raises(ValueError, match="qualities"):
        lrf_amd.qmf_encode_target(img, 30.0, qualities=[5, 101])
    with pytest.raises(TypeError):
        lrf_amd.qmf_encode_target([img], 30.0)
    # the kernel's public face refuses misshapen factors on host tensors alike
    U = torch.zeros((2, 10), dtype=torch.int8)
    with pytest.raises(ValueError):
        lrf_amd.sweep_sse_batch(img, [(U, U)], [(1, 1, 1)])
    with pytest.raises(ValueError):
        lrf_amd.sweep_sse_batch(img, None, [(1, 1, 1)])
    with pytest.raises(TypeError):
        lrf_amd.sweep_sse_batch(img.float(), [(U, U)], [(1, 1, 1)])


def test_the_export_is_declared_and_bound():
    from lrf_amd import _lib
    text = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    assert "int lrf_qmf_sweep_sse_rgb_u8(lrf_ctx* ctx, const uint8_t* rgb" in text
    assert "lrf_qmf_sweep_sse_rgb_u8" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "lrf_amd", "csrc", "lrf_encode8.hip")).read()
    assert "Prof p(c, LRF_K_METRICS)" in src  # timed as the scoring stage, with lrf_image_metrics_u8
    assert hasattr(_lib.load(), "lrf_qmf_sweep_sse_rgb_u8") and hasattr(_lib.Context, "sweep_sse")
