"""CPU suite: the list forms of qmf_encode_target / qmf_encode_budget without a GPU — every refusal before a context is asked for,
the choice with a per-image sample count on hand-made integer tables, the bpp to bytes conversion per image, and the
declarations of the two C entries behind them."""
import math
import os

import pytest
import torch

from conftest import ROOT

SIZES = [(48, 64), (40, 56), (33, 47)]


@pytest.fixture()
def no_gpu(monkeypatch):
    """every refusal below must come before a context is asked for: asking for one fails the test"""
    from lrf_amd import _lib

    def refuse(device=None):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(_lib, "context", refuse)


def _images():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for H, W in SIZES]


def _both(**common):
    import lrf_amd
    return ((lrf_amd.qmf_encode_target, dict(psnr=30.0, **common)), (lrf_amd.qmf_encode_budget, dict(nbytes=500, **common)))


def test_exported_declared_and_bound():
    import lrf_amd
    from lrf_amd import _lib
    assert "qmf_stream_sizes_ragged" in lrf_amd.__all__ and callable(lrf_amd.qmf_stream_sizes_ragged)
    text = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    assert "int lrf_qmf_encode_ragged_sweep_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_sweep_image* images" in text
    assert "int lrf_qmf_sse_ragged_rgb_u8(lrf_ctx* ctx, int64_t n, const lrf_ragged_image* items" in text
    for name in ("lrf_qmf_encode_ragged_sweep_rgb_u8", "lrf_qmf_sse_ragged_rgb_u8"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert hasattr(_lib.Context, "encode_ragged_sweep") and hasattr(_lib.Context, "sse_ragged")
    src = open(os.path.join(ROOT, "lrf_amd", "csrc", "lrf_encode8.hip")).read()
    body = src[src.index("int lrf_qmf_sse_ragged_rgb_u8("):]
    assert "Prof p(c, LRF_K_DECODE)" in body[:body.index("\n}\n")]  # timed with the decoders
    assert os.path.exists(os.path.join(ROOT, "lrf_amd", "csrc", "lrf_sse_ragged_kernel.hip"))


def test_image_refusals_need_no_gpu(no_gpu):
    ims = _images()
    for fn, kw in _both():
        with pytest.raises(NotImplementedError, match="image 2.*uint8"):
            fn(ims[:2] + [ims[2].float()], **kw)
        with pytest.raises(TypeError, match="image 1"):
            fn([ims[0], ims[1].numpy()], **kw)
        with pytest.raises(ValueError, match="image 1"):
            fn([ims[0], ims[1][0]], **kw)              # [H,W]: wrong rank
        with pytest.raises(ValueError, match="image 0"):
            fn([ims[0][:2]] + ims[1:], **kw)           # two channels
        with pytest.raises(ValueError, match="image 1"):
            fn([ims[0], torch.zeros((4, 16, 16), dtype=torch.uint8)], **kw)
        with pytest.raises(ValueError, match="image 1"):
            fn([ims[0], torch.zeros((3, 0, 16), dtype=torch.uint8)], **kw)
        with pytest.raises(TypeError, match="batch"):
            fn([torch.stack([ims[0], ims[0]])], **kw)  # a batch inside a list: the tensor form takes batches
        for empty in ([], ()):
            with pytest.raises(ValueError, match="non-empty"):
                fn(empty, **kw)
        with pytest.raises(ValueError, match="one device"):
            fn([ims[0], ims[1].to("meta")], **kw)
        with pytest.raises(NotImplementedError, match="num_iters"):
            fn(ims, num_iters=0, **kw)
        for q in ([], [5, 101], [-1]):
            with pytest.raises(ValueError, match="qualities"):
                fn(ims, qualities=q, **kw)
        with pytest.raises(ValueError, match="x_workspace_bytes"):
            fn(ims, x_workspace_bytes=0, **kw)
        with pytest.raises(ValueError, match="deflate") if "psnr" in kw else pytest.raises(TypeError):
            fn(ims, deflate="gpu", **kw)               # (the budget is met by device streams: it has no such keyword)


def test_a_quality_whose_triple_passes_rank_32_is_refused_with_its_image_and_quality(no_gpu):
    """min(M, 64) q / 100 > 32.5 needs q > 50 and a luma plane of 64 patches or more: 64x64 has 64, 48x64 has 48 (round(48 q / 100)
    passes 32 from q = 68), 33x47 has 30 and never does.  The default grid 1..32 gives at most round(64 * 0.32) = 20."""
    from lrf_amd import qmf_ranks
    big = torch.zeros((3, 64, 64), dtype=torch.uint8)
    ims = _images()
    assert max(qmf_ranks((64, 64), quality=51)) == 33 and max(qmf_ranks((64, 64), quality=50)) == 32
    assert max(qmf_ranks((48, 64), quality=68)) == 33 and max(qmf_ranks((48, 64), quality=67)) == 32 and max(qmf_ranks((33, 47), quality=100)) == 30
    for fn, kw in _both():
        with pytest.raises(NotImplementedError, match=r"image 3 \(64x64\) at quality 51"):
            fn(ims + [big], qualities=(3, 51, 40), **kw)   # (the other sizes stay within rank 32 at 51)
        with pytest.raises(NotImplementedError, match=r"image 0 \(48x64\) at quality 68"):
            fn(ims + [big], qualities=(50, 68), **kw)
        with pytest.raises(NotImplementedError, match=r"image 1 \(64x64\) at quality 60"):
            fn([ims[2], big], qualities=(60, 100), **kw)
    from lrf_amd.codec import _check_rate_list_args
    qs, sizes, cands = _check_rate_list_args(ims + [big], range(1, 33), 10, "qmf_encode_target")  # the default grid passes
    assert sizes == SIZES + [(64, 64)] and max(r for ts, _, _ in cands for t in ts for r in t) == 20
    # per size, which of its triples every quality (ascending) has: neighbours that round to the same ranks share a row
    for (ts, lowest, rows), hw in zip(cands, sizes):
        assert [ts[r] for r in rows] == [tuple(qmf_ranks(hw, quality=q)) for q in range(1, 33)] and rows == sorted(rows) and rows[-1] == len(ts) - 1
    assert _check_rate_list_args(ims + [big], (50, 3), 10, "qmf_encode_target")[0] == [50, 3]


def test_goal_counts_are_refused(no_gpu):
    import lrf_amd
    ims = _images()
    for bad in ([30.0, 31.0], [30.0] * 4, float("nan"), [30.0, float("nan"), 30.0]):
        with pytest.raises(ValueError, match="psnr"):
            lrf_amd.qmf_encode_target(ims, bad)
    for key in ("bpp", "nbytes"):
        for bad in ([1.0, 2.0], [1.0] * 4, float("nan"), -1.0, [1.0, -0.5, 1.0]):
            with pytest.raises(ValueError, match=key):
                lrf_amd.qmf_encode_budget(ims, **{key: bad})
        with pytest.raises(TypeError, match=key):
            lrf_amd.qmf_encode_budget(ims, **{key: [True, False, True]})
    with pytest.raises(ValueError, match="exactly one"):
        lrf_amd.qmf_encode_budget(ims)
    with pytest.raises(ValueError, match="exactly one"):
        lrf_amd.qmf_encode_budget(ims, bpp=1.0, nbytes=100)


def test_bpp_becomes_bytes_with_each_images_own_size():
    from lrf_amd.codec import budget_bytes_per_image
    sizes = [(48, 64), (40, 56), (33, 47), (512, 768)]
    got = budget_bytes_per_image(sizes, bpp=0.25)
    assert got.dtype == torch.int64 and got.tolist() == [96, 70, 48, 12288]  # 33 * 47 * 0.25 / 8 = 48.47
    assert budget_bytes_per_image(sizes, bpp=[1.0, 0.5, 0.3, 0.0]).tolist() == [384, 140, math.floor(0.3 * 33 * 47 / 8), 0]
    assert budget_bytes_per_image(sizes, nbytes=[10, 20.9, 30, 2 ** 40]).tolist() == [10, 20, 30, 2 ** 40]
    assert budget_bytes_per_image(sizes, nbytes=77).tolist() == [77] * 4
    # one size: what the tensor form computes
    from lrf_amd.codec import _check_budget_args
    batch = torch.zeros((3, 3, 40, 56), dtype=torch.uint8)
    for bpp in (0.25, [0.1, 0.77, 3.0]):
        assert torch.equal(budget_bytes_per_image([(40, 56)] * 3, bpp=bpp), _check_budget_args(batch, bpp, None, [5], 10)[1])


def test_select_target_with_a_count_per_image():
    """three images of 3 x 10, 3 x 1000 and 3 x 100000 samples with the SAME squared errors: the PSNR differs by 20 dB a step, so one
    target picks another candidate in each column"""
    from lrf_amd.codec import select_target
    from lrf_amd.metrics import psnr_from_sse
    sse = torch.tensor([[40000, 40000, 40000], [4000, 4000, 4000], [400, 400, 400], [0, 40, 40]], dtype=torch.int64)
    n = torch.tensor([30, 3000, 300000], dtype=torch.int64)
    psnr = lambda s, k: math.inf if s == 0 else 20 * math.log10(255 / math.sqrt(s / k))
    table, index, reached = select_target(sse, n, torch.tensor([40.0, 50.0, 66.0], dtype=torch.float64))
    want = [[psnr(int(sse[q, b]), int(n[b])) for b in range(3)] for q in range(4)]
    assert table.dtype == torch.float64 and torch.allclose(table, torch.tensor(want, dtype=torch.float64), rtol=1e-12) and math.isinf(table[3, 0])
    # column 0 (16.9, 26.9, 36.9, inf dB): 40 dB first at row 3; column 1 (36.9, 46.9, 56.9, 66.9): 50 dB at row 2; column 2
    # (56.9, 66.9, ...): 66 dB at row 1
    assert index.tolist() == [3, 2, 1] and reached.tolist() == [True, True, True]
    _, index, reached = select_target(sse, n, torch.tensor([10.0, 90.0, 80.0], dtype=torch.float64))
    # column 1: none reaches 90 dB, the best is row 3 (66.9); column 2 (56.9, 66.9, 76.9, 86.9): 80 dB at row 3
    assert index.tolist() == [0, 3, 3] and reached.tolist() == [True, False, True]
    # an integer count gives what it gave before, and equals a constant tensor of counts
    t_int, i_int, r_int = select_target(sse, 3000, torch.tensor([50.0] * 3, dtype=torch.float64))
    t_vec, i_vec, r_vec = select_target(sse, torch.full((3,), 3000, dtype=torch.int64), torch.tensor([50.0] * 3, dtype=torch.float64))
    assert torch.equal(t_int, t_vec) and torch.equal(i_int, i_vec) and torch.equal(r_int, r_vec)
    assert torch.equal(t_int, 20 * torch.log10(255 / torch.sqrt(sse.double() / 3000)))
    m, p = psnr_from_sse(sse, n)
    assert torch.equal(m, sse.double() / n.double()) and torch.equal(p, table)
    # a column is the integer form's for its count, by construction: repeated and unsorted counts, every column against the integer call
    wide = torch.arange(1, 4 * 7 + 1, dtype=torch.int64).reshape(4, 7) * 977
    counts = torch.tensor([4653, 3000, 4653, 7, 3000, 12288, 7], dtype=torch.int64)
    mw, pw = psnr_from_sse(wide, counts)
    for b, k in enumerate(counts.tolist()):
        mi, pi = psnr_from_sse(wide[:, b:b + 1], k)
        assert torch.equal(mw[:, b:b + 1], mi) and torch.equal(pw[:, b:b + 1], pi)
    with pytest.raises(ValueError, match="counts"):
        psnr_from_sse(wide, counts[:3])  # one count per column, nothing broadcasts silently


def test_select_budget_on_tables_gathered_per_image():
    """select_budget takes no sample count: the list form hands it [Q,B] tables gathered from per-candidate vectors.  Here the
    gather itself, with duplicate rows where two qualities share a triple (the first of them must win: the lowest quality)"""
    from lrf_amd.codec import select_budget
    size_vec = torch.tensor([100, 200, 300, 150, 250, 90], dtype=torch.int64)   # candidates: image 0 has three, image 1 two, image 2 one
    sse_vec = torch.tensor([900, 500, 100, 800, 300, 50], dtype=torch.int64)
    row = torch.tensor([[0, 3, 5], [1, 3, 5], [1, 4, 5], [2, 4, 5]])            # [quality, image] -> candidate
    size, sse = size_vec[row], sse_vec[row]
    index, reached = select_budget(size, sse, torch.tensor([250, 200, 10], dtype=torch.int64))
    assert index.tolist() == [1, 0, 0] and reached.tolist() == [True, True, False]
    index, reached = select_budget(size, sse, torch.tensor([1000, 1000, 1000], dtype=torch.int64))
    assert index.tolist() == [3, 2, 0] and reached.tolist() == [True, True, True]


def test_context_checks_its_arguments_without_a_device():
    from lrf_amd._lib import check_encode_ragged_sweep_args, check_sse_ragged_args
    rgb = torch.zeros(2 * 3 * 64 * 96 + 16, dtype=torch.uint8)
    ims, cds = check_encode_ragged_sweep_args(rgb, [(64, 96, 16), (64, 96, 16 + 3 * 64 * 96, None)], [(1, (7, 3, 3)), (0, (12, 6, 6)), (1, (3, 5, 1))])
    assert ims == [(64, 96, 16, -1), (64, 96, 16 + 3 * 64 * 96, -1)] and cds == [(1, [7, 3, 3]), (0, [12, 6, 6]), (1, [3, 5, 1])]
    one = [(64, 96, 0)]
    for bad_ims, bad_cds in ((one, []), (one, [(1, (7, 3, 3))]), (one, [(-1, (7, 3, 3))]), (one, [(0, (33, 3, 3))]), (one, [(0, (7, 0, 3))]),
                             (one, [(0, (7, 3))]), ([(64, 96, 3 * 64 * 96 + 17)], [(0, (7, 3, 3))]), ([(64, 96, -1)], [(0, (7, 3, 3))]),
                             ([(0, 96, 0)], [(0, (7, 3, 3))]), ([], []), (one + [(64, 96, 16)], [(0, (7, 3, 3)), (0, (8, 3, 3))]),
                             ([(64, 96, 0, 0)], [(0, (7, 3, 3))])):
        with pytest.raises(ValueError):
            check_encode_ragged_sweep_args(rgb, bad_ims, bad_cds)
    sign = torch.ones(12 + 6 + 5, dtype=torch.int8)  # the largest rank per channel over the image's candidates: (12, 6, 5)
    cands = [(0, (12, 3, 5)), (0, (7, 6, 1))]
    assert check_encode_ragged_sweep_args(rgb, [(64, 96, 0, 0)], cands, sign)[0][0][3] == 0
    with pytest.raises(ValueError, match="signs"):
        check_encode_ragged_sweep_args(rgb, [(64, 96, 0, 1)], cands, sign)
    with pytest.raises(TypeError):
        check_encode_ragged_sweep_args(rgb.float(), one, [(0, (7, 3, 3))])
    with pytest.raises(TypeError):
        check_encode_ragged_sweep_args(rgb, [(64, 96, 0, 0)], cands, sign.float())
    from lrf_amd import _lib
    nu, nv = sum(d[4] * r for d, r in zip(_lib.plane_dims(64, 96), (7, 3, 3))), 64 * 13
    U, V = torch.zeros(nu + 4, dtype=torch.int8), torch.zeros(nv + 4, dtype=torch.int8)
    ok = (64, 96, (7, 3, 3), 4, 4, 16)
    assert check_sse_ragged_args(rgb, [ok, ok], U, V) == [(64, 96, [7, 3, 3], 4, 4, 16)] * 2  # sources (and factors) may be shared
    for bad in ([ok[:5]], [ok[:3] + (5, 4, 16)], [ok[:4] + (5, 16)], [ok[:5] + (3 * 64 * 96 + 17,)], [ok[:5] + (-1,)], [(64, 96, (65, 3, 3), 4, 4, 16)], []):
        with pytest.raises(ValueError):
            check_sse_ragged_args(rgb, bad, U, V)
    with pytest.raises(TypeError):
        check_sse_ragged_args(rgb.float(), [ok], U, V)
    with pytest.raises(TypeError):
        check_sse_ragged_args(rgb, [ok], U.float(), V)
