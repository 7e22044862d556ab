"""GPU suite (-m gpu): lrf_deflate_sizes_i8 counts, per column, exactly the bytes the coder writes — against the host restatement
and against lrf_deflate_columns_i8 on the same table — and qmf_stream_sizes gives len() of the deflate="device" streams."""
import numpy as np
import pytest
import torch

import deflate_cases as dc
from conftest import make_image

pytestmark = pytest.mark.gpu
SENTINEL = -77
ROWS = [1, 2, 63, 65, 2047, 2049, 4180, 6144, 65537]


@pytest.fixture(scope="module")
def mixed():
    """One source buffer and one table: a matrix per (rows, content, cols) — column j drawn with seed j — placed at odd offsets
    in an order that is not the table's, their length entries in a third order with gaps between them
    -> (src, table [n, 5], out_len entries, expected length per out_len entry (SENTINEL in the gaps))"""
    from lrf_amd import _lib
    cg = _lib.LRF_DEFLATE_CG
    rng = np.random.default_rng(2024)
    mats = []
    for rows in ROWS:
        for content in dc.CONTENTS:
            if content == "fib" and rows != 4180:
                continue
            for cols in (1, 3, cg - 1, cg, cg + 1, 2 * cg + 1, 33):
                if rows == 65537 and cols not in (1, 3, cg + 1):
                    continue
                mats.append(np.stack([dc.column(content, rows, seed=j) for j in range(cols)], axis=1))
    all_head = len(mats)
    mats.append(np.array([[5, -3, 5]], dtype=np.int8))  # 3 bytes at 1 mod 16: all head
    past16 = len(mats)
    mats.append(np.stack([dc.column("geo", 11, seed=j) for j in range(3)], axis=1))  # 33 bytes from a 16-byte boundary: one past two vectors
    n = len(mats)
    src_off, at = np.zeros(n, dtype=np.int64), 1
    for i in rng.permutation(n):
        if i == all_head:
            at = (at + 15) // 16 * 16 + 1
        elif i == past16:
            at = (at + 15) // 16 * 16
        else:
            at |= 1
        src_off[i] = at
        at += mats[i].size
    src = np.full(at + 5, 99, dtype=np.int8)
    for m, o in zip(mats, src_off):
        src[o:o + m.size] = m.reshape(-1)
    len_off, at = np.zeros(n, dtype=np.int64), 2
    for i in rng.permutation(n):
        len_off[i] = at
        at += mats[i].shape[1] + int(rng.integers(0, 3))
    expected = np.full(at + 4, SENTINEL, dtype=np.int32)
    for m, o in zip(mats, len_off):
        expected[o:o + m.shape[1]] = [len(dc.host_stream(np.ascontiguousarray(m[:, j]))) for j in range(m.shape[1])]
    table = np.zeros((n, 5), dtype=np.int64)
    table[:, 0] = src_off
    table[:, 1] = [m.shape[0] for m in mats]
    table[:, 2] = [m.shape[1] for m in mats]
    slots = table[:, 2] * _lib.deflate_bound(table[:, 1])
    table[:, 3] = np.cumsum(slots) - slots
    table[:, 4] = len_off
    assert src_off[all_head] % 16 == 1 and src_off[past16] % 16 == 0 and (np.delete(src_off, past16) % 2 == 1).all()
    assert not (np.diff(src_off) > 0).all() and not (np.diff(len_off) > 0).all()
    return src, table, int(slots.sum()), expected


def test_counts_equal_the_restatement_and_the_coder(mixed):
    from lrf_amd import _lib
    src, table, nbytes, expected = mixed
    ctx = _lib.context()
    src_d = torch.from_numpy(src).cuda()  # (torch's allocations start at a multiple of 16 bytes and more)
    assert src_d.data_ptr() % 16 == 0
    lens = torch.full((expected.size,), SENTINEL, dtype=torch.int32, device="cuda")
    ctx.deflate_sizes_into(src_d, table, lens)
    got = ctx.to_host(lens)[0].numpy()
    bad = np.flatnonzero(got != expected)
    assert bad.size == 0, f"{bad.size} entries differ, first at {bad[0]}: counted {got[bad[0]]}, the stream has {expected[bad[0]]}"
    assert int(expected.max()) > 65535 + 11 and (expected == SENTINEL).any()
    # the coder itself on the same table: the same array, entry by entry (sentinels included)
    slots = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    written = torch.full((expected.size,), SENTINEL, dtype=torch.int32, device="cuda")
    ctx.deflate_columns_into(src_d, table, slots, written)
    assert np.array_equal(ctx.to_host(written)[0].numpy(), got)
    assert np.array_equal(src_d.cpu().numpy(), src), "the source was written"
    # and the convenience form: deflate_table's layout
    three = [(int(r[0]), int(r[1]), int(r[2])) for r in table[:40]]
    a = ctx.deflate_sizes(src_d, three)
    b = ctx.deflate_columns(src_d, three)[1]
    assert a.dtype == torch.int32 and torch.equal(a, b)


def test_the_corpus_has_the_edges(mixed):
    """zero at 65,537 rows: a count above 16 bits; full at 65,537 rows: two stored blocks"""
    zero, full = dc.host_stream(dc.column("zero", 65537)), dc.host_stream(dc.column("full", 65537))
    assert (zero[2] >> 1) & 3 != 0 and len(zero) < 65537 // 7
    assert full[2] == 0 and full[2 + 5 + 65535] == 1 and len(full) == dc.bound(65537)
    from lrf_amd import _lib
    cg = _lib.LRF_DEFLATE_CG
    _, table, _, expected = mixed
    assert dc.bound(65537) in expected.tolist() and {1, 3, cg - 1, cg, cg + 1, 2 * cg + 1, 33} <= set(table[:, 2].tolist())


def test_argument_checks_launch_nothing():
    from lrf_amd import _lib
    ctx = _lib.context()
    src = torch.zeros((64 * 3,), dtype=torch.int8, device="cuda")
    lens = torch.full((6,), SENTINEL, dtype=torch.int32, device="cuda")
    good = np.array([[0, 64, 3, 0, 0]], dtype=np.int64)
    for table, ln in ((np.array([[0, 0, 3, 0, 0]], dtype=np.int64), lens),            # rows < 1
                      (np.array([[0, (1 << 30) + 1, 1, 0, 0]], dtype=np.int64), lens),  # rows > 2^30
                      (np.array([[0, 64, 0, 0, 0]], dtype=np.int64), lens),            # cols < 1
                      (np.array([[0, 1, 4097, 0, 0]], dtype=np.int64), lens),          # cols > 4096
                      (np.zeros((0, 5), dtype=np.int64), lens),                        # n < 1
                      (np.array([[-1, 64, 3, 0, 0]], dtype=np.int64), lens),           # a negative source offset
                      (np.array([[0, 64, 3, 0, -1]], dtype=np.int64), lens),           # a negative length offset
                      (np.array([[1, 64, 3, 0, 0]], dtype=np.int64), lens),            # the matrix leaves src
                      (np.array([[0, 64, 3, 0, 4]], dtype=np.int64), lens),            # its lengths leave out_len
                      (good, lens[:2]),                                                # out_len_count below cols
                      (np.array([[0, 32, 3, 0, 0], [96, 32, 3, 0, 2]], dtype=np.int64), lens)):  # overlapping length entries
        with pytest.raises(ValueError):
            ctx.deflate_sizes_into(src, table, ln)
    torch.cuda.synchronize()
    assert bool((lens == SENTINEL).all())
    # dst_off is ignored: a negative one and two equal ones are no refusal
    ok = np.array([[0, 32, 3, -5, 3], [96, 32, 3, -5, 0]], dtype=np.int64)
    ctx.deflate_sizes_into(src, ok, lens)
    assert ctx.to_host(lens)[0].tolist() == [len(dc.host_stream(np.zeros(32, dtype=np.int8)))] * 6
    lens.fill_(SENTINEL)
    ctx.deflate_sizes_into(src, good, lens)  # the good table does run
    assert ctx.to_host(lens)[0].tolist() == [len(dc.host_stream(np.zeros(64, dtype=np.int8)))] * 3 + [SENTINEL] * 3


TRIPLES = [(1, 1, 1), (7, 3, 3), (9, 4, 4), (20, 10, 10), (38, 19, 19)]


@pytest.mark.parametrize("hw", [(48, 64), (37, 53)], ids=["48x64", "37x53"])
def test_stream_sizes_equal_the_streams(hw):
    import lrf_amd
    from lrf_amd import _lib
    H, W = hw
    images = torch.stack([make_image(dict(kind="smooth" if i % 2 else "randint", seed=900 + i, H=H, W=W)) for i in range(6)]).contiguous()
    dev = images.cuda()
    want = torch.tensor([[len(s) for s in lrf_amd.qmf_encode_batch(dev, rank=list(t), deflate="device")] for t in TRIPLES], dtype=torch.int64)
    pairs = [lrf_amd.qmf_factorize_batch(dev, list(t)) for t in TRIPLES]
    got = lrf_amd.qmf_stream_sizes(pairs, TRIPLES, hw)  # (separate tensors: concatenated)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (len(TRIPLES), 6)
    assert torch.equal(got.cpu(), want), (got.cpu() - want).tolist()
    assert torch.equal(lrf_amd.qmf_stream_sizes(pairs[1], TRIPLES[1], hw).cpu(), want[1:2])  # one triple: the pair itself
    fused = [t for t in TRIPLES if max(t) <= 32]
    swept = _lib.context().encode_sweep_rgb(dev, fused, 10, -16, 15)  # consecutive views of two flat buffers: counted where they lie
    assert torch.equal(lrf_amd.qmf_stream_sizes(swept, fused, hw).cpu(), want[:len(fused)])
