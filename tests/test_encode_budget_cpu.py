"""CPU suite: the host side of qmf_encode_budget — container_bytes against the containers liblrf_pack.so folds, select_budget
against the rule written as a plain loop, and every refusal of the entry point with no GPU present."""
import ctypes

import numpy as np
import pytest
import torch

import deflate_cases as dc


def fold(fac, meta):
    """lrf_pack_qmf_streams_deflated over host-made slots of one image's six factors -> (the container, its column lengths)"""
    from lrf_amd.codec import _pack_lib
    lib = _pack_lib()
    chunks, col_off, col_len, at = [], [], [], 0
    for f in fac:
        for j in range(f.shape[1]):
            s = dc.host_stream(np.ascontiguousarray(f[:, j]))
            slot = dc.bound(f.shape[0])
            chunks.append(s + b"\xA5" * (slot - len(s)))
            col_off.append(at)
            col_len.append(len(s))
            at += slot
    slots = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    col_off, col_len = np.array(col_off, dtype=np.int64), np.array(col_len, dtype=np.int32)
    M = np.array([fac[0].shape[0], fac[2].shape[0], fac[4].shape[0]], dtype=np.int64)
    R = np.array([fac[0].shape[1], fac[2].shape[1], fac[4].shape[1]], dtype=np.int32)
    out, out_len = (ctypes.c_void_p * 1)(), (ctypes.c_int64 * 1)()
    rc = lib.lrf_pack_qmf_streams_deflated(slots.ctypes.data, slots.size, 1, M.ctypes.data, R.ctypes.data, col_off.ctypes.data, col_len.ctypes.data,
                                           col_off.size, (ctypes.c_char_p * 1)(meta), np.array([len(meta)], dtype=np.int64).ctypes.data, 1, out, out_len)
    assert rc == 0
    stream = ctypes.string_at(out[0], out_len[0])
    lib.lrf_pack_free(out[0])
    return stream, col_len


def test_container_bytes_equals_the_folded_containers():
    from lrf_amd import container_bytes
    from lrf_amd.codec import _stream_metadata, parse_stream
    from lrf_amd.container import bytes_to_dict, separate_bytes
    seen, ranks_seen = 0, set()
    for name, fac in dc.golden_factor_sets():
        z = np.load(f"{dc.HERE}/golden/{name}.npz")
        meta = bytes_to_dict(separate_bytes(z["encoded"].tobytes(), 2)[0])
        if not all(f.shape[0] == 64 for f in fac[1::2]) or not meta.get("patch") or meta.get("color space") != "YCbCr":
            continue  # (the 8x8-patch default branch: planes of 64 columns)
        H, W = meta["original size"][0]
        ranks = [f.shape[1] for f in fac[0::2]]
        mb = _stream_metadata((H, W), ranks, tuple(meta["bounds"]))
        stream, col_len = fold(fac, mb)
        assert int(container_bytes(len(mb), ranks, col_len)) == len(stream), name
        assert int(container_bytes(len(mb), ranks, torch.from_numpy(col_len))) == len(stream), name
        got_meta, got_fac = parse_stream(stream)  # and it is a container every reader takes
        assert got_meta == bytes_to_dict(mb) and all(np.array_equal(a, b) for a, b in zip(got_fac, fac))
        seen += 1
        ranks_seen.add(tuple(ranks))
    assert seen >= 10 and len(ranks_seen) >= 4, (seen, ranks_seen)
    assert any(max(r) >= 10 for r in ranks_seen), "a two-digit num_fibers changes the header's length"


def test_container_bytes_is_vectorised_and_refuses_a_wrong_column_count():
    from lrf_amd import container_bytes
    lens = np.arange(3 * 26, dtype=np.int64).reshape(3, 26) + 11
    one = [int(container_bytes(120, (7, 3, 3), row)) for row in lens]
    assert container_bytes(120, (7, 3, 3), lens).tolist() == one
    assert container_bytes(120, (7, 3, 3), torch.from_numpy(lens).to(torch.int32)).tolist() == one
    assert one[1] - one[0] == 26 * 26 and int(container_bytes(121, (7, 3, 3), lens[0])) == one[0] + 1
    with pytest.raises(ValueError):
        container_bytes(120, (7, 3, 3), lens[:, :25])
    with pytest.raises(ValueError):
        container_bytes(120, (7, 3), lens)


def rule(size, sse, budget):
    """the issue's rule, candidate by candidate"""
    index, reached = [], []
    for b in range(len(budget)):
        fit = [q for q in range(len(size)) if size[q][b] <= budget[b]]
        if fit:
            index.append(min(fit, key=lambda q: (sse[q][b], size[q][b], q)))
        else:
            index.append(min(range(len(size)), key=lambda q: (size[q][b], q)))
        reached.append(bool(fit))
    return index, reached


BUDGET_TABLES = {
    # size [Q][B], sse [Q][B], budget [B], what the rule must give
    "not monotonic": ([[500, 900], [400, 300], [700, 800], [650, 1000]], [[90, 40], [95, 70], [30, 60], [50, 10]], [660, 850], ([3, 2], [True, True])),
    "tie on sse, sizes differ": ([[300], [200], [250]], [[7], [7], [7]], [1000], ([1], [True])),
    "full tie": ([[300], [200], [200], [400]], [[9], [5], [5], [5]], [1000], ([1], [True])),
    "nothing fits": ([[300, 50], [200, 50], [200, 60]], [[1, 3], [2, 2], [3, 1]], [199, 49], ([1, 0], [False, False])),
    "everything fits": ([[300, 100], [200, 200], [250, 300]], [[5, 9], [9, 8], [1, 8]], [10 ** 12, 10 ** 12], ([2, 1], [True, True])),
    "per-image budgets": ([[100, 100, 100], [200, 200, 200], [300, 300, 300]], [[30, 30, 30], [20, 20, 20], [10, 10, 10]], [150, 250, 99],
                          ([0, 1, 0], [True, True, False])),
    "a budget equal to a size fits": ([[100], [200], [300]], [[30], [20], [10]], [200], ([1], [True])),
    "zero budget": ([[100, 80], [90, 80]], [[1, 1], [2, 2]], [0, 0], ([1, 0], [False, False])),
}


@pytest.mark.parametrize("name", list(BUDGET_TABLES))
def test_select_budget(name):
    from lrf_amd import select_budget
    size, sse, budget, want = BUDGET_TABLES[name]
    assert rule(size, sse, budget) == want, "the table is not the case its name says"
    index, reached = select_budget(torch.tensor(size, dtype=torch.int64), torch.tensor(sse, dtype=torch.int64), torch.tensor(budget, dtype=torch.int64))
    assert index.dtype == torch.int64 and reached.dtype == torch.bool
    assert (index.tolist(), reached.tolist()) == want


def test_select_budget_random_tables_with_many_ties():
    from lrf_amd import select_budget
    rng = np.random.default_rng(8)
    for _ in range(40):
        Q, B = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        size, sse = rng.integers(1, 6, (Q, B)), rng.integers(0, 4, (Q, B))
        budget = rng.integers(0, 7, B)
        index, reached = select_budget(torch.from_numpy(size), torch.from_numpy(sse), torch.from_numpy(budget))
        assert (index.tolist(), reached.tolist()) == rule(size.tolist(), sse.tolist(), budget.tolist())


@pytest.fixture
def no_gpu(monkeypatch):
    """any request for a context fails the test: a refusal must come first"""
    from lrf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a GPU context was asked for before the refusal")
    monkeypatch.setattr(_lib, "context", boom)


IMG = torch.zeros((2, 3, 16, 24), dtype=torch.uint8)
REFUSALS = [
    ("both", dict(bpp=1.0, nbytes=100), ValueError),
    ("neither", dict(), ValueError),
    ("wrong count", dict(nbytes=[100, 200, 300]), ValueError),
    ("wrong count bpp", dict(bpp=torch.tensor([1.0, 2.0, 3.0])), ValueError),
    ("nan", dict(bpp=float("nan")), ValueError),
    ("nan among nbytes", dict(nbytes=[100.0, float("nan")]), ValueError),
    ("negative", dict(nbytes=-1), ValueError),
    ("negative bpp", dict(bpp=[0.5, -0.5]), ValueError),
    ("float images", dict(nbytes=100, images=IMG.float()), NotImplementedError),
    ("3-D", dict(nbytes=100, images=IMG[0]), ValueError),
    ("not a tensor", dict(nbytes=100, images=IMG.numpy()), TypeError),
    ("num_iters 0", dict(nbytes=100, num_iters=0), NotImplementedError),
    ("no qualities", dict(nbytes=100, qualities=[]), ValueError),
    ("quality out of range", dict(nbytes=100, qualities=[5, 101]), ValueError),
]


@pytest.mark.parametrize("name,kw,error", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_need_no_gpu(no_gpu, name, kw, error):
    import lrf_amd
    kw = dict(kw)
    images = kw.pop("images", IMG)
    with pytest.raises(error):
        lrf_amd.qmf_encode_budget(images, **kw)


def test_bpp_becomes_bytes_once():
    from lrf_amd.codec import _check_budget_args
    img = torch.zeros((3, 3, 37, 53), dtype=torch.uint8)
    _, b = _check_budget_args(img, 0.75, None, range(1, 33), 10)
    assert b.dtype == torch.int64 and b.tolist() == [int(np.floor(np.float64(0.75) * 37 * 53 / 8))] * 3
    _, b = _check_budget_args(img, None, torch.tensor([5, 0, 70000]), [7], 10)
    assert b.tolist() == [5, 0, 70000]
    _, b = _check_budget_args(img, [0.0, 1.0, float("inf")], None, [7], 10)
    assert b.tolist()[:2] == [0, 37 * 53 // 8] and b[2] >= 2 ** 62


def test_public_names():
    import lrf_amd
    for name in ("qmf_encode_budget", "qmf_stream_sizes", "select_budget", "container_bytes"):
        assert name in lrf_amd.__all__ and callable(getattr(lrf_amd, name))
