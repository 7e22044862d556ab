"""GPU suite: lrf_inflate_columns_i8 gives the host restatement's bytes and statuses, stream by stream (the restatement itself is
held against zlib.decompress by tests/test_inflate_host.py)."""
import zlib

import numpy as np
import pytest
import torch

import inflate_cases as ic

pytestmark = pytest.mark.gpu
MARK, GUARD, GAP = -77, 4096, 5
COLS = (1, 3, 7, 64, 65, 130)


def layout(groups):
    """groups: [(rows, [stream per column])] -> (src bytes, table [n, 4], col_off, col_len, bytes of dst without the guard): the
    matrices GAP marker bytes apart in dst, the streams back to back in src"""
    table, col_off, col_len, parts, at, dst_at, first = [], [], [], [], 0, GAP, 0
    for rows, streams in groups:
        table.append((dst_at, rows, len(streams), first))
        dst_at += rows * len(streams) + GAP
        first += len(streams)
        for z in streams:
            parts.append(z)
            col_off.append(at)
            col_len.append(len(z))
            at += len(z)
    return (np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(table, dtype=np.int64), np.array(col_off, dtype=np.int64),
            np.array(col_len, dtype=np.int32), dst_at)


def run(ctx, src, table, col_off, col_len, nbytes, dst=None, status=None):
    src_d = torch.from_numpy(src).cuda()
    dst = torch.full((nbytes + GUARD,), MARK, dtype=torch.int8, device="cuda") if dst is None else dst
    status = torch.full((col_off.size,), -1, dtype=torch.int32, device="cuda") if status is None else status
    ctx.inflate_columns_into(src_d, table, col_off, col_len, dst, status)
    d, s = ctx.to_host(dst, status)
    return d.numpy(), s.numpy()


@pytest.fixture(scope="module")
def good_call():
    """the whole corpus and the hand-built streams as matrices of 1, 3, 7, 64, 65 and 130 columns: streams of equal rows share
    matrices, so rows mix within the call and waves straddle matrices -> (layout, expected dst without the guard)"""
    by_rows = {}
    for _, z, data in ic.corpus() + ic.hand_built():
        by_rows.setdefault(len(data), []).append((z, data))
    groups, cols, k = [], [], 0
    for rows in sorted(by_rows):  # (ascending here: the plan, not the call, puts the long columns first)
        items = by_rows[rows]
        while items:
            take, items = items[:COLS[k % len(COLS)]], items[COLS[k % len(COLS)]:]
            k += 1
            groups.append((rows, [z for z, _ in take]))
            cols.append([d for _, d in take])
    lay = layout(groups)
    want = np.full(lay[4], MARK, dtype=np.int8)
    for (dst_off, rows, ncol, _), datas in zip(lay[1], cols):
        m = np.stack([np.frombuffer(d, dtype=np.int8) for d in datas], axis=1)
        want[dst_off:dst_off + rows * ncol] = m.reshape(-1)
    assert {len(c) for c in cols} >= set(COLS)
    return lay, want


def test_status_and_bytes_of_every_stream(good_call):
    from lrf_amd import _lib
    (src, table, col_off, col_len, nbytes), want = good_call
    ctx = _lib.context()
    for _ in range(2):  # twice: the second call reuses the context's tables
        dst, status = run(ctx, src, table, col_off, col_len, nbytes)
        assert not status.any(), (np.flatnonzero(status)[:8], status[np.flatnonzero(status)[:8]])
        bad = np.flatnonzero(dst[:nbytes] != want)
        assert bad.size == 0, f"first differing byte {bad[0]} of {bad.size}"
        assert (dst[nbytes:] == MARK).all()


def test_corrupt_streams_between_good_ones(good_call):
    from lrf_amd import _lib
    by_rows = {}
    for name, z, rows in ic.corrupt():
        if len(z) >= 8:  # (shorter ones are refused by the argument check: test_argument_checks_launch_nothing)
            by_rows.setdefault(rows, []).append(z)
    groups, expect = [], []
    rng = np.random.default_rng(8)
    for rows in sorted(by_rows):
        streams = []
        for z in by_rows[rows]:  # lane by lane: a corrupt stream, a good one
            g = rng.integers(-16, 16, rows).astype(np.int8)
            streams += [z, zlib.compress(g.tobytes(), 9)]
        groups.append((rows, streams))
        expect.append([ic.host_inflate(z, rows) for z in streams])
    assert sum(rc != 0 for e in expect for rc, _ in e) >= 60
    src, table, col_off, col_len, nbytes = layout(groups)
    ctx = _lib.context()
    dst, status = run(ctx, src, table, col_off, col_len, nbytes)
    assert status.tolist() == [rc for e in expect for rc, _ in e]
    want = np.full(nbytes + GUARD, MARK, dtype=np.int8)
    own = np.zeros(nbytes + GUARD, dtype=bool)  # the elements of the refused columns: the only bytes whose content is unspecified
    for (dst_off, rows, ncol, _), e in zip(table, expect):
        for j, (rc, col) in enumerate(e):
            if rc == 0:
                want[dst_off + j:dst_off + rows * ncol:ncol] = col
            else:
                own[dst_off + j:dst_off + rows * ncol:ncol] = True
    bad = np.flatnonzero((dst != want) & ~own)
    assert bad.size == 0, f"first wrong byte {bad[0]} of {bad.size}"
    (src, table, col_off, col_len, nbytes), want = good_call  # and a good call behind it is right
    dst, status = run(ctx, src, table, col_off, col_len, nbytes)
    assert not status.any() and np.array_equal(dst[:nbytes], want) and (dst[nbytes:] == MARK).all()


def test_argument_checks_launch_nothing():
    from lrf_amd import _lib
    ctx = _lib.context()
    cols = [np.random.default_rng(j).integers(-16, 16, 64).astype(np.int8) for j in range(4)]
    streams = [zlib.compress(c.tobytes(), 9) for c in cols]
    src, table, col_off, col_len, nbytes = layout([(64, streams[:3]), (64, streams[3:])])
    src_d = torch.from_numpy(src).cuda()
    dst = torch.full((nbytes + GUARD,), MARK, dtype=torch.int8, device="cuda")
    status = torch.full((4,), -1, dtype=torch.int32, device="cuda")

    def changed(**kw):
        t, o, l = table.copy(), col_off.copy(), col_len.copy()
        for key, v in kw.items():
            {"t": t, "o": o, "l": l}[key[0]][int(key[1:]) if key[0] != "t" else (int(key[1]), int(key[2]))] = v
        return t, o, l

    bad = [changed(o3=src.size - int(col_len[3]) + 1),         # a stream past src_len
           changed(l2=7),                                       # col_len 7
           changed(t10=int(table[0, 0]) + 64 * 3 - 1),          # overlapping matrices
           changed(t13=2),                                      # overlapping stream indices
           changed(t01=0),                                      # rows 0
           changed(t02=4097),                                   # cols 4097
           (table[:0], col_off, col_len),                       # n 0
           (table, col_off, col_len, dst[:int(table[1, 0]) + 63])]  # a matrix past dst_len
    for args in bad:
        with pytest.raises(ValueError):
            ctx.inflate_columns_into(src_d, args[0], args[1], args[2], args[3] if len(args) > 3 else dst, status)
    with pytest.raises(ValueError):  # ncols is not the sum of cols
        ctx.inflate_columns_into(src_d, table, np.append(col_off, 0), np.append(col_len, 8), dst, torch.full((5,), -1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert bool((dst == MARK).all()) and bool((status == -1).all())
    ctx.inflate_columns_into(src_d, table, col_off, col_len, dst, status)  # the good call does run
    d, s = ctx.to_host(dst, status)
    assert s.tolist() == [0, 0, 0, 0]
    assert np.array_equal(d[GAP:GAP + 192].numpy().reshape(64, 3), np.stack(cols[:3], axis=1))
    assert np.array_equal(d[int(table[1, 0]):int(table[1, 0]) + 64].numpy(), cols[3]) and bool((d[nbytes:] == MARK).all())
