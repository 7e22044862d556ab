"""GPU suite (-m gpu): the calls on a caller's stream.  Every wrapper binds the context to torch's current stream, so "the call is
ordered on your stream" is the contract; here the current stream is a side stream with work queued ahead of the call.

The construction (`on_stream`): the call's input buffers hold a DECOY (other images, other factors); on the stream S a chain of
large matmuls is queued (at least 20 ms, measured with events and asserted), behind it the copy of the real input into the
buffers, then the call, then a clone of the call's output and the copy of the decoy back into the inputs.  No host
synchronisation of the test's own until the end.  A call that ran ahead of its stream reads the decoy; one that left work running
on another stream after it returned reads the decoy put back, or its output is cloned before it is written.  Expected values are
computed first, the ordinary way on the default stream.  The control test shows the construction has teeth: the same sequence
with the context on its own stream (lrf_ctx_use_own_stream) decodes the decoy.

Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import deflate_cases as dc

pytestmark = pytest.mark.gpu
MIN_BUSY_MS = 20.0


def _crop_slots():
    """LRF_CROP_SLOTS, read from the header: the pinned staging slots of a table that travels stream-ordered"""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "lrf_amd", "csrc", "lrf_host.h")).read()
    return int(re.search(r"^#define\s+LRF_CROP_SLOTS\s+(\d+)", text, re.M).group(1))


SLOTS = _crop_slots()
SIZES = [(96, 160), (61, 117)]
TRIPLES = [(7, 3, 3), (16, 8, 8)]


class Busy:
    """a chain of 4096^3 matmuls, its length sized once so that it takes about 60 ms"""

    def __init__(self):
        g = torch.Generator(device="cuda").manual_seed(1)
        self.a = torch.randn((4096, 4096), device="cuda", generator=g) / 128.0  # (spectral norm about 1: the chain stays finite)
        self.b = torch.randn((4096, 4096), device="cuda", generator=g)
        self.c = torch.empty_like(self.b)
        self._timed(4)  # (the BLAS library's first call)
        per = min(self._timed(32) for _ in range(3)) / 32  # the fastest link seen sizes the chain: three times the minimum
        self.n = int(3 * MIN_BUSY_MS / per) + 1
        self.measured = []

    def _timed(self, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.queue(n)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def queue(self, n=None):
        x, y = self.b, self.c
        for _ in range(n or self.n):
            torch.mm(self.a, x, out=y)
            x, y = y, x
        self.b, self.c = x, y


@pytest.fixture(scope="module")
def busy():
    b = Busy()
    yield b
    print(f"\nproducer busy times (ms): min {min(b.measured or [0]):.1f} max {max(b.measured or [0]):.1f} over {len(b.measured)} runs, chain {b.n}")
    del b.a, b.b, b.c
    torch.cuda.empty_cache()


def _flat(out):
    """a call's result as a list of tensors"""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [out[k] for k in sorted(out) if isinstance(out[k], torch.Tensor)]
    return [t for t in out if isinstance(t, torch.Tensor)]


def on_stream(S, busy, inputs, calls):
    """inputs: [(buffer, real, decoy)], the buffers holding the decoy now; calls: functions without arguments, run back to back
    -> per call the clones of its result's tensors, taken on S"""
    for buf, _, decoy in inputs:
        assert torch.equal(buf, decoy)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(S):
        e0.record()
        busy.queue()
        e1.record()
        for buf, real, _ in inputs:
            buf.copy_(real)
        outs = [c() for c in calls]
        snaps = [[t.clone() for t in _flat(o)] for o in outs]
        for buf, _, decoy in inputs:
            buf.copy_(decoy)
    S.synchronize()
    ms = e0.elapsed_time(e1)
    busy.measured.append(ms)
    assert ms >= MIN_BUSY_MS, f"the producer took {ms:.1f} ms: raise the chain length"
    return snaps


def _same(got, want):
    want = _flat(want)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, i
        same_bits = torch.equal(g.view(torch.uint8), w.view(torch.uint8))  # bits, not values: NaN and -0.0 included
        assert same_bits, i


def _images(seed, n, H, W):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(n, 3, max(H // 8, 1), max(W // 8, 1), generator=g) * 255
    sm = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    return (sm + torch.randn(sm.shape, generator=g) * 6).clamp(0, 255).to(torch.uint8).cuda()


def _ctx():
    from lrf_amd import _lib
    return _lib.context(0)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("ranks", TRIPLES)
def test_factorize_then_decode(busy, hw, ranks):
    """qmf_factorize_batch, Context.decode_rgb and image_metrics_batch"""
    import lrf_amd
    ctx = _ctx()
    real, decoy = _images(1, 8, *hw), _images(2, 8, *hw)
    want = lrf_amd.qmf_factorize_batch(real, ranks)
    wrong = lrf_amd.qmf_factorize_batch(decoy, ranks)
    assert not torch.equal(want[0], wrong[0])
    S = torch.cuda.Stream()
    buf = decoy.clone()
    _same(on_stream(S, busy, [(buf, real, decoy)], [lambda: lrf_amd.qmf_factorize_batch(buf, ranks)])[0], want)
    want_rgb = ctx.decode_rgb(want[0], want[1], hw[0], hw[1], list(ranks))
    ub, vb = wrong[0].clone(), wrong[1].clone()
    _same(on_stream(S, busy, [(ub, want[0], wrong[0]), (vb, want[1], wrong[1])], [lambda: ctx.decode_rgb(ub, vb, hw[0], hw[1], list(ranks))])[0], want_rgb)
    want_m = lrf_amd.image_metrics_batch(real, want_rgb)
    rb = decoy.clone()
    got = on_stream(S, busy, [(rb, real, decoy)], [lambda: lrf_amd.image_metrics_batch(rb, want_rgb), lambda: lrf_amd.image_metrics_batch(want_rgb, rb, want_ssim=False)])
    _same(got[0], want_m)
    _same(got[1], lrf_amd.image_metrics_batch(want_rgb, real, want_ssim=False))


class Resident:
    """eight images of the two sizes and the two triples as resident factors (random int8 in [-16, 15]), and a decoy of the same shape"""

    def __init__(self):
        from lrf_amd import _lib
        from lrf_amd.codec import ResidentFactors
        self.ctx = _ctx()
        self.items = [(H, W, r) for k in range(2) for (H, W) in SIZES for r in TRIPLES]
        images, uo, vo = [], 0, 0
        for H, W, r in self.items:
            images.append((H, W, r, uo, vo))
            uo += sum(d[4] * x for d, x in zip(_lib.plane_dims(H, W), r))
            vo += 64 * sum(r)
        g = torch.Generator().manual_seed(3)
        self.real = [torch.randint(-16, 16, (n,), dtype=torch.int8, generator=g).cuda() for n in (uo, vo)]
        self.decoy = [torch.randint(-16, 16, (n,), dtype=torch.int8, generator=g).cuda() for n in (uo, vo)]
        self.U, self.V = self.decoy[0].clone(), self.decoy[1].clone()
        self.rf = ResidentFactors(self.ctx, self.U, self.V, images)
        self.images = images

    def inputs(self):
        return [(self.U, self.real[0], self.decoy[0]), (self.V, self.real[1], self.decoy[1])]

    def expected(self, fn):
        """fn() with the real factors in the buffers, on the default stream; the decoy is put back"""
        self.U.copy_(self.real[0])
        self.V.copy_(self.real[1])
        out = [t.clone() for t in _flat(fn())]
        self.U.copy_(self.decoy[0])
        self.V.copy_(self.decoy[1])
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module")
def resident():
    return Resident()


def _crop_lists(items, n_lists, size, n=12):
    """n_lists different crop lists of one length over the images: (image, y0, x0).  One length, so that a call that read another
    call's table would write wrong bytes, never outside its output."""
    h, w = size
    rng = np.random.default_rng(17)
    out = []
    for k in range(n_lists):
        im = rng.integers(0, len(items), n)
        out.append(np.array([(i, rng.integers(0, items[i][0] - h + 1), rng.integers(0, items[i][1] - w + 1)) for i in im], dtype=np.int64))
    return out


def test_resident_decodes(busy, resident):
    """ResidentFactors.decode (the ragged decode), .decode_crops, .decode(scale=4), .decode_resized_crops"""
    r = resident
    crops = _crop_lists(r.items, 1, (32, 40))[0]
    boxes = np.array([(i, 1, 2, H - 3, W - 5) for i, (H, W, _) in enumerate(r.items)] + [(0, 10, 20, 17, 23), (3, 0, 0, 61, 117)], dtype=np.int64)
    calls = [lambda: r.rf.decode(), lambda: r.rf.decode_crops(crops, (32, 40)), lambda: r.rf.decode(scale=4),
             lambda: r.rf.decode_resized_crops(boxes, (24, 28), flip=[bool(k & 1) for k in range(len(boxes))])]
    want = [r.expected(c) for c in calls]
    wrong = [t.clone() for t in _flat(calls[0]())]
    assert not torch.equal(wrong[0], want[0][0])
    for c, w in zip(calls, want):  # each behind a producer of its own, on a stream of its own (the context comes from another one)
        _same(on_stream(torch.cuda.Stream(), busy, r.inputs(), [c])[0], w)
    for got, w in zip(on_stream(torch.cuda.Stream(), busy, r.inputs(), calls), want):  # and back to back behind one
        _same(got, w)


def test_sse_ragged(busy, resident):
    r = resident
    parts = [_images(20 + i, 1, H, W)[0].reshape(-1) for i, (H, W, _) in enumerate(r.items)]
    offs = np.cumsum([0] + [t.numel() for t in parts])
    real = torch.cat(parts)
    g = torch.Generator().manual_seed(4)
    decoy = torch.randint(0, 256, (real.numel(),), dtype=torch.uint8, generator=g).cuda()
    rgb = decoy.clone()
    items = [(H, W, rk, uo, vo, int(o)) for (H, W, rk, uo, vo), o in zip(r.images, offs)]
    call = lambda: r.ctx.sse_ragged(rgb, items, r.U, r.V)
    rgb.copy_(real)
    want = r.expected(call)
    rgb.copy_(decoy)
    dec = r.expected(lambda: r.rf.decode())
    direct = [int(((d.long().reshape(-1) - real[int(o):int(o) + d.numel()].long()) ** 2).sum()) for d, o in zip(dec, offs)]
    assert want[0].tolist() == direct
    _same(on_stream(torch.cuda.Stream(), busy, r.inputs() + [(rgb, real, decoy)], [call])[0], want)


def test_encode_ragged_of_device_tensors(busy):
    import lrf_amd
    real = [_images(30 + i, 1, H, W)[0] for i, (H, W) in enumerate(SIZES * 4)]
    decoy = [_images(40 + i, 1, H, W)[0] for i, (H, W) in enumerate(SIZES * 4)]
    ranks = [TRIPLES[(i // 2) % 2] for i in range(8)]
    want = lrf_amd.qmf_encode_ragged(real, ranks=ranks)
    assert want != lrf_amd.qmf_encode_ragged(decoy, ranks=ranks)
    bufs = [d.clone() for d in decoy]
    got = []
    on_stream(torch.cuda.Stream(), busy, list(zip(bufs, real, decoy)), [lambda: got.append(lrf_amd.qmf_encode_ragged(bufs, ranks=ranks))])
    assert got[0] == want


def _mat_lists(n_lists):
    """per list: matrices (rows, cols) back to back in one source — the same six matrices in another order, so that every list
    has the same bytes, slots and columns (a call that read another call's table would write wrong bytes, never outside its
    buffers) and another layout"""
    base = [(64, 3), (700, 2), (33, 5), (100, 4), (171, 6), (90, 7)]
    return [base[k % 6:] + base[:k % 6] for k in range(n_lists)]


def test_deflate_and_inflate_table_slots(busy):
    """SLOTS + 2 device deflates back to back behind one producer, each with a table of its own (the slot a call reuses has a
    copy pending), then the same for the inflates of their streams.  A table travels through every slot before, so that no call
    grows a slot or the device table (which waits for the stream)."""
    from lrf_amd import _lib
    ctx = _ctx()
    lists = _mat_lists(SLOTS + 2)
    total = max(sum(r * c for r, c in ms) for ms in lists)
    g = torch.Generator().manual_seed(6)
    real = torch.randint(-16, 16, (total,), dtype=torch.int8, generator=g).cuda()
    decoy = torch.randint(-3, 3, (total,), dtype=torch.int8, generator=g).cuda()
    src = decoy.clone()
    mats = []
    for ms in lists:
        at, m = 0, []
        for r, c in ms:
            m.append((at, r, c))
            at += r * c
        mats.append(m)
    src.copy_(real)
    for _ in range(SLOTS):  # a table through every pinned slot: no later call grows one
        ctx.deflate_columns(src, mats[-1])
    want = [[t.clone() for t in ctx.deflate_columns(src, m)] for m in mats]
    src.copy_(decoy)
    real_h = real.cpu().numpy()
    for m, (slots, lens) in zip(mats, want):  # the expected values against the host restatement
        offs, lens_h, slots_h, k = _lib.deflate_column_offsets(_lib.deflate_table(m)[0]), lens.cpu().numpy(), slots.cpu().numpy(), 0
        for at, r, c in m:
            for j in range(c):
                assert slots_h[offs[k]:offs[k] + lens_h[k]].tobytes() == dc.host_stream(np.ascontiguousarray(real_h[at:at + r * c].reshape(r, c)[:, j]))
                k += 1
    S = torch.cuda.Stream()
    got = on_stream(S, busy, [(src, real, decoy)], [lambda m=m: ctx.deflate_columns(src, m) for m in mats])
    for m, g_, w in zip(mats, got, want):
        assert torch.equal(g_[1], w[1])  # the lengths; the slots up to each stream's length (the rest of a slot is not written)
        lens_h = w[1].cpu().numpy()
        keep = torch.zeros_like(w[0], dtype=torch.bool)
        for o, n in zip(_lib.deflate_column_offsets(_lib.deflate_table(m)[0]), lens_h):
            keep[int(o):int(o) + int(n)] = True
        assert torch.equal(g_[0][keep], w[0][keep])
    # inflate: per list the streams of `want`, the decoy streams those of the decoy source
    src.copy_(decoy)
    wrong = [[t.clone() for t in ctx.deflate_columns(src, m)] for m in mats]
    torch.cuda.synchronize()
    inputs, calls, wants = [], [], []
    for m, (slots, lens), (dslots, dlens) in zip(mats, want, wrong):
        tab, nbytes, ncols = _lib.inflate_table([(r, c) for _, r, c in m])
        offs = _lib.deflate_column_offsets(_lib.deflate_table(m)[0])
        sbuf = dslots.clone()
        # the stream LENGTHS are host arguments: the real ones; the decoy bytes under them are other streams (a non-zero status)
        lens_h = lens.cpu().numpy()

        def call(sbuf=sbuf, tab=tab, offs=offs, lens_h=lens_h, nbytes=nbytes, ncols=ncols):
            dst = torch.full((nbytes,), 99, dtype=torch.int8, device="cuda")
            status = torch.full((ncols,), -1, dtype=torch.int32, device="cuda")
            ctx.inflate_columns_into(sbuf, tab, offs, lens_h, dst, status)
            return dst, status
        sbuf.copy_(slots)
        if not wants:
            for _ in range(SLOTS):  # a table through every pinned slot
                call()
        w = [t.clone() for t in call()]
        sbuf.copy_(dslots)
        assert w[1].tolist() == [0] * ncols and torch.equal(w[0], real[:nbytes])
        inputs.append((sbuf, slots, dslots))
        calls.append(call)
        wants.append(w)
    torch.cuda.synchronize()
    for g_, w in zip(on_stream(S, busy, inputs, calls), wants):
        _same(g_, w)


def test_crop_table_slots(busy, resident):
    """SLOTS + 2 decode_crops calls back to back behind one producer, each with a crop list and an expected output of its own"""
    r = resident
    lists = _crop_lists(r.items, SLOTS + 2, (24, 24))
    calls = [lambda c=c: r.rf.decode_crops(c, (24, 24)) for c in lists]
    for _ in range(SLOTS):  # a list through every pinned slot first: no later call grows a slot or the device table
        r.expected(calls[-1])
    want = [r.expected(c) for c in calls]
    assert all(not torch.equal(a[0], b[0]) for i, a in enumerate(want) for b in want[:i])
    for got, w in zip(on_stream(torch.cuda.Stream(), busy, r.inputs(), calls), want):
        _same(got, w)


def test_stream_changes_and_family_streams(busy):
    """Two streams in turn and then the default stream, the second call larger than the first (the encoder's workspace and its
    tables grow between calls on different streams; the crop, deflate and inflate tables: test_tables_grow_between_streams).
    Both calls fork the family streams: plan_bcd splits a call of
    ranks above 16 into a run per rank family from 256 blocks on and gives streams = CALL — 88 images of 96x160 at (20, 10, 10) are
    264 blocks in two runs (88 + 176), 12 images of 512x768 are 288 (192 + 96); 85 images of 96x160 (255 blocks) would be one run
    and no fork.  (tests/test_bcd_plan.py's shim: plan(lib, image_planes(88, 96, 160, (20, 10, 10))) has head["streams"] == 2 and
    two runs.)"""
    import lrf_amd
    ranks = (20, 10, 10)
    small, large = _images(50, 88, 96, 160), _images(51, 12, 512, 768)
    dsmall, dlarge = _images(52, 88, 96, 160), _images(53, 12, 512, 768)
    want_s = lrf_amd.qmf_factorize_batch(small, ranks)
    want_l = lrf_amd.qmf_factorize_batch(large, ranks)
    ctx = _ctx()
    ctx.trim()  # the workspace grows again below, first on S1, then on S2
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    bs, bl = dsmall.clone(), dlarge.clone()
    for _ in range(2):
        _same(on_stream(S1, busy, [(bs, small, dsmall)], [lambda: lrf_amd.qmf_factorize_batch(bs, ranks)])[0], want_s)
        _same(on_stream(S2, busy, [(bl, large, dlarge)], [lambda: lrf_amd.qmf_factorize_batch(bl, ranks)])[0], want_l)
    bl.copy_(large)
    _same(_flat(lrf_amd.qmf_factorize_batch(bl, ranks)), want_l)  # the default stream again
    # without a host synchronisation of the test's between the streams: S2's call is made while S1's work may still run
    bs.copy_(dsmall)
    bl.copy_(dlarge)
    torch.cuda.synchronize()
    with torch.cuda.stream(S1):
        busy.queue()
        bs.copy_(small)
        o1 = [t.clone() for t in lrf_amd.qmf_factorize_batch(bs, ranks)]
        bs.copy_(dsmall)
    with torch.cuda.stream(S2):
        busy.queue(4)
        bl.copy_(large)
        o2 = [t.clone() for t in lrf_amd.qmf_factorize_batch(bl, ranks)]
        bl.copy_(dlarge)
    torch.cuda.synchronize()
    _same(o1, want_s)
    _same(o2, want_l)


def test_tables_grow_between_streams(busy, resident):
    """A context of the test's own, so that every table and pinned slot starts empty: decode_crops, the device deflate and the
    inflate are called on S1, then on S2, then on S1 again and at last on the default stream, every time with a list several
    times the last one's — the crop, deflate and inflate device tables are freed and made anew, and the pinned slots grow, while
    the other stream's call that used the old ones was queued behind a producer and nothing of the test's waits in between.
    S1's and S2's calls read factor and source buffers of their own (decoy, real behind the producer, decoy again).  Every
    result equals the shared context's on the default stream."""
    from lrf_amd import _lib
    from lrf_amd.codec import ResidentFactors
    r = resident
    shared = r.ctx
    good = ResidentFactors(shared, r.real[0], r.real[1], r.images)
    rng = np.random.default_rng(23)
    size = (16, 24)
    crops = []
    for n in (5, 60, 700, 5000):
        im = rng.integers(0, len(r.items), n)
        crops.append(np.array([(i, rng.integers(0, r.items[i][0] - size[0] + 1), rng.integers(0, r.items[i][1] - size[1] + 1)) for i in im], dtype=np.int64))
    shapes = [[(64, 3), (33, 5)], [(50 + k, 2 + k % 5) for k in range(24)], [(40 + k % 37, 1 + k % 7) for k in range(300)],
              [(30 + k % 41, 1 + k % 3) for k in range(2000)]]
    mats = []
    for sh in shapes:
        at, m = 0, []
        for rows, cols in sh:
            m.append((at, rows, cols))
            at += rows * cols
        mats.append(m)
    total = max(m[-1][0] + m[-1][1] * m[-1][2] for m in mats)
    g = torch.Generator().manual_seed(9)
    src_real = torch.randint(-16, 16, (total,), dtype=torch.int8, generator=g).cuda()
    src_decoy = torch.randint(-3, 3, (total,), dtype=torch.int8, generator=g).cuda()
    want_crops = [good.decode_crops(c, size) for c in crops]
    want_defl = [shared.deflate_columns(src_real, m) for m in mats]
    torch.cuda.synchronize()

    def inflate(ctx, k):
        """the matrices of list k back from the expected streams"""
        tab, nbytes, ncols = _lib.inflate_table([(rows, cols) for _, rows, cols in mats[k]])
        offs = _lib.deflate_column_offsets(_lib.deflate_table(mats[k])[0])
        dst = torch.full((nbytes,), 99, dtype=torch.int8, device="cuda")
        status = torch.full((ncols,), -1, dtype=torch.int32, device="cuda")
        ctx.inflate_columns_into(want_defl[k][0], tab, offs, lens_h[k], dst, status)
        return dst, status
    lens_h = [w[1].cpu().numpy() for w in want_defl]
    ctx = _lib.Context(0)
    try:
        bufs = []
        for _ in range(2):  # S1's and S2's inputs
            U, V, src = r.decoy[0].clone(), r.decoy[1].clone(), src_decoy.clone()
            bufs.append((ResidentFactors(ctx, U, V, r.images), U, V, src))
        S = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        got = []
        for k, which in enumerate((0, 1, 0)):
            rf, U, V, src = bufs[which]
            with torch.cuda.stream(S[which]):
                if k < 2:  # (S1's third visit finds its inputs real: the decoy goes back behind it)
                    busy.queue(None if k == 0 else busy.n // 4)
                    U.copy_(r.real[0])
                    V.copy_(r.real[1])
                    src.copy_(src_real)
                out = [rf.decode_crops(crops[k], size), *ctx.deflate_columns(src, mats[k]), *inflate(ctx, k)]
                got.append([t.clone() for t in out])
        for which in (0, 1):
            with torch.cuda.stream(S[which]):
                bufs[which][1].copy_(r.decoy[0])
                bufs[which][2].copy_(r.decoy[1])
                bufs[which][3].copy_(src_decoy)
        torch.cuda.synchronize()
        rf = ResidentFactors(ctx, r.real[0], r.real[1], r.images)
        got.append([rf.decode_crops(crops[3], size), *ctx.deflate_columns(src_real, mats[3]), *inflate(ctx, 3)])  # the default stream
        ctx.synchronize()
        for k, (crop, slots, lens, dst, status) in enumerate(got):
            assert torch.equal(crop, want_crops[k]), k
            assert torch.equal(lens, want_defl[k][1]), k
            offs = torch.from_numpy(_lib.deflate_column_offsets(_lib.deflate_table(mats[k])[0])).cuda()
            ends = offs + want_defl[k][1].long()
            mark = torch.zeros((slots.numel() + 1,), dtype=torch.int32, device="cuda")
            mark.index_add_(0, offs, torch.ones_like(offs, dtype=torch.int32))
            mark.index_add_(0, ends, -torch.ones_like(ends, dtype=torch.int32))
            keep = mark.cumsum(0)[:-1] > 0  # (a slot is written up to its stream's length)
            assert torch.equal(slots[keep], want_defl[k][0][keep]), k
            nbytes = dst.numel()
            assert status.tolist() == [0] * status.numel() and torch.equal(dst, src_real[:nbytes]), k
    finally:
        ctx.close()


def test_control_a_context_on_its_own_stream_reads_the_decoy(busy):
    """lrf_qmf_decode_rgb_u8 through the C ABI, the sequence of `on_stream` — but the context is on its own stream
    (lrf_ctx_use_own_stream), so the call is NOT ordered behind the producer and decodes the decoy factors.  Both buffers are valid
    memory throughout.  Then lrf_ctx_set_stream(S) and the same sequence: the real factors."""
    from lrf_amd import _lib
    lib = _lib.load()
    ctx = _lib.Context(0)  # (a context of the test's own: the shared one stays on torch's streams)
    try:
        H, W, ranks, B = 96, 160, (7, 3, 3), 8
        dims = _lib.plane_dims(H, W)
        nu, nv = sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks)
        g = torch.Generator().manual_seed(8)
        real = [torch.randint(-16, 16, (B, n), dtype=torch.int8, generator=g).cuda() for n in (nu, nv)]
        decoy = [torch.randint(-16, 16, (B, n), dtype=torch.int8, generator=g).cuda() for n in (nu, nv)]
        want_real = _ctx().decode_rgb(real[0], real[1], H, W, list(ranks))
        want_decoy = _ctx().decode_rgb(decoy[0], decoy[1], H, W, list(ranks))
        assert not torch.equal(want_real, want_decoy)
        U, V = decoy[0].clone(), decoy[1].clone()
        out = torch.zeros((B, 3, H, W), dtype=torch.uint8, device="cuda")
        R = (ctypes.c_int * 3)(*ranks)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())

        def call():
            _lib.check(lib.lrf_qmf_decode_rgb_u8(ctx._h, ptr(U), ptr(V), B, H, W, R, ptr(out)))
            return out
        inputs = [(U, real[0], decoy[0]), (V, real[1], decoy[1])]
        S = torch.cuda.Stream()
        _lib.check(lib.lrf_ctx_use_own_stream(ctx._h))
        got = on_stream(S, busy, inputs, [call])[0]
        ctx.synchronize()
        assert torch.equal(got[0], want_decoy), "the control read the real factors: the producer is too short"
        assert torch.equal(out, want_decoy)
        out.zero_()
        torch.cuda.synchronize()
        _lib.check(lib.lrf_ctx_set_stream(ctx._h, ctypes.c_void_p(S.cuda_stream)))
        got = on_stream(S, busy, inputs, [call])[0]
        assert torch.equal(got[0], want_real)
        _lib.check(lib.lrf_ctx_use_own_stream(ctx._h))  # back: waits for S, then the context's own stream again
        out.zero_()
        torch.cuda.synchronize()
        call()
        ctx.synchronize()
        assert torch.equal(out, want_decoy)
    finally:
        ctx.close()
