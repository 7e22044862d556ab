"""What tests/test_inflate_host.py, tests/test_inflate_gpu.py and the sanitizer program share: the corpus of zlib streams, the
hand-built streams, the fixed list CORRUPT, and the host restatement (lrf_pack_inflate_column_i8 of liblrf_pack.so) through
ctypes.  Every list is built once per process and never changed."""
import ctypes
import functools
import os
import struct
import zlib

import numpy as np

import deflate_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = None


def pack_lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "lrf_amd", "liblrf_pack.so"))
        lib.lrf_pack_inflate_column_i8.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
        lib.lrf_pack_inflate_max_distance.restype = ctypes.c_int64
        lib.lrf_pack_inflate_max_distance.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64]
        lib.lrf_pack_index_qmf_columns_ragged.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_int64,
                                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_int64]
        _LIB = lib
    return _LIB


MARK, GUARD = -77, 64


def host_inflate(stream, rows, stride=1):
    """-> (status, the column or None): the restatement on a marker-filled buffer; asserts that the padding between the elements
    and the guard behind them are untouched whatever the status"""
    buf = np.full(rows * stride + GUARD, MARK, dtype=np.int8)
    rc = pack_lib().lrf_pack_inflate_column_i8(bytes(stream), len(stream), buf.ctypes.data, rows, stride)
    body = buf[:rows * stride].reshape(rows, stride)
    assert (buf[rows * stride:] == MARK).all(), "the guard behind the column was written"
    assert (body[:, 1:] == MARK).all(), "padding between the column's elements was written"
    return rc, (np.ascontiguousarray(body[:, 0]) if rc == 0 else None)


def zlib_verdict(stream, rows):
    """what zlib.decompress makes of it: the bytes when it succeeds with exactly `rows` of them, else None"""
    try:
        out = zlib.decompress(bytes(stream))
    except zlib.error:
        return None
    return out if len(out) == rows else None


def deflate_with(data, level, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return co.compress(data) + co.flush()


VARIANTS = [("l0", dict(level=0)), ("l1", dict(level=1)), ("l6", dict(level=6)), ("l9", dict(level=9)),
            ("fixed", dict(level=9, strategy=zlib.Z_FIXED)), ("huff", dict(level=9, strategy=zlib.Z_HUFFMAN_ONLY)),
            ("rle", dict(level=9, strategy=zlib.Z_RLE)), ("w9", dict(level=9, wbits=9)), ("w15", dict(level=9, wbits=15))]


def period_column():
    """40,000 rows: a random period of 32,768 bytes repeated, whose every byte behind the first period is a match at distance 32,768"""
    p = np.random.default_rng(32768).integers(-128, 128, 32768).astype(np.int8)
    return np.resize(p, 40000)


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, stream, column bytes)]: every distinct column of the golden factor sets and those of deflate_cases.pairs() at rows <= 6144,
    each through every variant and through the project's own coder; one column each of 65,535 / 65,536 / 65,537 rows; the
    distance-32,768 column"""
    cols, seen = [], set()
    for name, fac in dc.golden_factor_sets():
        for f, m in enumerate(fac):
            for j in range(m.shape[1]):
                c = np.ascontiguousarray(m[:, j])
                if c.tobytes() not in seen:  # (every golden column, whatever its length; equal columns once)
                    seen.add(c.tobytes())
                    cols.append((f"{name}.f{f}.c{j}", c))
    for rows, content in dc.pairs():
        if rows <= 6144:
            cols.append((f"{content}{rows}", dc.column(content, rows)))
    out = []
    for name, c in cols:
        data = c.tobytes()
        for v, kw in VARIANTS:
            out.append((f"{name}.{v}", deflate_with(data, **kw), data))
        out.append((f"{name}.own", dc.host_stream(c), data))
    for rows in (65535, 65536, 65537):
        c = dc.column("geo", rows)
        out.append((f"geo{rows}.l9", deflate_with(c.tobytes(), 9), c.tobytes()))
        out.append((f"geo{rows}.own", dc.host_stream(c), c.tobytes()))
    # The period column.  zlib's own matcher never looks further back than 32,768 - 262 bytes (deflate.h: MAX_DIST), so its
    # level-9 stream of this column holds no match at the full distance; the writer below states them: the first period stored,
    # the rest as matches of distance 32,768 exactly.  That such a match is really read is asserted from the restatement's count.
    c = period_column()
    out.append(("period32768.l9", deflate_with(c.tobytes(), 9), c.tobytes()))
    w = Bits()
    stored_block(w, c[:32768].tobytes(), final=False)
    rest = c.size - 32768
    fixed_block(w, [(258, 32768)] * (rest // 258) + [(rest % 258, 32768), 256])
    w.align()
    z = b"\x78\xda" + bytes(w.out) + struct.pack(">I", zlib.adler32(c.tobytes()))
    assert zlib.decompress(z) == c.tobytes() and rest % 258 >= 3
    far = pack_lib().lrf_pack_inflate_max_distance(z, len(z), c.size)
    assert far == 32768, f"the period column's stream has no match at distance 32,768 (largest: {far})"
    out.append(("period32768.far", z, c.tobytes()))
    return out


# ---- a deflate writer for streams zlib would never emit ----------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):  # LSB first: header fields and extra bits
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):  # a Huffman code: most significant bit first
        for i in range(n - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += bytes(b)


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2)"""
    code, out = 0, {}
    for l in range(1, 16):
        for s, ls in enumerate(lens):
            if ls == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def put_items(w, items, lit, dist):
    """items: ints (literals, 256 = end of block) and (length, distance) pairs, or ("sym", s) / ("dsym", s) for a bare symbol"""
    for it in items:
        if isinstance(it, int):
            w.code(*lit[it])
        elif it[0] == "sym":
            w.code(*lit[it[1]])
        elif it[0] == "dsym":
            w.code(*dist[it[1]])
        else:
            length, d = it
            ls = max(i for i in range(29) if LEN_BASE[i] <= length) if length != 258 else 28
            w.code(*lit[257 + ls])
            w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(i for i in range(30) if DIST_BASE[i] <= d)
            w.code(*dist[ds])
            w.bits(d - DIST_BASE[ds], DIST_EXTRA[ds])


def fixed_block(w, items, final=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_items(w, items, FIXED_LIT, FIXED_DIST)


def stored_block(w, data, final=True, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xffff) if nlen is None else nlen))
    w.raw(data)


def flat_cl_lens(used):
    """lengths of a complete code over the code-length symbols in `used` (at least two)"""
    used = sorted(used)
    k = max(1, (len(used) - 1).bit_length())
    short = (1 << k) - len(used)
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    return lens


def dynamic_block(w, litlens, distlens, items, final=True, cl_lens=None, seq=None, hlit=None, hdist=None):
    """seq: the code-length symbols to send, ints or (16 | 17 | 18, extra value); default: every length as itself"""
    if seq is None:
        seq = list(litlens) + list(distlens)
    if cl_lens is None:
        used = {s if isinstance(s, int) else s[0] for s in seq}
        if len(used) < 2:
            used |= {0, 1}
        cl_lens = flat_cl_lens(used)
    cl = canonical(cl_lens)
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(litlens) - 257 if hlit is None else hlit, 5)
    w.bits(len(distlens) - 1 if hdist is None else hdist, 5)
    hclen = max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]] or i < 4)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lens[CL_ORDER[i]], 3)
    for s in seq:
        if isinstance(s, int):
            w.code(*cl[s])
        else:
            w.code(*cl[s[0]])
            w.bits(s[1], {16: 2, 17: 3, 18: 7}[s[0]])
    put_items(w, items, canonical(litlens), canonical(distlens))


def lit_lens(spec, n=257):
    lens = [0] * n
    for s, l in spec.items():
        lens[s] = l
    return lens


@functools.lru_cache(maxsize=None)
def hand_built():
    """[(name, stream, the bytes zlib.decompress gives)]; each is checked against zlib here"""
    out = []

    def finish(name, w, trailer=b""):
        w.align()
        body = bytes(w.out)
        data = zlib.decompressobj(-15).decompress(body)
        z = b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data)) + trailer
        assert zlib.decompress(z) == data and len(data) >= 1, name
        out.append((name, z, data))

    w = Bits(); fixed_block(w, [7, (258, 1), 256]); finish("overlap258", w)
    w = Bits(); fixed_block(w, [1, 2, 3, 4, 5, (5, 5), 256]); finish("dist_is_written", w)
    w = Bits()
    stored_block(w, bytes(range(40)), final=False)
    fixed_block(w, [200, 201, (30, 42), 256], final=False)
    dynamic_block(w, lit_lens({5: 2, 6: 2, 256: 2, 257: 2}, 258), [1, 1], [5, 6, 5, (3, 2), 256])
    finish("three_blocks", w)
    w = Bits(); stored_block(w, b"", final=False); fixed_block(w, [9, 8, 7, 256]); finish("empty_stored_first", w)
    w = Bits(); stored_block(w, np.random.default_rng(65535).integers(0, 256, 65535).astype(np.uint8).tobytes()); finish("stored65535", w)
    w = Bits(); dynamic_block(w, lit_lens({3: 1, 256: 2, 260: 2}, 261), [1], [3, 3, (6, 1), 3, 256]); finish("single_dist_code", w)
    # literal codes of 1..15 bits (symbols 0..14 and end-of-block) behind a code-length code that uses all 19 symbols, two at 7 bits
    ll = lit_lens({**{s: s + 1 for s in range(14)}, 14: 15, 256: 15})
    cl_lens = [0] * 19
    for s in range(1, 16):
        cl_lens[s] = 4
    cl_lens[0], cl_lens[18], cl_lens[16], cl_lens[17] = 5, 6, 7, 7
    seq = list(range(1, 15)) + [15] + [(18, 138 - 11), (18, 241 - 138 - 11), 15] + [(17, 0), 0]  # 15 + 241 zeros + EOB; four distance lengths of 0
    dynamic_block(w := Bits(), ll, [0, 0, 0, 0], [0, 14, 13, 1, 0, 12, 256], cl_lens=cl_lens, seq=seq)
    finish("lit15_cl7", w)
    # eight codes of three bits, seven of them sent as one length and a repeat-previous code
    w = Bits(); dynamic_block(w, lit_lens({0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 6: 3, 256: 3}), [1, 1], [0, 1, 2, 3, 4, 5, 6, 256],
                              seq=[3, (16, 3), (18, 138 - 11), (18, 249 - 138 - 11), 3, 1, 1]); finish("repeat16", w)
    w = Bits(); fixed_block(w, [65, 66, 67, 256]); finish("trailing_bytes", w, trailer=b"\x00\xff garbage behind the checksum")
    return out


def _deflate_body(w):
    w.align()
    return bytes(w.out)


@functools.lru_cache(maxsize=None)
def refusals():
    """[(name, stream, rows)]: one hand-built stream per rule of refusal"""
    out = []

    def add(name, w, rows, header=b"\x78\x9c", adler=None, data=b""):
        out.append((name, header + _deflate_body(w) + struct.pack(">I", zlib.adler32(data) if adler is None else adler), rows))

    good = [65, 66, 67, 256]
    for name, hdr in (("cm7", b"\x77\x85"), ("cinfo8", b"\x88\x1c"), ("not31", b"\x78\x9d"), ("fdict", b"\x78\xbb")):
        w = Bits(); fixed_block(w, good); add("header_" + name, w, 3, header=hdr, data=b"ABC")
    assert all((h[0] * 256 + h[1]) % 31 == 0 for h in (b"\x77\x85", b"\x88\x1c", b"\x78\xbb"))
    w = Bits(); w.bits(1, 1); w.bits(3, 2); w.bits(0, 13); add("btype3", w, 3)
    w = Bits(); stored_block(w, b"ABC", nlen=0x1234); add("stored_nlen", w, 3, data=b"ABC")
    base = lit_lens({65: 1, 256: 1})
    w = Bits(); dynamic_block(w, base + [0] * 30, [1, 1], [65, 256]); add("hlit287", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, base, [1] * 2 + [0] * 29, [65, 256]); add("hdist31", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, lit_lens({65: 1, 66: 1, 256: 1}), [1, 1], []); add("oversubscribed", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, lit_lens({65: 2, 256: 2}), [1, 1], []); add("incomplete_lit", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, base, [2, 2], []); add("incomplete_dist", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, base, [1, 1], [], seq=[(16, 0), 1, 1]); add("repeat_first", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, base, [1, 1], [], seq=[0] * 65 + [1] + [(18, 127), (18, 127)]); add("repeat_past_end", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, lit_lens({65: 1, 66: 1}), [1, 1], []); add("no_end_of_block", w, 1, data=b"A")
    w = Bits(); dynamic_block(w, lit_lens({3: 1, 256: 2, 260: 2}, 261), [1], [3, 3, ("sym", 260)]); w.bits(1, 1); w.bits(0, 12); add("no_such_code", w, 8, data=b"\x03" * 8)
    w = Bits(); fixed_block(w, [65, ("sym", 286), 256]); add("length_symbol_286", w, 4, data=b"A")
    w = Bits(); fixed_block(w, [65, ("sym", 287), 256]); add("length_symbol_287", w, 4, data=b"A")
    w = Bits(); fixed_block(w, [65, ("sym", 257), ("dsym", 30), 256]); add("distance_symbol_30", w, 4, data=b"A")
    w = Bits(); fixed_block(w, [65, ("sym", 257), ("dsym", 31), 256]); add("distance_symbol_31", w, 4, data=b"A")
    w = Bits(); fixed_block(w, [65, 66, (3, 3), 256]); add("distance_too_far", w, 5, data=b"AB")
    w = Bits(); fixed_block(w, [65, 66, (10, 1), 256]); add("too_long", w, 11, data=b"AB" + b"B" * 10)
    w = Bits(); fixed_block(w, [65, 66, (10, 1), 256]); add("too_short", w, 13, data=b"AB" + b"B" * 10)
    w = Bits(); fixed_block(w, [65, 66, 67]); out.append(("input_exhausted", b"\x78\x9c" + _deflate_body(w), 3))  # ends inside a code
    w = Bits(); fixed_block(w, good); add("adler", w, 3, adler=zlib.adler32(b"ABC") ^ 0x10000)
    return out


@functools.lru_cache(maxsize=None)
def corrupt():
    """The fixed list CORRUPT [(name, stream, rows)]: of three short corpus streams every truncation and single-bit flips at
    seeded positions in the header, the code-length section, the body and the Adler-32; then the refusals"""
    out = []
    rng = np.random.default_rng(1951)
    picks = [("u32_63.l9", deflate_with(dc.column("u32", 63).tobytes(), 9), 63),
             ("geo64.l0", deflate_with(dc.column("geo", 64).tobytes(), 0), 64),
             ("two65.own", dc.host_stream(dc.column("two", 65)), 65)]
    for name, z, rows in picks:
        assert zlib_verdict(z, rows) is not None
        for cut in range(len(z)):
            out.append((f"{name}.cut{cut}", z[:cut], rows))
        regions = [(0, 2), (2, min(12, len(z) - 4)), (min(12, len(z) - 4), len(z) - 4), (len(z) - 4, len(z))]
        for r, (lo, hi) in enumerate(regions):
            lo = max(0, min(lo, hi - 1))
            for _ in range(4):
                p, bit = int(rng.integers(lo, hi)), int(rng.integers(0, 8))
                b = bytearray(z)
                b[p] ^= 1 << bit
                out.append((f"{name}.flip{r}.{p}.{bit}", bytes(b), rows))
    return out + refusals()


def dump(path):
    """The corpus, the hand-built streams and CORRUPT for tools/inflate_san_main.cpp: int64 count, then per stream int64 rows, int64
    length, int64 ok (1: zlib.decompress gives exactly `rows` bytes, which follow the stream), the stream, the bytes"""
    items = [(z, len(d)) for _, z, d in corpus() + hand_built()] + [(z, rows) for _, z, rows in corrupt()]
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(items)))
        for z, rows in items:
            want = zlib_verdict(z, rows)
            f.write(struct.pack("<qqq", rows, len(z), 0 if want is None else 1))
            f.write(z)
            if want is not None:
                f.write(want)
    return len(items)


def deflated_container(fac, metadata):
    """the stream lrf_pack_qmf_streams_deflated assembles from the project's own coder's columns of six factor matrices (what
    deflate="device" encoders write)"""
    lib = ctypes.CDLL(os.path.join(ROOT, "lrf_amd", "liblrf_pack.so"))
    chunks, col_off, col_len, at = [], [], [], 0
    for f in fac:
        for j in range(f.shape[1]):
            s = dc.host_stream(np.ascontiguousarray(f[:, j]))
            chunks.append(s)
            col_off.append(at)
            col_len.append(len(s))
            at += len(s)
    slots = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    col_off, col_len = np.array(col_off, dtype=np.int64), np.array(col_len, dtype=np.int32)
    M = np.array([fac[0].shape[0], fac[2].shape[0], fac[4].shape[0]], dtype=np.int64)
    R = np.array([fac[0].shape[1], fac[2].shape[1], fac[4].shape[1]], dtype=np.int32)
    out, out_len = (ctypes.c_void_p * 1)(), (ctypes.c_int64 * 1)()
    lib.lrf_pack_qmf_streams_deflated.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]
    lib.lrf_pack_free.argtypes = [ctypes.c_void_p]
    rc = lib.lrf_pack_qmf_streams_deflated(slots.ctypes.data, slots.size, 1, M.ctypes.data, R.ctypes.data, col_off.ctypes.data, col_len.ctypes.data,
                                           col_off.size, (ctypes.c_char_p * 1)(metadata), np.array([len(metadata)], dtype=np.int64).ctypes.data, 1,
                                           out, out_len)
    assert rc == 0
    stream = ctypes.string_at(out[0], out_len[0])
    lib.lrf_pack_free(out[0])
    return stream
