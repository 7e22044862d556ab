"""What tests/test_deflate_host.py and tests/test_deflate_gpu.py share: the columns the issue names and the host restatement
(lrf_pack_deflate_column_i8 of liblrf_pack.so) through ctypes."""
import ctypes
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T = 2048  # LRFD_T (lrf_amd/csrc/lrf_deflate_shared.h); test_deflate_host.py checks it against the header through its shim
ROWS = [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 4180, 6144, 65535, 65536, 65537]
CONTENTS = ["zero", "m16", "two", "u32", "full", "geo", "fib"]


def fibonacci_column():
    """17 distinct values with counts 1, 1, 2, 3, ..., 1597 (4,180 rows), shuffled with a fixed seed"""
    counts = [1, 1]
    while len(counts) < 17:
        counts.append(counts[-1] + counts[-2])
    col = np.repeat(np.arange(-8, 9, dtype=np.int8), counts)
    assert col.size == 4180
    return np.random.default_rng(1597).permutation(col)


def column(content, rows, seed=0):
    rng = np.random.default_rng([seed, rows, CONTENTS.index(content)])
    if content == "zero":
        c = np.zeros(rows)
    elif content == "m16":
        c = np.full(rows, -16)
    elif content == "two":
        c = rng.choice([-3, 5], rows)
    elif content == "u32":
        c = rng.integers(-16, 16, rows)
    elif content == "full":
        c = rng.integers(-128, 128, rows)
    elif content == "geo":
        c = np.minimum(rng.geometric(0.4, rows) - 1, 15) * rng.choice([-1, 1], rows)
    else:
        c = np.resize(fibonacci_column(), rows) if rows != 4180 else fibonacci_column()
    return np.ascontiguousarray(c, dtype=np.int8)


def pairs():
    """every (rows, content) pair; the Fibonacci column exists at its own 4,180 rows only"""
    return [(r, c) for r in ROWS for c in CONTENTS if c != "fib" or r == 4180]


_LIB = None


def pack_lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "lrf_amd", "liblrf_pack.so"))
        lib.lrf_pack_deflate_bound.restype = ctypes.c_int64
        lib.lrf_pack_deflate_bound.argtypes = [ctypes.c_int64]
        lib.lrf_pack_deflate_column_i8.restype = ctypes.c_int64
        lib.lrf_pack_deflate_column_i8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
        _LIB = lib
    return _LIB


def bound(rows):
    return 2 + 5 * -(-rows // 65535) + rows + 4


def host_stream(col, stride=1, guard=16):
    """the restatement's stream of an int8 column laid out with `stride`; checks the bound and that nothing behind the
    returned length was touched"""
    col = np.asarray(col, dtype=np.int8)
    rows = col.size
    src = np.full((rows, stride), 77, dtype=np.int8)
    src[:, 0] = col
    cap = pack_lib().lrf_pack_deflate_bound(rows)
    assert cap == bound(rows)
    dst = np.full(cap + guard, 0xA5, dtype=np.uint8)
    n = pack_lib().lrf_pack_deflate_column_i8(src.ctypes.data, rows, stride, dst.ctypes.data, cap)
    assert 0 < n <= cap, n
    assert (dst[n:] == 0xA5).all(), "bytes behind the stream were written"
    return dst[:n].tobytes()


def golden_factor_sets():
    """[(name, [six 2-D int8 matrices])]: every tests/golden/*.npz whose `encoded` parses into six per-column matrices"""
    from lrf_amd.container import decode_tensor, separate_bytes
    out = []
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "*.npz"))):
        z = np.load(path)
        if "encoded" not in z.files:
            continue
        try:
            fac = [decode_tensor(f) for f in separate_bytes(separate_bytes(z["encoded"].tobytes(), 2)[1], 6)]
        except Exception:
            continue
        if len(fac) == 6 and all(f.ndim == 2 and f.dtype == np.int8 for f in fac):
            out.append((os.path.basename(path)[:-4], fac))
    return out
