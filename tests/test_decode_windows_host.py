"""CPU suite: the window list of the ten entries that decode crops (check_window_call, check_windows: lrf_amd/csrc/lrf_plan.cpp) —
next to describe_images the one check between a C caller's crop list and an out-of-bounds read in a kernel, and the items the
kernels index with.  The source needs no device: it is built here with g++ together with tests/decode_windows_host_shim.cpp and
called through ctypes.

Every refusal names the check, the crop and the operands its message needs; accepted lists come back in call order.  The
independent oracle is the Python layer's own validation (_lib.check_crop_args, check_scaled_args, check_resized_args,
check_gray_crop_args, check_gray_resized_args on zero host tensors): seeded random lists go through both."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from lrf_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
OK, N_IMAGES, N_CROPS, SIZE, CAPACITY, IMAGE, SCALE, SIDES, BOX = range(9)  # WIN_* of lrf_plan.h
I32, I64 = 2 ** 31 - 1, 2 ** 63 - 1
COLOUR_SCALES, GRAY_SCALES = 0x114, 0x116  # LRF_WIN_SCALES_*: bit f set for every admitted scale f
assert COLOUR_SCALES == sum(1 << f for f in _lib.SCALES) and GRAY_SCALES == sum(1 << f for f in _lib.GRAY_SCALES)
# kind: (shape: 0 lrf_crop / 1 lrf_scaled_crop / 2 lrf_resized_crop, gray, admitted scales, channels)
KINDS = {"crops": (0, False, 0, 3), "scaled": (1, False, COLOUR_SCALES, 3), "resized": (2, False, 0, 3),
         "gray_crops": (1, True, GRAY_SCALES, 1), "gray_resized": (2, True, 0, 1)}
SIZES = [(24, 48), (45, 61)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("decode_windows") / "libdecode_windows_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "decode_windows_host_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_check_windows.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                           ctypes.c_long, ctypes.c_uint, ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def windows(lib, kind, crops, size, sizes=SIZES, out_len=None, n_images=None, n_crops=None, want_items=True):
    """crops: rows of the kind's ABI shape; size: (h, w) or (oh, ow); out_len None: the exact fit; n_images, n_crops: what the call
    claims, if not the lists' lengths -> (check, crop, image, scale, y0, x0, h, w, H, W), the items [n, 10] or None"""
    shape, gray, scales, channels = KINDS[kind]
    arr = np.ascontiguousarray(np.asarray(crops, dtype=np.int64).reshape(-1, (3, 4, 6)[shape]), dtype=np.int32)
    n = arr.shape[0] if n_crops is None else n_crops
    dims = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64).reshape(-1, 2))
    refusal = np.full(10, -7, dtype=np.int64)
    items = np.full((arr.shape[0], 10), -7, dtype=np.int64) if want_items else None
    rc = lib.lrf_test_check_windows(shape, gray, dims.shape[0] if n_images is None else n_images, dims.ctypes.data, n, arr.ctypes.data, size[0], size[1],
                                    scales, channels, channels * size[0] * size[1] * n if out_len is None else out_len, refusal.ctypes.data,
                                    items.ctypes.data if want_items else None)
    assert rc == refusal[0]
    return tuple(int(x) for x in refusal), items if rc == OK else None


def crop_row(kind, image, scale, y0, x0, h, w, flip=0):
    """the fields of one crop as a row of the kind's ABI shape (a field the shape lacks is dropped)"""
    return {0: [image, y0, x0], 1: [image, scale, y0, x0], 2: [image, y0, x0, h, w, flip]}[KINDS[kind][0]]


def good(kind):
    """three windows of 8x12 inside the two images (the scaled kinds: at scale 2), (h, w) of the call"""
    f = 2 if KINDS[kind][0] == 1 else 1
    return [crop_row(kind, 0, f, 0, 0, 8, 12), crop_row(kind, 1, f, 3, 5, 8, 12, 1), crop_row(kind, 1, f, 14, 18, 8, 12)], (8, 12)


def level(kind, image, f):
    H, W = SIZES[image]
    return -(-H // f), -(-W // f)


def refusal_table(kind):
    """name -> (the crop that replaces crop 1 of good(kind), the (check, image, scale, y0, x0, h, w, H, W) expected)"""
    shape = KINDS[kind][0]
    f = 2 if shape == 1 else 1
    H, W = level(kind, 1, f)
    t = {}
    for name, image in (("image -1", -1), ("image 2", 2), ("image INT32_MAX", I32), ("image INT32_MIN", -I32 - 1)):
        t[name] = ((image, f, 0, 0, 8, 12), (IMAGE, image, f, 0, 0, 8, 12, 0, 0))
    for name, y0, x0, h, w in (("y0 -1", -1, 0, 8, 12), ("x0 -1", 0, -1, 8, 12), ("one row past", H - 8 + 1, 0, 8, 12), ("one column past", 0, W - 12 + 1, 8, 12),
                               ("y0 INT32_MAX", I32, 0, 8, 12), ("x0 INT32_MAX", 0, I32, 8, 12), ("y0 INT32_MIN", -I32 - 1, 0, 8, 12)):
        t[name] = ((1, f, y0, x0, h, w), (BOX, 1, f, y0, x0, h, w, H, W))
    if shape == 1:
        bad = (-1, 0, 3, 5, 6, 7, 9, 16, 32, I32, -I32 - 1) + (() if kind == "gray_crops" else (1,))
        for s in bad:
            t[f"scale {s}"] = ((1, s, 0, 0, 8, 12), (SCALE, 1, s, 0, 0, 8, 12, 0, 0))
    if shape == 2:
        for name, h, w in (("h 0", 0, 12), ("w 0", 8, 0), ("h -1", -1, 12), ("w INT32_MIN", 8, -I32 - 1)):
            t[name] = ((1, 1, 0, 0, h, w), (SIDES, 1, 1, 0, 0, h, w, 0, 0))
        for name, y0, x0, h, w in (("a row too tall", 0, 0, H + 1, W), ("a column too wide", 0, 0, H, W + 1), ("h = w = INT32_MAX", 0, 0, I32, I32),
                                   ("INT32_MAX everywhere", I32, I32, I32, I32), ("h 1 at y0 INT32_MAX", I32, 0, 1, 1), ("w 1 at x0 = W", 0, W, 1, 1)):
            t[name] = ((1, 1, y0, x0, h, w), (BOX, 1, 1, y0, x0, h, w, H, W))
    return t


CASES = [(kind, name) for kind in KINDS for name in refusal_table(kind)]


@pytest.mark.parametrize("kind,name", CASES)
def test_the_first_offender_is_named(lib, kind, name):
    """the bad crop at place 1, a different offender behind it: the refusal names crop 1, its check and its operands"""
    crop, want = refusal_table(kind)[name]
    crops, size = good(kind)
    crops[1] = crop_row(kind, *crop)
    crops[2] = crop_row(kind, 5, 3, -1, -1, 0, 0)  # (refused by every check)
    got, items = windows(lib, kind, crops, size)
    assert got == (want[0], 1) + want[1:] and items is None
    crops[0], crops[1] = crops[1], crops[0]  # in front it is found at place 0
    assert windows(lib, kind, crops, size)[0] == (want[0], 0) + want[1:]


@pytest.mark.parametrize("kind", KINDS)
def test_the_order_of_the_checks_inside_one_crop(lib, kind):
    """image before scale before box sides before the box"""
    shape = KINDS[kind][0]
    crops, size = good(kind)
    f = 2 if shape == 1 else 1
    crops[1] = crop_row(kind, 2, 3, -1, -1, 0, 0)
    assert windows(lib, kind, crops, size)[0][:3] == (IMAGE, 1, 2)
    crops[1] = crop_row(kind, 1, 3, -1, -1, 0, 0)
    assert windows(lib, kind, crops, size)[0][:2] == ({0: BOX, 1: SCALE, 2: SIDES}[shape], 1)
    crops[1] = crop_row(kind, 1, f, -1, -1, 0, 0)
    assert windows(lib, kind, crops, size)[0][:2] == (SIDES if shape == 2 else BOX, 1)
    crops[1] = crop_row(kind, 1, f, -1, -1, 8, 12)
    assert windows(lib, kind, crops, size)[0][:2] == (BOX, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_the_ranges_of_the_call(lib, kind):
    """n_images, then n_crops, then the size — before the list is looked at (every crop here is bad)"""
    shape = KINDS[kind][0]
    top = 16384 if shape == 2 else I32
    bad = [crop_row(kind, 9, 3, -1, -1, 0, 0)]
    for n_images in (0, -1, 65536, I64):
        assert windows(lib, kind, bad, (0, 0), n_images=n_images, n_crops=0)[0][0] == N_IMAGES
    for n_crops in (0, -1, 2 ** 20 + 1, I64):
        assert windows(lib, kind, bad, (0, 0), n_crops=n_crops, out_len=I64)[0][0] == N_CROPS
    for size in ((0, 4), (4, 0), (-1, 4), (top + 1, 4), (4, top + 1), (I64, I64)):
        assert windows(lib, kind, bad, size, out_len=I64)[0][0] == SIZE
    assert windows(lib, kind, bad, (top, 1), out_len=I64)[0][0] == IMAGE
    assert windows(lib, kind, bad, (1, top), out_len=I64)[0][0] == IMAGE
    assert windows(lib, kind, [crop_row(kind, 65535, 3, -1, -1, 0, 0)], (4, 4), sizes=[(8, 8)] * 65535, out_len=I64)[0][:3] == (IMAGE, 0, 65535)


@pytest.mark.parametrize("kind", KINDS)
def test_the_capacity_of_the_output(lib, kind):
    """checked before any crop (crop 0 here is bad), against products that no 64-bit arithmetic holds"""
    shape, _, _, ch = KINDS[kind]
    crops, size = good(kind)
    n, fit = len(crops), ch * size[0] * size[1] * len(crops)
    assert windows(lib, kind, crops, size, out_len=fit)[0][0] == OK
    assert windows(lib, kind, crops, size, out_len=I64)[0][0] == OK
    bad = [crop_row(kind, 9, 3, -1, -1, 0, 0)] + crops[1:]
    assert windows(lib, kind, bad, size, out_len=fit)[0][0] == IMAGE
    for out_len in (fit - 1, fit - ch * size[0] * size[1], 2, 1, 0, -1, -I64 - 1):
        got = windows(lib, kind, bad, size, out_len=out_len)[0]
        assert got == (CAPACITY, 0, 0, 1, 0, 0, 0, 0, 0, 0), (out_len, got)
    # one pixel per crop: 2 elements hold two gray crops and no colour crop
    one = [crop_row(kind, 0, 1 if kind != "scaled" else 2, 0, 0, 1, 1)]
    assert windows(lib, kind, one * 2, (1, 1), out_len=2)[0][0] == (OK if ch == 1 else CAPACITY)
    assert windows(lib, kind, one * 3, (1, 1), out_len=2)[0][0] == CAPACITY
    if shape != 2:  # windows of INT32_MAX x INT32_MAX: 3 h w is beyond int64, h w is not (two gray ones fit INT64_MAX, three do not)
        big = (I32, I32)
        assert windows(lib, kind, one, big, out_len=I64)[0][0] == (BOX if ch == 1 else CAPACITY)
        assert windows(lib, kind, one * 2, big, out_len=I64)[0][0] == (BOX if ch == 1 else CAPACITY)
        assert windows(lib, kind, one * 3, big, out_len=I64)[0][0] == CAPACITY
        assert windows(lib, kind, one, (I32, 1), out_len=ch * I32)[0][0] == BOX
        assert windows(lib, kind, one, (I32, 1), out_len=ch * I32 - 1)[0][0] == CAPACITY
    else:  # the largest output: 2^20 boxes to 16384 x 16384 are 3 x 2^48 elements
        top = 16384
        assert windows(lib, kind, one, (top, top), out_len=ch * top * top)[0][0] == OK
        assert windows(lib, kind, one, (top, top), out_len=ch * top * top - 1)[0][0] == CAPACITY


@pytest.mark.parametrize("kind", KINDS)
def test_the_longest_list(lib, kind):
    """2^20 crops: accepted into INT64_MAX elements and into the exact fit, refused one element short of it; the last crop bad:
    named at 2^20 - 1"""
    shape, _, _, ch = KINDS[kind]
    n, size = 2 ** 20, (4, 6)
    f = 2 if shape == 1 else 1
    crops = np.array([crop_row(kind, 1, f, 2, 3, 4, 6, 1)] * n, dtype=np.int32)
    crops[:, 2 if shape == 2 else -1] = np.arange(n) % 8  # x0
    fit = ch * 4 * 6 * n
    got, items = windows(lib, kind, crops, size, out_len=I64)
    assert got[0] == OK
    assert np.array_equal(items[:, 7], np.arange(n)) and np.array_equal(items[:, 3], np.arange(n) % 8) and (items[:, 0] == 1).all()
    assert windows(lib, kind, crops, size, out_len=fit, want_items=False)[0][0] == OK
    assert windows(lib, kind, crops, size, out_len=fit - 1, want_items=False)[0][0] == CAPACITY
    crops[n - 1, 0] = 2
    assert windows(lib, kind, crops, size, want_items=False)[0][:3] == (IMAGE, n - 1, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_accepted_lists_come_back_in_call_order(lib, kind):
    """every field of every item, windows that touch each edge of their image among them"""
    shape, gray, scales, ch = KINDS[kind]
    fs = [f for f in (1, 2, 4, 8) if scales >> f & 1] or [1]
    h, w = (3, 5)
    rows, want = [], []
    for image in (1, 0, 1):
        for f in fs:
            H, W = level(kind, image, f)
            boxes = [(0, 0, H, W), (0, 0, 1, 1), (H - 1, W - 1, 1, 1), (H - 2, 1, 2, W - 1)] if shape == 2 else [(0, 0, h, w), (H - h, W - w, h, w), (H - h, 0, h, w)]
            for y0, x0, bh, bw in boxes:
                flip = len(rows) % 3  # (0, 1, 2: any value but 0 flips)
                rows.append(crop_row(kind, image, f, y0, x0, bh, bw, flip))
                j = len(want)
                if kind == "crops":
                    want.append((image, -1, y0, x0, -1, -1, -1, j, -1, -1))
                elif kind == "scaled":
                    want.append((image, f, y0, x0, h, w, -1, j, 3 * h * w * j, 0))
                elif kind == "resized":
                    want.append((image, 1, y0, x0, bh, bw, int(flip != 0), j, -1, -1))
                elif kind == "gray_crops":
                    want.append((image, f, y0, x0, h, w, 0, j, h * w * j, w))
                else:  # (plan_gray_resized sets out_off and pitch)
                    want.append((image, 1, y0, x0, bh, bw, int(flip != 0), j, 0, 0))
    got, items = windows(lib, kind, rows, (h, w))
    assert got == (OK, 0, 0, 1, 0, 0, 0, 0, 0, 0)
    assert items.tolist() == [list(x) for x in want]


@pytest.mark.parametrize("kind", ["scaled", "gray_crops"])
def test_an_image_of_one_pixel_at_scale_8(lib, kind):
    """ceil(1 / 8) = 1: the level holds one pixel, and nothing else"""
    assert windows(lib, kind, [[0, 8, 0, 0]], (1, 1), sizes=[(1, 1)])[0][0] == OK
    for y0, x0, size in ((1, 0, (1, 1)), (0, 1, (1, 1)), (0, 0, (2, 1)), (0, 0, (1, 2))):
        got = windows(lib, kind, [[0, 8, y0, x0]], size, sizes=[(1, 1)])[0]
        assert got == (BOX, 0, 0, 8, y0, x0) + size + (1, 1)
    # 9 rows are two rows at scale 8, 8 rows one
    assert windows(lib, kind, [[0, 8, 1, 0]], (1, 1), sizes=[(9, 1)])[0][0] == OK
    assert windows(lib, kind, [[0, 8, 1, 0]], (1, 1), sizes=[(8, 1)])[0][:2] == (BOX, 0)


# ---- the Python layer's validation as the oracle -----------------------------------------------------------------------------------
def _usable(gray, H, W):
    try:
        _lib.chan_dims(H, W, 1, (8, 8)) if gray else _lib.plane_dims(H, W)
    except ValueError:
        return False
    return True


def _image_list(rng, gray):
    """two to four images of sides 1..70 the decoders take, zero factors on the host"""
    images, uo, vo, n = [], 0, 0, int(rng.integers(2, 5))
    while len(images) < n:
        H, W = (int(x) for x in rng.integers(1, 71, size=2))
        if not _usable(gray, H, W):
            continue
        if gray:
            images.append((H, W, 1, uo, vo))
            uo, vo = uo + _lib.chan_dims(H, W, 1, (8, 8))[2], vo + 64
        else:
            images.append((H, W, (1, 1, 1), uo, vo))
            uo, vo = uo + sum(d[4] for d in _lib.plane_dims(H, W)), vo + 192
    return torch.zeros(uo, dtype=torch.int8), torch.zeros(vo, dtype=torch.int8), images


def _python_check(kind, U, V, images, crops, size):
    """-> None, or (check, crop) of the refusal"""
    fn = {"crops": _lib.check_crop_args, "resized": _lib.check_resized_args, "gray_crops": _lib.check_gray_crop_args,
          "gray_resized": _lib.check_gray_resized_args, "scaled": lambda U, V, images, crops, size: _lib.check_scaled_args(U, V, images, crops=crops, size=size)}[kind]
    try:
        fn(U, V, images, crops, size)
    except ValueError as e:
        m = re.match(r"crop (\d+): (.*)", str(e))
        assert m, str(e)
        what = m.group(2)
        check = IMAGE if what.startswith("image ") else SCALE if what.startswith("scale ") else SIDES if what.startswith("box of ") else BOX
        assert check != BOX or " leaves image " in what, str(e)
        return check, int(m.group(1))
    return None


def _random_crop(rng, kind, images, size, bad):
    """one crop inside its image — or, `bad`, with one field out of range"""
    shape, _, scales, _ = KINDS[kind]
    fs = [f for f in (1, 2, 4, 8) if scales >> f & 1] or [1]
    for _ in range(64):
        image, f = int(rng.integers(len(images))), int(rng.choice(fs))
        H, W = -(-images[image][0] // f), -(-images[image][1] // f)
        h, w = (int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))) if shape == 2 else size
        if h <= H and w <= W:
            break
    else:
        return None
    y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    if bad:
        far = [int(x) for x in (-1, -I32 - 1, I32, rng.integers(-70, 0), rng.integers(71, 200))]
        what = str(rng.choice(["image", "y0", "x0"] + ["scale"] * (shape == 1) + ["h", "w"] * (shape == 2)))
        if what == "image":
            image = int(rng.choice([-1, len(images), len(images) + 1, I32, -I32 - 1]))
        elif what == "scale":
            f = int(rng.choice([s for s in (-1, 0, 1, 3, 5, 6, 7, 9, 16, I32) if s not in fs]))
        elif what == "y0":
            y0 = int(rng.choice(far + [H - h + 1]))
        elif what == "x0":
            x0 = int(rng.choice(far + [W - w + 1]))
        elif what == "h":
            h = int(rng.choice([0, -1, H + 1, I32, H - y0 + 1]))
        else:
            w = int(rng.choice([0, -1, W + 1, I32, W - x0 + 1]))
    return crop_row(kind, image, f, y0, x0, h, w, int(rng.integers(0, 3)))


@pytest.mark.parametrize("kind", KINDS)
def test_random_lists_against_the_python_checks(lib, kind):
    """800 seeded lists per kind (4000 in all), a third of them good, a third with exactly one bad crop, a third with several:
    accept / refuse agree on every list, and with one bad crop its place and the check agree too (the Python checks are
    vectorised by check, so with several bad crops they may name another one)"""
    shape, gray, _, ch = KINDS[kind]
    rng = np.random.default_rng(2024 + sorted(KINDS).index(kind))
    counts = {"accepted": 0, "one bad": 0, "several bad": 0}
    for trial in range(800):
        if trial % 40 == 0:
            U, V, images = _image_list(rng, gray)
            sizes = [im[:2] for im in images]
        f_max = 1 if shape != 1 else 8
        size = (int(rng.integers(1, 12)), int(rng.integers(1, 12))) if shape == 2 else \
               (int(rng.integers(1, -(-min(s[0] for s in sizes) // f_max) + 1)), int(rng.integers(1, -(-min(s[1] for s in sizes) // f_max) + 1)))
        n = int(rng.integers(1, 12))
        n_bad = (0, 1, int(rng.integers(2, 5)))[trial % 3]
        places = set(rng.choice(n, size=min(n_bad, n), replace=False).tolist())
        crops = [_random_crop(rng, kind, images, size, j in places) for j in range(n)]
        assert None not in crops
        want = _python_check(kind, U, V, images, np.array(crops, dtype=np.int64), size)
        got, items = windows(lib, kind, crops, size, sizes=sizes)
        assert (got[0] == OK) == (want is None), (images, crops, size, got, want)
        if want is None:
            assert not places and items[:, 7].tolist() == list(range(n))
            counts["accepted"] += 1
        elif len(places) == 1:
            assert got[:2] == want and got[1] in places, (images, crops, size, got, want)
            counts["one bad"] += 1
        else:
            assert got[1] == min(places), (images, crops, size, got, want)
            counts["several bad"] += 1
    print(kind, counts)
    assert min(counts.values()) >= 200


# ---- the sanitizer program --------------------------------------------------------------------------------------------------
def test_sanitizer_program_is_clean(tmp_path):
    """tools/windows_san_main.cpp: check_window_call and check_windows under ASan and UBSan, as a program of its own — every field
    at the extremes of int32, the call's numbers at those of int64, 2^20 crops"""
    exe = str(tmp_path / "windows_san")
    # (the sanitizer runtimes linked statically: ASan's start-up check that its runtime comes first among the loaded libraries does
    # not apply then, so the program also starts in an environment that preloads a library of its own)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HERE, "..", "tools", "windows_san_main.cpp"),
                           os.path.join(HERE, "decode_windows_host_shim.cpp"), os.path.join(CSRC, "lrf_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " calls, 0 failures" in r.stdout


# ---- the Python layer's limit of 2^20 crops is per kernel call ------------------------------------------------------------------
def test_a_mixed_scale_list_is_limited_per_part():
    """qmf_decode_crops with per-crop scales makes two kernel calls, full-size and scaled: each takes 1 to 2^20 crops, so a list of
    2^20 + 2 crops passes when neither part is longer, and is refused when one part is"""
    from lrf_amd.codec import _split_crops_by_scale
    U, V, images = _image_list(np.random.default_rng(5), False)
    n = 2 ** 20 + 2
    crops = np.zeros((n, 3), dtype=np.int64)
    scale = np.where(np.arange(n) % 2 == 0, 1, 8)
    full, b1, scaled, b2 = _split_crops_by_scale(U, V, images, crops, (1, 1), scale)
    assert full.size == scaled.size == n // 2 and b1.shape == (n // 2, 3) and b2.shape == (n // 2, 4) and (b2[:, 1] == 8).all()
    scale[:] = 8
    scale[0] = 1
    with pytest.raises(ValueError, match="decode_scaled_crops needs 1 to 2\\^20 crops"):
        _split_crops_by_scale(U, V, images, crops, (1, 1), scale)
    with pytest.raises(ValueError, match="decode_crops needs 1 to 2\\^20 crops"):
        _split_crops_by_scale(U, V, images, crops, (1, 1), 9 - scale)
