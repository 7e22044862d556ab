"""CPU suite: the image list of the decode and SSE entries (describe_images, lrf_amd/csrc/lrf_plan.cpp) — the one check between a
C caller's numbers and an out-of-bounds read in a kernel, and the descriptors the kernels index with.  The source needs no
device: it is built here with g++ together with tests/decode_images_host_shim.cpp and called through ctypes.

The refusals are the image-side rows of test_c_entry_refuses_on_the_host_and_launches_nothing (tests/test_decode_ragged_gpu.py),
asked of the host function: each names the check and the image it expects.  The descriptors are compared field by field with
their inputs, with geom_of, and byte by byte with a zeroed mirror filled from those fields (the bytes are the device table's
key, so what no field covers must be zero)."""
import ctypes
import os
import subprocess

import pytest

from lrf_amd import _lib
from test_decode_ragged_plan import ANY, R8, STRIP, TILE16, classify

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
OK, SIZE, GEOM, RANK, NEGATIVE, U_EXTENT, V_EXTENT, RGB_EXTENT = range(8)  # DESC_* of lrf_plan.h


class PlaneGeom(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("h", "w", "hp", "wp", "top", "left", "top_crop", "left_crop", "nw", "nh", "pr0", "M")] + \
               [("xoff", ctypes.c_long), ("o4", ctypes.c_long)]


class ImageGeom(ctypes.Structure):
    _fields_ = [("p", PlaneGeom * 3), ("tot4", ctypes.c_long), ("img_floats", ctypes.c_long)]


class RaggedDesc(ctypes.Structure):
    _fields_ = [("g", ImageGeom), ("u_off", ctypes.c_long), ("v_off", ctypes.c_long), ("rgb_off", ctypes.c_long)] + \
               [(k, ctypes.c_int) for k in ("H", "W", "R0", "R1", "R2", "kind", "cls", "per_strip")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("decode_images") / "libdecode_images_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "decode_images_host_shim.cpp")])
    lib = ctypes.CDLL(so)
    lib.lrf_test_sizeof_ragged_desc.restype = ctypes.c_long
    lib.lrf_test_describe_images.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_long, ctypes.c_int,
                                             ctypes.c_ulong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.lrf_test_geom_of.argtypes = [ctypes.c_long, ctypes.c_long, ctypes.c_void_p]
    assert lib.lrf_test_sizeof_ragged_desc() == ctypes.sizeof(RaggedDesc)
    return lib


def describe(lib, images, u_len, v_len, rgb_len=None, rgb_base=None, no_tiled=False, want_work=True):
    """images: (H, W, ranks, u_off, v_off, rgb_off).  rgb_len None: the output is not the images' (no rgb check); rgb_base None:
    every image counts as aligned -> (check, image, a, b), descriptors, [(kind, cls, units)]"""
    n = len(images)
    arr = (_lib.RaggedImage * n)()
    for d, (H, W, r, uo, vo, ro) in zip(arr, images):
        d.H, d.W, d.u_off, d.v_off, d.rgb_off = H, W, uo, vo, ro
        d.R[0], d.R[1], d.R[2] = r
    refusal = (ctypes.c_long * 4)()
    descs = (RaggedDesc * n)()
    work = (ctypes.c_long * (3 * n))()
    rc = lib.lrf_test_describe_images(n, arr, u_len, v_len, rgb_len is not None, rgb_len or 0, rgb_base is None, rgb_base or 0, no_tiled, refusal,
                                      descs, work if want_work else None)
    assert rc == refusal[0]
    return tuple(refusal), descs, [tuple(work[3 * i:3 * i + 3]) for i in range(n)]


def sizes_of(H, W, ranks):
    dims = _lib.plane_dims(H, W)
    return sum(d[4] * r for d, r in zip(dims, ranks)), 64 * sum(ranks), 3 * H * W


H0, W0, RANKS0 = 64, 96, (7, 3, 3)
NU, NV, NPX = sizes_of(H0, W0, RANKS0)
FIRST = (H0, W0, RANKS0, 0, 0, 0)


def second(H=H0, W=W0, ranks=RANKS0, u_off=NU, v_off=NV, rgb_off=NPX):
    return (H, W, ranks, u_off, v_off, rgb_off)


# name: (second image, lengths that differ from the exact fit, with the rgb check, (check, image, a, b) expected)
REFUSALS = {
    "rank 0": (second(ranks=(7, 0, 3)), {}, False, (RANK, 1, 0, 0)),
    "rank 65": (second(ranks=(65, 3, 3)), {}, False, (RANK, 1, 65, 0)),
    "H = 0": (second(H=0), {}, False, (SIZE, 1, 0, W0)),
    "1x1": (second(H=1, W=1), {}, False, (GEOM, 1, 1, 1)),
    "u_len one short": (second(), {"u_len": 2 * NU - 1}, False, (U_EXTENT, 1, 2 * NU - 1, 0)),
    "v_len one short": (second(), {"v_len": 2 * NV - 1}, False, (V_EXTENT, 1, 2 * NV - 1, 0)),
    "u_off one past": (second(u_off=NU + 1), {}, False, (U_EXTENT, 1, 2 * NU, 0)),
    "v_off = -1": (second(v_off=-1), {}, False, (NEGATIVE, 1, 0, 0)),
    "u_off = 2^63 - 1": (second(u_off=2 ** 63 - 1), {}, False, (U_EXTENT, 1, 2 * NU, 0)),
    "H = 2^31": (second(H=2 ** 31), {}, False, (SIZE, 1, 2 ** 31, W0)),
    "W = 2^31": (second(W=2 ** 31), {}, False, (SIZE, 1, H0, 2 ** 31)),
    "rgb_len one short": (second(), {"rgb_len": 2 * NPX - 1}, True, (RGB_EXTENT, 1, 2 * NPX - 1, 0)),
    "rgb_off = -1": (second(rgb_off=-1), {}, True, (NEGATIVE, 1, 0, 0)),
    "rgb_off one past": (second(rgb_off=NPX + 1), {}, True, (RGB_EXTENT, 1, 2 * NPX, 0)),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_the_first_offender_is_named(lib, name):
    im, lens, with_rgb, want = REFUSALS[name]
    lens = dict({"u_len": 2 * NU, "v_len": 2 * NV, "rgb_len": 2 * NPX}, **lens)
    got, _, _ = describe(lib, [FIRST, im], lens["u_len"], lens["v_len"], lens["rgb_len"] if with_rgb else None)
    assert got == want
    if not with_rgb:  # the image-side checks come before the output's: the same answer with the output check on
        assert describe(lib, [FIRST, im], lens["u_len"], lens["v_len"], lens["rgb_len"])[0] == want
    if want[0] in (SIZE, GEOM, RANK, NEGATIVE):  # checks of the image alone: in front it is found at index 0
        assert describe(lib, [im, FIRST], lens["u_len"], lens["v_len"], lens["rgb_len"] if with_rgb else None)[0] == (want[0], 0) + want[2:]


def test_the_exact_fit_is_accepted(lib):
    for rgb_len in (None, 2 * NPX):
        got, descs, work = describe(lib, [FIRST, second()], 2 * NU, 2 * NV, rgb_len)
        assert got == (OK, 0, 0, 0)
        assert [(d.u_off, d.v_off) for d in descs] == [(0, 0), (NU, NV)]
        assert [d.rgb_off for d in descs] == ([0, NPX] if rgb_len else [0, 0])
    # without the output check rgb_off is neither looked at nor handed on
    got, descs, _ = describe(lib, [FIRST, second(rgb_off=-1)], 2 * NU, 2 * NV)
    assert got == (OK, 0, 0, 0) and descs[1].rgb_off == 0


GEOMETRIES = [(24, 48), (32, 272), (40, 272), (45, 61), (173, 264), (64, 96)]
TRIPLES = [(7, 3, 3), (16, 9, 16), (64, 64, 64)]


@pytest.mark.parametrize("with_rgb", [False, True])
def test_descriptors(lib, with_rgb):
    """one list of every geometry at every triple; with the output check every other image starts at a multiple of 8 bytes"""
    images, uo, vo, ro = [], 0, 0, 0
    for H, W in GEOMETRIES:
        for r in TRIPLES:
            nu, nv, npx = sizes_of(H, W, r)
            images.append((H, W, r, uo, vo, ro))
            uo, vo, ro = uo + nu, vo + nv, ro + (npx + 7) // 8 * 8 + 4
    base = 4096
    got, descs, work = describe(lib, images, uo, vo, ro if with_rgb else None, base if with_rgb else None)
    assert got == (OK, 0, 0, 0)
    kinds = set()
    for (H, W, r, u_off, v_off, rgb_off), d, w in zip(images, descs, work):
        assert (d.u_off, d.v_off, d.H, d.W, d.R0, d.R1, d.R2) == (u_off, v_off, H, W) + r
        assert d.rgb_off == (rgb_off if with_rgb else 0)
        g = ImageGeom()
        assert lib.lrf_test_geom_of(H, W, ctypes.byref(g)) == 0
        assert bytes(d.g) == bytes(g)
        assert d.per_strip == (g.p[0].nw + 31) // 32
        aligned8 = (base + rgb_off) % 8 == 0 if with_rgb else True
        assert (d.kind, d.cls) == w[:2] == classify(H, W, r, aligned8)[:2]
        if d.kind == TILE16:
            units = (H // 16) * d.per_strip
        elif d.kind == STRIP:
            units = ((g.p[0].nh + 1) // 2) * d.per_strip
        else:
            units = H * ((W + 3) // 4)
        assert w[2] == units == classify(H, W, r, aligned8)[2]
        kinds.add(d.kind)
        mirror = RaggedDesc()  # zeroed
        mirror.g = g
        mirror.u_off, mirror.v_off, mirror.rgb_off, mirror.H, mirror.W = d.u_off, d.v_off, d.rgb_off, d.H, d.W
        mirror.R0, mirror.R1, mirror.R2, mirror.kind, mirror.cls, mirror.per_strip = d.R0, d.R1, d.R2, d.kind, d.cls, d.per_strip
        assert bytes(d) == bytes(mirror)
    assert kinds == {TILE16, STRIP, R8, ANY}
    if with_rgb:  # 64x96 and 32x272 at a tiled triple: the 16-aligned body where the output is aligned, the strip body elsewhere
        by_alignment = {((base + im[5]) % 8 == 0, d.kind) for im, d in zip(images, descs) if im[:2] in ((64, 96), (32, 272)) and im[2] != (64, 64, 64)}
        assert by_alignment == {(True, TILE16), (False, STRIP)}
    # the descriptors do not depend on whether the work list is asked for
    again = describe(lib, images, uo, vo, ro if with_rgb else None, base if with_rgb else None, want_work=False)[1]
    assert bytes(again) == bytes(descs)


def test_the_no_tiled_switch_reaches_the_descriptors(lib):
    got, descs, work = describe(lib, [FIRST], NU, NV, no_tiled=True)
    assert got == (OK, 0, 0, 0) and (descs[0].kind, work[0]) == (R8, (R8, 0, H0 * ((W0 + 3) // 4)))
